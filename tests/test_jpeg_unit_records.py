"""JPEG encoder: the 16-byte unit record between jpeg_dct_quant_kernel and jpeg_pack_kernel.

A unit (one component of one 8x8 block) hands the pack kernel one record: its meta word and the first 96 bits of its AC code;
what lies beyond 96 bits stays in the unit's slot of the AC scratch.  The pictures here put AC codes of 0, 31..33, 63..65,
95..97 and more than 128 bits into luma and into chroma units -- every word boundary of the record from both sides and the
step into the scratch slot -- with test_jpeg_unit_coder's construction: coefficients of +-1 and +-2 planted at quality 50 at
zig-zag positions 1..n, every other block flat.  With the Annex K tables a run-0 size-1 coefficient costs 3 bits, a size-2 one
4 (luma) or 5 (chroma) bits and the end-of-block code 4 (luma) or 2 (chroma) bits, which gives the mixes of _MIXES.  A chroma
pattern of 20 and more coefficients at quality 50 leaves the RGB cube when the block's luma is flat (B = Y + 1.772 Cb), so the
luma of such a block carries -0.714 times the Cb (-0.344 times the Cr) pattern: R, G and B then move by at most 1.058 times the
pattern, and the block's luma unit simply has an AC code of its own.  The signs are the best of a seeded search for a small
peak.  The CPU test proves with the oracle's quantised coefficients and the code lengths of the oracle's own DHT segments that
each count is there; the GPU tests compare streams byte for byte."""
import functools

import numpy as np
import pytest

import jpeg_surgery
import synth
from test_jpeg_unit_coder import _BASIS, _UNZIGZAG, _same, _tile, gpu_jpeg

Q = 50
COUNTS = (31, 32, 33, 63, 64, 65, 95, 96, 97)
# AC bits -> (coefficients of size 1, of size 2): luma 3 n1 + 4 n2 + 4, chroma 3 n1 + 5 n2 + 2; the last one is "above 128"
_MIXES = {
    "luma": {31: (9, 0), 32: (8, 1), 33: (7, 2), 63: (17, 2), 64: (20, 0), 65: (19, 1), 95: (29, 1), 96: (28, 2), 97: (31, 0), 139: (45, 0)},
    "chroma": {31: (8, 1), 32: (10, 0), 33: (7, 2), 63: (17, 2), 64: (19, 1), 65: (21, 0), 95: (16, 9), 96: (18, 8), 97: (20, 7), 129: (34, 5)},
}
BX = 8                      # blocks per row of the boundary picture
HEADER = 623                # bytes in front of the scan data
WINDOW = 32 * 1024          # the pack kernel's LDS window of the stream


def _pattern(qtab, n1, n2, seed, trials=20000):
    """8x8 samples (float, zero mean): +-2 at zig-zag positions 1..n2, +-1 at the n1 positions behind them, times the
    quantiser's steps; of `trials` seeded sign choices the one with the smallest peak."""
    n = n1 + n2
    amp = np.array([(2.0 if z <= n2 else 1.0) * float(qtab[_UNZIGZAG[z]]) for z in range(1, n + 1)])
    basis = np.stack([np.outer(_BASIS[_UNZIGZAG[z] // 8], _BASIS[_UNZIGZAG[z] % 8]).ravel() for z in range(1, n + 1)])
    signs = np.random.default_rng(seed).choice([-1.0, 1.0], (trials, n))
    s = (signs * amp) @ basis
    return s[np.argmin(np.abs(s).max(axis=1))].reshape(8, 8)


def _pattern_block(oracle, comp, n1, n2, seed):
    luma, chroma = oracle.jpeg_qtables(Q)
    Y, Cb, Cr = np.full((8, 8), 128.0), np.zeros((8, 8)), np.zeros((8, 8))
    if comp == 0:
        Y = Y + _pattern(luma, n1, n2, seed)
    elif comp == 1:
        Cb = _pattern(chroma, n1, n2, seed)
        Y = Y - 0.714 * Cb
    else:
        Cr = _pattern(chroma, n1, n2, seed)
        Y = Y - 0.344 * Cr
    rgb = np.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], axis=2)
    assert rgb.min() >= -0.5 and rgb.max() <= 255.5, "pattern block clips"
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _boundary_blocks():
    """[(component, AC bits the block was built for, 8x8x3 block)]: every count for Y, Cb and Cr."""
    import oracle_lib
    oracle = oracle_lib.load()
    out = []
    for comp in range(3):
        for bits, (n1, n2) in _MIXES["luma" if comp == 0 else "chroma"].items():
            out.append((comp, bits, _pattern_block(oracle, comp, n1, n2, seed=100 * comp + bits)))
    return out


def _boundary_picture():
    """The pattern blocks with a flat block behind every third of them: 30 pattern blocks among 40."""
    blocks, i = {}, 0
    for _, _, blk in _boundary_blocks():
        blocks[i] = blk
        i += 2 if i % 4 == 2 else 1
    assert i <= 5 * BX
    return _tile(blocks, BX, 5), blocks


def _second_window_picture():
    """A 96 x 96 noise field, then the boundary picture's blocks in the same order: at quality 100 the noise fills the first
    32 KB window of the stream and more."""
    _, blocks = _boundary_picture()
    bx = 12
    img = _tile({12 * bx + i: blk for i, blk in blocks.items()}, bx, 12 + 4)
    img[:96] = np.random.default_rng(5).integers(0, 256, (96, 96, 3), dtype=np.uint8)
    return img


def _ac_code_lengths(stream):
    """{table id: {symbol: code length}} of the AC tables in the stream's DHT segments."""
    out = {}
    for m, p in jpeg_surgery.segments(stream)[0]:
        o = 0
        while m == jpeg_surgery.DHT and o < len(p):
            tc, th, counts = p[o] >> 4, p[o] & 15, list(p[o + 1:o + 17])
            vals = p[o + 17:o + 17 + sum(counts)]
            if tc == 1:
                out[th] = dict(zip(vals, [l + 1 for l in range(16) for _ in range(counts[l])]))
            o += 17 + len(vals)
    return out


def _ac_bits(unit, lengths):
    """Bits of BitWriter::write_block's AC part for one unit's 64 zig-zag coefficients."""
    bits, prev = 0, 0
    for pos in np.nonzero(unit[1:])[0] + 1:
        run = int(pos) - prev - 1
        prev = int(pos)
        bits += (run // 16) * lengths[0xF0]
        size = int(abs(int(unit[pos]))).bit_length()
        bits += lengths[((run % 16) << 4) | size] + size
    return bits + (lengths[0x00] if prev != 63 else 0)


# ----------------------------------------------------------------------------- CPU: the pictures hold their counts --

def test_boundary_picture_holds_every_count(oracle):
    img, blocks = _boundary_picture()
    lengths = _ac_code_lengths(oracle.jpeg_encode(img, Q))
    assert sorted(lengths) == [0, 1]
    coef = oracle.jpeg_coefficients(img, Q).reshape(-1, 3, 64)
    assert len(coef) == 5 * BX
    got = {c: [_ac_bits(coef[i, c], lengths[0 if c == 0 else 1]) for i in range(len(coef))] for c in range(3)}
    print("AC bits per unit:", got)
    # every block holds what it was built for, in the component it was built for
    for i, (comp, bits, _) in zip(sorted(blocks), _boundary_blocks()):
        assert got[comp][i] == bits, f"block {i} component {comp}: {got[comp][i]} bits, built for {bits}"
    for c in range(3):
        have = set(got[c])
        for want in COUNTS:
            assert want in have, f"component {c}: no unit of {want} AC bits"
        assert max(have) > 128, f"component {c}: no unit above 128 AC bits"
        # the flat blocks: no AC term at all, so the unit's whole AC code is the end-of-block code (0 bits of coefficients)
        eob = lengths[0 if c == 0 else 1][0x00]
        flat = [i for i in range(len(coef)) if not np.any(coef[i, c, 1:])]
        assert flat and all(got[c][i] == eob for i in flat) and min(have) == eob


def test_second_window_picture_is_long_enough(oracle):
    img = _second_window_picture()
    stream = oracle.jpeg_encode(img, 100)
    assert len(stream) > WINDOW + HEADER
    # ... and the noise alone already is: the boundary blocks lie in the second window
    assert len(oracle.jpeg_encode(img[:96], 100)) > WINDOW + HEADER + 2


# ----------------------------------------------------------------------------- GPU: streams equal the oracle's --

ROUND_BLOCKS = (170, 171, 341, 342, 1023, 1025)      # 510, 513, 1023, 1026, 3069, 3075 units: around the rounds of 512 threads


@pytest.mark.gpu
def test_gpu_boundary_picture(fl, gpu_state, oracle):
    img, _ = _boundary_picture()
    ok, msg = _same(gpu_jpeg(fl, gpu_state, img, Q), oracle.jpeg_encode(img, Q))
    assert ok, msg


@pytest.mark.gpu
def test_gpu_boundary_blocks_in_the_second_window(fl, gpu_state, oracle):
    img = _second_window_picture()
    ok, msg = _same(gpu_jpeg(fl, gpu_state, img, 100), oracle.jpeg_encode(img, 100))
    assert ok, msg


@pytest.mark.gpu
@pytest.mark.parametrize("nblocks", ROUND_BLOCKS)
def test_gpu_unit_counts_around_the_pack_rounds(fl, gpu_state, oracle, nblocks):
    img = synth.photo(8, 8 * nblocks, 3, index=nblocks)
    ok, msg = _same(gpu_jpeg(fl, gpu_state, img, 75), oracle.jpeg_encode(img, 75))
    assert ok, f"{nblocks} blocks: {msg}"


@pytest.mark.gpu
def test_gpu_mixed_batch_keeps_record_offsets(fl, gpu_state, oracle):
    imgs = [_boundary_picture()[0], _second_window_picture(), synth.photo(1, 1, 3, index=7), synth.photo(200, 300, 4, index=8)]
    qs = [Q, 100, 75, 75]
    outs = gpu_state.process_batch(imgs, [fl.make_params(quality=q, front_end=fl.FE_JPEG) for q in qs])
    for i, (img, q) in enumerate(zip(imgs, qs)):
        ok, msg = _same(outs[i], gpu_jpeg(fl, gpu_state, img, q))
        assert ok, f"job {i} {img.shape}: in the batch and alone: {msg}"
        ok, msg = _same(outs[i], oracle.jpeg_encode(img, q))
        assert ok, f"job {i} {img.shape}: {msg}"
