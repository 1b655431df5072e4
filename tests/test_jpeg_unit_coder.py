"""JPEG encoder: the AC coder of jpeg_dct_quant_kernel, one lane per unit (a unit = one component of one 8x8 block).

A wave transforms 16 consecutive blocks, then lane 16 k + b codes component k of block b; a workgroup holds two such waves.  The pictures here are built to hit the coder's edges: zero runs that need one, two and three ZRL codes,
a non-zero coefficient 63 (no end-of-block code), units with all 63 AC terms non-zero (the longest unit), DC-only units, one
busy lane among idle ones, and block counts around the wave and workgroup sizes.  The CPU tests prove with the oracle's
quantised coefficients that each picture holds the pattern it was built for; the GPU tests compare streams byte for byte."""
import numpy as np
import pytest

import synth

B = 16            # blocks per wave
WG = 2 * B        # blocks per workgroup

_k = np.arange(8)
_BASIS = np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16) * np.where(_k[:, None] == 0, np.sqrt(0.5), 1.0) * 0.5
_UNZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                      28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                      54, 47, 55, 62, 63])


def _plane(coefs, qtab):
    """8x8 samples (float) whose quantised coefficients are `coefs` {zig-zag position: value} around a DC of 128."""
    f = np.zeros(64)
    for zz, v in coefs.items():
        f[_UNZIGZAG[zz]] = v * float(qtab[_UNZIGZAG[zz]])
    return 128.0 + _BASIS.T @ f.reshape(8, 8) @ _BASIS


def _block(oracle, q, y=None, cb=None, cr=None):
    """An 8x8 RGB block with the given coefficients per component (JFIF YCbCr -> RGB, rounded)."""
    luma, chroma = oracle.jpeg_qtables(q)
    Y = _plane(y or {}, luma)
    Cb = _plane(cb or {}, chroma) - 128.0
    Cr = _plane(cr or {}, chroma) - 128.0
    rgb = np.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], axis=2)
    assert rgb.min() >= -0.5 and rgb.max() <= 255.5, "pattern block clips"
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def _tile(blocks, bx, by, fill=(128, 128, 128)):
    """A picture of by x bx blocks; `blocks` maps block index -> 8x8x3 block, every other block is flat `fill`."""
    img = np.empty((by * 8, bx * 8, 3), np.uint8)
    img[:, :] = np.array(fill, np.uint8)
    for i, blk in blocks.items():
        r, c = divmod(i, bx)
        img[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = blk
    return img


def _all_ac(seed):
    rng = np.random.default_rng(seed)
    return {zz: int(rng.choice([-1, 1])) * int(rng.integers(2, 4)) for zz in range(1, 64)}


# (name, quality, {block index: {component: {zig-zag position: value}}}, what the named units must look like)
def _patterns():
    pats = []
    for comp in range(3):
        units = {}
        for j, zz in enumerate((17, 33, 49, 18, 34, 50)):           # runs of 16, 32, 48 (1, 2, 3 ZRLs), then 17, 33, 49
            units[2 * j] = {comp: {zz: (-1) ** j}}
        units[13] = {comp: {63: -1}}                              # only coefficient 63: three ZRLs, run 14, no EOB
        units[15] = {comp: {1: 1, 63: 1}}                         # a run of 61 behind coefficient 1, no EOB
        units[17] = {comp: {16: 1, 32: -1, 48: 1, 63: 1}}         # one ZRL in front of 32 and 48, run 14 in front of 63
        pats.append((f"zrl_eob_c{comp}", 50, units))
    pats.append(("all_ac", 100, {i: {0: _all_ac(3 * i), 1: _all_ac(3 * i + 1), 2: _all_ac(3 * i + 2)} for i in range(0, 12, 3)}))
    return pats


def _build(oracle, name, q, units, bx=8, by=3):
    return _tile({i: _block(oracle, q, c.get(0), c.get(1), c.get(2)) for i, c in units.items()}, bx, by)


def _busy_lanes(oracle):
    """One busy block per wave at each of the B positions: wave j's busy block is its block j."""
    bx, by = B + 1, B
    busy = _block(oracle, 75, {zz: (-1) ** (zz // 2) for zz in range(1, 64, 2)}, {5: 1, 40: -1}, {63: 1})
    return _tile({j * B + j: busy for j in range(B)}, bx, by), 75


def _dc_only(oracle):
    """Non-flat blocks whose every unit quantises to DC alone (they take the transform, not the flat-block shortcut)."""
    rng = np.random.default_rng(11)
    img = np.clip(rng.integers(-1, 2, (24, 40, 3)) + np.array([60, 140, 200]), 0, 255).astype(np.uint8)
    return img, 20


# ----------------------------------------------------------------------------- CPU: the pictures hold their patterns --

@pytest.mark.parametrize("idx", range(4))
def test_pattern_pictures_hold_their_coefficients(oracle, idx):
    name, q, units = _patterns()[idx]
    img = _build(oracle, name, q, units)
    coef = oracle.jpeg_coefficients(img, q).reshape(-1, 3, 64)
    for i, comps in units.items():
        for comp, want in comps.items():
            got = coef[i, comp]
            nz = {int(k): int(got[k]) for k in np.nonzero(got[1:])[0] + 1}
            if name == "all_ac":                                  # (rounding to bytes may move a value by one, never to zero)
                nz = {k: want[k] for k in nz if abs(nz[k] - want[k]) <= 1}
            assert nz == want, f"{name}: block {i} component {comp}: {nz} != {want}"


def test_pattern_pictures_cover_every_edge(oracle):
    runs, no_eob, full = set(), [0, 0, 0], [0, 0, 0]
    for name, q, units in _patterns():
        coef = oracle.jpeg_coefficients(_build(oracle, name, q, units), q).reshape(-1, 3, 64)
        for blk in coef:
            for comp in range(3):
                pos = np.nonzero(blk[comp][1:])[0] + 1
                prev = 0
                for p in pos:
                    runs.add((comp, (int(p) - prev - 1) // 16))
                    prev = int(p)
                no_eob[comp] += int(blk[comp][63] != 0)
                full[comp] += int(len(pos) == 63)
    for comp in range(3):
        assert {(comp, 1), (comp, 2), (comp, 3)} <= runs, f"component {comp} lacks 1, 2 or 3 ZRLs"
        assert no_eob[comp] >= 3 and full[comp] >= 4


def test_busy_lane_and_dc_only_pictures(oracle):
    img, q = _busy_lanes(oracle)
    coef = oracle.jpeg_coefficients(img, q).reshape(-1, 3, 64)
    busy = [i for i in range(len(coef)) if np.any(coef[i, :, 1:])]
    assert busy == [j * B + j for j in range(B)]
    assert all(np.count_nonzero(coef[i, 0, 1:]) >= 30 for i in busy)
    img, q = _dc_only(oracle)
    coef = oracle.jpeg_coefficients(img, q).reshape(-1, 3, 64)
    assert not np.any(coef[:, :, 1:])
    assert all(len(np.unique(img[r:r + 8, c:c + 8].reshape(-1, 3), axis=0)) > 1 for r in range(0, 24, 8) for c in range(0, 40, 8))


# ----------------------------------------------------------------------------- GPU: streams equal the oracle's --

def gpu_jpeg(fl, st, img, q):
    return st.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_JPEG), capacity=img.shape[0] * img.shape[1] * 16 + 4096)


def _same(got, want):
    return got == want, f"{len(got)} vs {len(want)} bytes, first difference at {next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)}"


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(4))
def test_gpu_pattern_pictures(fl, gpu_state, oracle, idx):
    name, q, units = _patterns()[idx]
    img = _build(oracle, name, q, units)
    for qq in sorted({q, 50, 100}):
        ok, msg = _same(gpu_jpeg(fl, gpu_state, img, qq), oracle.jpeg_encode(img, qq))
        assert ok, f"{name} q {qq}: {msg}"


@pytest.mark.gpu
def test_gpu_busy_lane_and_dc_only(fl, gpu_state, oracle):
    for img, q in (_busy_lanes(oracle), _dc_only(oracle)):
        ok, msg = _same(gpu_jpeg(fl, gpu_state, img, q), oracle.jpeg_encode(img, q))
        assert ok, msg


@pytest.mark.gpu
@pytest.mark.parametrize("nblocks", [1, B - 1, B, B + 1, WG - 1, WG, WG + 1, 3 * B - 1, 3 * B, 3 * B + 1, 2 * WG - 1, 2 * WG, 2 * WG + 1])
def test_gpu_block_counts_around_the_wave(fl, gpu_state, oracle, nblocks):
    img = synth.photo(8, 8 * nblocks, 3, index=nblocks)                    # one row of blocks
    for q in (30, 100):
        ok, msg = _same(gpu_jpeg(fl, gpu_state, img, q), oracle.jpeg_encode(img, q))
        assert ok, f"{nblocks} blocks q {q}: {msg}"
    tall = synth.uniform(8 * nblocks, 5, 3, index=nblocks)                 # one column of partial blocks
    ok, msg = _same(gpu_jpeg(fl, gpu_state, tall, 90), oracle.jpeg_encode(tall, 90))
    assert ok, f"{nblocks} x 1 blocks: {msg}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (8, 8), (7, 9), (16, 8 * B - 3)])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_gpu_small_pictures_and_channels(fl, gpu_state, oracle, shape, channels):
    for q, img in ((75, synth.photo(*shape, channels, index=channels)), (100, synth.uniform(*shape, channels, index=channels))):
        ok, msg = _same(gpu_jpeg(fl, gpu_state, img, q), oracle.jpeg_encode(img, q))
        assert ok, f"{shape} x {channels} q {q}: {msg}"


@pytest.mark.gpu
def test_gpu_batch_of_mixed_sizes(fl, gpu_state, oracle):
    # one launch: the grid is sized by the largest picture, the others leave most of their workgroups idle
    shapes = [(200, 300, 4), (8, 8, 3), (1, 1, 3), (33, 17, 1), (64, 8 * WG + 8, 3), (96, 40, 4), (8, 8 * B, 3)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(*s, index=40 + i) for i, s in enumerate(shapes)]
    qs = [75, 100, 50, 90, 100, 30, 100]
    outs = gpu_state.process_batch(imgs, [fl.make_params(quality=q, front_end=fl.FE_JPEG) for q in qs])
    for i, (img, q) in enumerate(zip(imgs, qs)):
        ok, msg = _same(outs[i], oracle.jpeg_encode(img, q))
        assert ok, f"job {i} {img.shape} q {q}: {msg}"
