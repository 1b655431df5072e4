"""The corpus of FLGPU_FEO_JPEG_PROGRESSIVE, shared by tests/test_jpeg_progressive_host.py (CPU) and tests/test_jpeg_progressive.py (GPU):
the smallest pictures at which each part of the coder can go wrong.  The kernels' constants decide the edges: 16 blocks per wave and 32
per workgroup in the statistics and coding grids, 256 blocks per step of the run resolution, 512 records per round of the pack kernel
and its window of 262,144 bits, 32,767 blocks per end-of-band run.  (name, picture, quality); pictures and model files are built once
per process."""
import functools

import numpy as np

import jpeg_opt_cases as opt_cases
import synth
import test_jpeg_unit_coder as uc

ROW_BLOCKS = (15, 16, 17, 31, 32, 33, 65)
ROW_PERIODS = (1, 2, 17, 33)
RUN_LENGTHS = tuple(sorted({n for k in range(1, 11) for n in ((1 << k) - 1, 1 << k)} | {1, 2}))   # 1, 2, 3, 4, 7, 8, .. 1023, 1024
RUNS_BX = 64
LIMIT_SHAPES = ((1208, 1736), (1024, 2048), (2040, 2056))      # flat pictures of 32,767, 32,768 and 65,535 blocks
PHOTO_QUALITIES = (1, 30, 75, 100)
FLAT = (90, 140, 200)


def _noise_block(k):
    return synth.uniform(8, 8, 3, index=100 + k % 7)


def _strip(busy, q=75):
    """One row of blocks: flat where busy[i] is false, noise where it is true."""
    img = np.empty((8, 8 * len(busy), 3), np.uint8)
    img[:] = FLAT
    for i, b in enumerate(busy):
        if b:
            img[:, 8 * i:8 * i + 8] = _noise_block(i)
    return img


def _closer(oracle, q=50):
    """A block whose every band ends in a non-zero coefficient: it closes a run and starts none."""
    return uc._block(oracle, q, {5: 1, 63: 1}, {63: 1}, {63: -1})


def _runs(oracle):
    """Flat strips of every length in RUN_LENGTHS, each closed by _closer; the rest of the last row is one more run, to the scan's end."""
    total = sum(RUN_LENGTHS) + len(RUN_LENGTHS)
    by = (total + RUNS_BX - 1) // RUNS_BX
    blocks, at, closer = {}, 0, _closer(oracle)
    for n in RUN_LENGTHS:
        at += n
        blocks[at] = closer
        at += 1
    return uc._tile(blocks, RUNS_BX, by, fill=FLAT)


def _band_ends(oracle):
    units = {0: {0: {5: 1}}, 2: {0: {6: -1}}, 4: {0: {63: 1}}, 6: {0: {5: -1, 6: 1}}, 8: {1: {63: -1}}, 10: {2: {63: 1}}, 12: {0: {1: 1, 5: -1}},
             13: {0: {4: 1}, 1: {62: 1}}, 15: {0: {6: 1, 63: -1}, 1: {1: 1, 63: 1}, 2: {17: 1}}, 17: {0: {22: 1}, 2: {1: -1}}, 23: {0: {63: -1}, 1: {63: 1}, 2: {63: 1}}}
    return uc._build(oracle, "band_ends", 50, units)


def _fold(oracle):
    """The _OPTIMIZE corpus' chain of 17 symbols in Cb, whose scan covers 1-63 as the baseline's does: every block holds a coefficient
    and ends in a zero, so each end-of-band run is one block long and EOB0 takes the end-of-block code's count."""
    units = opt_cases.fold_units()
    return uc._tile({b: uc._block(oracle, opt_cases.FOLD_Q, None, c.get(0)) for b, c in units.items()}, opt_cases.FOLD_BX, opt_cases.FOLD_BY)


def _flat(h, w):
    img = np.empty((h, w, 3), np.uint8)
    img[:] = FLAT
    return img


def _row_name(nb, period):
    return f"row_{nb}_blocks_period_{period}"


_BUILDERS = {}
_BUILDERS["photo_1x1_c3_q75"] = lambda o: (synth.photo(1, 1, 3, index=1), 75)
_BUILDERS["flat_8x8_q75"] = lambda o: (_flat(8, 8), 75)
_BUILDERS["photo_9x7_c4_q1"] = lambda o: (synth.photo(7, 9, 4, index=3), 1)
_BUILDERS["photo_17x17_c2_q50"] = lambda o: (synth.photo(17, 17, 2, index=6), 50)
_BUILDERS["photo_33x17_c1_q75"] = lambda o: (synth.photo(17, 33, 1, index=8), 75)
for _nb in ROW_BLOCKS:
    for _p in ROW_PERIODS:
        _BUILDERS[_row_name(_nb, _p)] = lambda o, nb=_nb, p=_p: (_strip([(i // p) % 2 == 1 for i in range(nb)]), 75)
_BUILDERS["run_lengths_q50"] = lambda o: (_runs(o), 50)
_BUILDERS["ends_busy_q75"] = lambda o: (_strip([False, False, False, True]), 75)
_BUILDERS["ends_in_run_q75"] = lambda o: (_strip([True, False, False, False]), 75)
_BUILDERS["band_ends_q50"] = lambda o: (_band_ends(o), 50)
for _h, _w in LIMIT_SHAPES:
    _BUILDERS[f"flat_{_w}x{_h}_q75"] = lambda o, h=_h, w=_w: (_flat(h, w), 75)
_BUILDERS["noise_32x32_q100"] = lambda o: (synth.uniform(32, 32, 3, index=9), 100)
_BUILDERS["noise_128x128_q100"] = lambda o: (synth.uniform(128, 128, 3, index=12), 100)
_BUILDERS["noise_256x256_q100"] = lambda o: (synth.uniform(256, 256, 3, index=13), 100)   # (the 128 x 128 picture's longest scan is 15,691 bytes)
_BUILDERS["fold_cb_256x176_q75"] = lambda o: (_fold(o), opt_cases.FOLD_Q)
for _q in PHOTO_QUALITIES:
    _BUILDERS[f"photo_83x61_c4_q{_q}"] = lambda o, q=_q: (synth.photo(61, 83, 4, index=5), q)
    _BUILDERS[f"photo_300x200_q{_q}"] = lambda o, q=_q: (synth.photo(200, 300, 3, index=3), q)

NAMES = list(_BUILDERS)
LARGE = [f"flat_{w}x{h}_q75" for h, w in LIMIT_SHAPES]


@functools.lru_cache(maxsize=None)
def get(oracle, name):
    return _BUILDERS[name](oracle)


@functools.lru_cache(maxsize=None)
def model(oracle, name):
    """(file, info) of the model for a corpus case, computed once"""
    import jpeg_prog_model as pm
    img, q = get(oracle, name)
    return pm.encode(oracle, img, q)


def eob_runs(info, scan):
    """The end-of-band run lengths AC scan `scan` (1 .. 4) codes, in order"""
    return [(1 << (s >> 4)) + v for _, s, v, _ in info["scans"][scan] if (s & 15) == 0 and s != 0xF0]


def check_conditions(oracle):
    """What the corpus is there to reach, asserted on the model."""
    runs = model(oracle, "run_lengths_q50")[1]
    for scan in (1, 2, 3, 4):
        got = eob_runs(runs, scan)
        assert tuple(got[:-1]) == RUN_LENGTHS and got[-1] == RUNS_BX - (sum(RUN_LENGTHS) + len(RUN_LENGTHS)) % RUNS_BX, (scan, got)
    for (h, w), name in zip(LIMIT_SHAPES, LARGE):
        n = (h // 8) * (w // 8)
        want = [32767] * (n // 32767) + ([n % 32767] if n % 32767 else [])
        info = model(oracle, name)[1]
        assert all(eob_runs(info, scan) == want for scan in (1, 2, 3, 4)), name
    assert all(eob_runs(model(oracle, "flat_8x8_q75")[1], scan) == [1] and len(model(oracle, "flat_8x8_q75")[1]["scans"][scan]) == 1 for scan in (1, 2, 3, 4))
    busy, idle = model(oracle, "ends_busy_q75")[1], model(oracle, "ends_in_run_q75")[1]
    for scan in (1, 2, 3, 4):
        assert busy["scans"][scan][0][1] == 0x10 and busy["scans"][scan][0][2] == 1, "a run of three in front of the last block"
        assert (idle["scans"][scan][-1][1] & 15) == 0 and eob_runs(idle, scan)[-1] >= 3, "the scan ends in a run"
    # runs that start and end on both sides of the wave and workgroup edges
    starts = set()
    for nb in ROW_BLOCKS:
        for p in ROW_PERIODS:
            info = model(oracle, _row_name(nb, p))[1]
            assert len(info["scans"][0]) == 3 * nb
            if p < nb:
                starts.update(range(0, nb, 2 * p))
    assert {0, 16, 32, 64} <= starts and {15, 17, 31, 33} & {s + p for p in ROW_PERIODS for s in starts}
    ends = model(oracle, "band_ends_q50")[1]
    assert sum(s == 0xF0 for _, s, _, _ in ends["scans"][4]) >= 6 and any(s == 0xF0 for _, s, _, _ in ends["scans"][2]), "ZRL x 3 in front of coefficient 63"
    coef = oracle.jpeg_coefficients(*get(oracle, "band_ends_q50")).reshape(-1, 3, 64)
    assert np.nonzero(coef[0, 0, 1:])[0].tolist() == [4] and np.nonzero(coef[2, 0, 1:])[0].tolist() == [5] and np.nonzero(coef[4, 0, 1:])[0].tolist() == [62]
    assert np.nonzero(coef[23, :, 1:])[1].tolist() == [62, 62, 62]
    sizes = [len(s) for s in _scan_bytes(model(oracle, "noise_256x256_q100")[0])]
    assert min(sizes[2:]) > 32768 > max(sizes[:2]), "scans longer than one pack window, and scans that start in the middle of one"
    fold = model(oracle, "fold_cb_256x176_q75")[1]
    assert fold["rules"][3]["folded"] and max(fold["rules"][3]["lengths"].values()) == 16


def _scan_bytes(data):
    """The entropy-coded bytes of every scan of a file"""
    out, at = [], 2
    while data[at + 1] != 0xD9:
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        at += 2 + n
        if marker == 0xDA:
            end = at
            while not (data[end] == 0xFF and data[end + 1] != 0):
                end += 1
            out.append(data[at:end])
            at = end
    return out
