"""Pictures for the tests of the lossless WebP encoder (csrc/fl_webpll.hip), written from construction: a case states the residual
stream it wants (tests/vp8l_model.py `residuals`: a, r - g, g, b - g against L on row 0, T below, black at the origin), and
`from_residuals` gives the picture that has it.  The request the device tests use is the identity, so the picture IS the encoder's
input and the properties below (where runs start and end against the tile of 4096 pixels, the thread's 16 and the period of 4097,
how many tiles, which code lengths) are properties of the case.  Every case is (name, picture, property); the property asserts on
vm.residuals / vm.tokens / vm.histograms / vm.parse(vm.encode(px)) what makes the case an edge, and tests/test_webp_lossless_edges.py
checks it on the host before the device is asked anything.

A run (s, L) below is a literal at pixel s and the L pixels behind it that repeat it: one backward reference of length L where
L <= 4096, and beyond that a forced reference of 4096, a literal, and so on with period 4097."""
import numpy as np

import vp8l_model as vm

TILE, THREAD, PERIOD = 4096, 16, vm.MAX_RUN + 1


def from_residuals(res, w, h, c=4):
    """The inverse of vm.residuals: the (h, w, c) picture whose residual stream is res ((w h, 4): a, r - g, g, b - g).  Sums mod 256
    along row 0 from ARGB black, then down the columns, then green added back.  c < 4 only where the stream allows it: no alpha
    residual for c = 1 and 3, no red or blue one for c = 1 and 2."""
    argb = np.asarray(res, np.uint8).reshape(h, w, 4).astype(np.int64)
    argb[0, 0, 0] += 255
    argb[0] = np.cumsum(argb[0], axis=0)
    argb = np.cumsum(argb, axis=0) & 255
    a, r, g, b = (argb[..., k] for k in range(4))
    if c >= 3:
        assert c == 4 or (a == 255).all(), "an alpha residual in an opaque picture"
        return np.stack([(r + g) & 255, g, (b + g) & 255, a][:c], axis=-1).astype(np.uint8)
    assert not r.any() and not b.any(), "a red or blue residual in a grey picture"
    assert c == 2 or (a == 255).all(), "an alpha residual in an opaque picture"
    return np.stack([g, a][:c], axis=-1).astype(np.uint8)


def filler(n, c, seed):
    """n literals, each different from its neighbours (the green residual steps by 37), every green value used once n >= 256; only
    the channels a picture of c channels can express."""
    rng = np.random.default_rng(seed)
    res = np.zeros((n, 4), np.uint8)
    res[:, 2] = (np.arange(n) * 37 + 11) & 255
    if c >= 3:
        res[:, 1], res[:, 3] = rng.integers(0, 256, n), rng.integers(0, 256, n)
    if c in (2, 4):
        res[:, 0] = rng.integers(0, 256, n)
    return res


def run_tuple(k, c):
    """the k-th run's own residual tuple (k < 255), never zero"""
    t = np.array([k + 1, 3 * k + 7, 53 * k + 1, 5 * k + 2], np.int64) & 255
    if c < 3:
        t[1] = t[3] = 0
        t[2] = k + 1
    if c in (1, 3):
        t[0] = 0
    return t.astype(np.uint8)


def expected_m(n, runs):
    """vm.tokens' m for n pixels that are literals but for the runs"""
    m = np.zeros(n, np.int64)
    for s, L in runs:
        m[s:s + L + 1] = np.arange(L + 1) % PERIOD
    return m


def run_stream(n, runs, c=4, zero=False):
    """n residuals: filler but for the runs; a run's tuple is its own, or zero for every run (zero is what the kernels' missing
    neighbours read as)."""
    res = filler(n, c, seed=n + c)
    for k, (s, L) in enumerate(sorted(runs)):
        assert 0 <= s and s + L < n
        t = np.zeros(4, np.uint8) if zero else run_tuple(k, c)
        res[s:s + L + 1] = t
        for nb in (s - 1, s + L + 1):
            if 0 <= nb < n and (res[nb] == t).all():
                res[nb, 2] += 1
    assert np.array_equal(vm.tokens(res)[2], expected_m(n, runs)), "the runs interact"
    return res


def shape_for(last, w=97):
    """(w, h) of the smallest picture of width w (no tile is a multiple of it) with a literal behind pixel `last`"""
    return w, (last + 2 + w - 1) // w


def pixel_bits(px, data):
    """bits of every pixel's token in the model's file `data`, and the bit the data start at"""
    hdr = vm.parse(data)
    res = vm.residuals(px)
    lit, ref, m = vm.tokens(res)
    ln = [np.asarray(cd["lengths"] if "lengths" in cd else [0] * vm.ALPHABETS[k], np.int64) for k, cd in enumerate(hdr["codes"][:4])]
    bits = np.zeros(len(res), np.int64)
    bits[lit] = ln[0][res[lit, 2]] + ln[1][res[lit, 1]] + ln[2][res[lit, 3]] + ln[3][res[lit, 0]]
    pc = [vm.prefix_code(int(v)) for v in m[ref]]
    bits[ref] = [ln[0][256 + p[0]] + p[1] for p in pc]
    return bits, hdr["data_bit"]


def run_starts(res):
    key = res.view(np.uint32).reshape(len(res))
    return np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))


CASES = {}     # name -> (build() -> picture, prop(picture))
_PX, _MODEL = {}, {}


def add(name, build, prop):
    assert name not in CASES, name
    CASES[name] = (build, prop)


def get(name):
    if name not in _PX:
        px = CASES[name][0]()
        px.setflags(write=False)
        _PX[name] = px
    return _PX[name]


def model(name):
    """the model's file for the case, made once"""
    if name not in _MODEL:
        _MODEL[name] = vm.encode(get(name))
    return _MODEL[name]


def check(name):
    CASES[name][1](get(name))


# ---- run geometry -------------------------------------------------------------------------------------------------------------
RUN_STARTS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192)
# 4096 equal pixels are a reference of 4095, 4096 copies one of 4096: both readings of "a run of 4096", and 8192 .. 8194 likewise
RUN_LENGTHS = (1, 2, 3, 4095, 4096, 4097, 4098, 8192, 8193, 8194)
RUN_ENDS = (15, 16, 31, 4094, 4095, 4096, 8191)       # ... and short runs given by their last pixel
GRID = [(s, L) for L in RUN_LENGTHS for s in RUN_STARTS] + [(e - L, L) for L in (1, 2, 3) for e in RUN_ENDS]


def pack(pairs):
    """first fit, longest first: the runs of one picture keep at least one literal between them"""
    bins = []
    for s, L in sorted(dict.fromkeys(pairs), key=lambda p: (-p[1], p[0])):
        for b in bins:
            if all(s > s2 + L2 + 1 or s + L + 1 < s2 for s2, L2 in b):
                b.append((s, L))
                break
        else:
            bins.append([(s, L)])
    return [sorted(b) for b in bins]


RUN_PICTURES = pack(GRID)       # the (s, L) pairs of picture "runsNN_*"


def _runs_case(runs, c, zero, shape=None):
    w, h = shape or shape_for(max(s + L for s, L in runs))

    def build():
        return from_residuals(run_stream(w * h, runs, c, zero), w, h, c)

    def prop(px):
        assert px.shape == (h, w, c) and w * h <= 20000
        res = vm.residuals(px)
        lit, ref, m = vm.tokens(res)
        assert np.array_equal(m, expected_m(w * h, runs))
        for s, L in runs:
            assert res[s:s + L + 1].any() != zero and (res[s:s + L + 1] == res[s]).all()
    return build, prop


for _j, _runs in enumerate(RUN_PICTURES):
    add("runs%02d_own" % _j, *_runs_case(_runs, 4, False))
    add("runs%02d_zero" % _j, *_runs_case(_runs, 4, True))


def picture_of(pair):
    return next(j for j, b in enumerate(RUN_PICTURES) if pair in b)


# the same pictures as grey, grey + alpha and opaque (load_argb's into_rgba8 branches under runs)
CHANNEL_PICTURES = sorted({picture_of((4095, 8193)), picture_of((16, 3)), picture_of((4096, 4097))})
for _j in CHANNEL_PICTURES:
    for _c in (1, 2, 3):
        add("runs%02d_own_c%d" % (_j, _c), *_runs_case(RUN_PICTURES[_j], _c, False))


def forced_reference_ends_a_tile(m, flag):
    """pixels i: a reference of 4096 ends on a tile's last pixel and the next tile opens with the run's literal"""
    return np.flatnonzero((m[:-1] == vm.MAX_RUN) & (np.arange(len(m) - 1) % TILE == TILE - 1) & (m[1:] == 0) & ~flag[1:])


def run_ends_on_a_tile(m, flag):
    """pixels i: the last pixel of a tile and of a run that is no forced reference there (only the next tile's first residual says so)"""
    n = len(m)
    return np.flatnonzero((m[:-1] != 0) & (m[:-1] != vm.MAX_RUN) & (np.arange(n - 1) % TILE == TILE - 1) & flag[1:])


def tiles_inside_a_run(m, flag):
    """tiles without a run start whose run started two tiles earlier or more"""
    n = len(m)
    idx = np.arange(n)
    start = np.maximum.accumulate(np.where(flag, idx, 0))
    out = []
    for t in range(n // TILE):
        if not flag[t * TILE:(t + 1) * TILE].any() and start[t * TILE] // TILE <= t - 2:
            out.append(t)
    return out


def flags_of(px):
    res = vm.residuals(px)
    flag = np.zeros(len(res), bool)
    flag[run_starts(res)] = True
    return vm.tokens(res)[2], flag


# 1 x N and N x 1: the last tile holds one pixel (4097, 8193), the last thread 16, 1 and 15 pixels (N mod 16 = 0, 1, 15)
LINE_LENGTHS = (4096, 4097, 8193, 4111, 8207)
assert {n % 16 for n in LINE_LENGTHS} == {0, 1, 15} and {n % TILE for n in LINE_LENGTHS} >= {0, 1}


def _line_case(n, tall, ending):
    # "run": a run of 5 (its tuple its own, or zero) ends on the last pixel; "literal": the last pixel is a literal behind a run
    runs = [(40, 3), (n - 6, 5)] if ending != "literal" else [(40, 3), (n - 8, 5)]
    build, prop = _runs_case(runs, 4, ending == "zero_run", shape=(1, n) if tall else (n, 1))

    def prop_line(px):
        prop(px)
        lit, ref, m = vm.tokens(vm.residuals(px))
        assert (ref[-1] and m[-1] == 5) if ending != "literal" else (lit[-1] and lit[-2] and ref[-3])
    return build, prop_line


for _n in LINE_LENGTHS:
    for _tall in (False, True):
        for _ending in ("run", "zero_run", "literal"):
            add("line_%s_%s" % ("1x%d" % _n if _tall else "%dx1" % _n, _ending), *_line_case(_n, _tall, _ending))

# ---- a length sweep: every length symbol ------------------------------------------------------------------------------------------
SWEEP = list(range(1, 131)) + [(1 << k) + d for k in range(8, 12) for d in (-1, 0, 1)] + [4095, 4096, 4097, 4098, 8193, 8194]
SWEEP_SHAPE = (97, 549)      # 52,808 copies + 148 literals in front of them = 52,956 pixels, then 297 literals: every green value


def _sweep():
    w, h = SWEEP_SHAPE
    runs, s = [], 0
    for L in SWEEP:
        runs.append((s, L))
        s += L + 1
    assert s == 52956 and w * h - s >= 256
    res = filler(w * h, 4, seed=1)
    for k, (s0, L) in enumerate(runs):
        res[s0:s0 + L + 1] = run_tuple(k, 4)
    if (res[s - 1] == res[s]).all():
        res[s, 2] += 1
    assert np.array_equal(vm.tokens(res)[2], expected_m(w * h, runs))
    return from_residuals(res, w, h)


def _sweep_prop(px):
    res = vm.residuals(px)
    lit, ref, m = vm.tokens(res)
    assert set(m[ref]) == {min(L, vm.MAX_RUN) for L in SWEEP}
    hists = vm.histograms(res, lit, ref, m)
    assert len(hists[0]) == 280 and (hists[0] > 0).all(), "all 256 green values and all 24 length symbols"
    lengths = vm.parse(vm.encode(px))["codes"][0]["lengths"]
    assert min(lengths) >= 1


add("length_sweep", _sweep, _sweep_prop)

# ---- more than 256 tiles: 1025 x 1024 ------------------------------------------------------------------------------------------------
BIG_W, BIG_H = 1025, 1024
BIG_TILES = 257
ROUND = 256 * TILE            # the first pixel of tile 256, the first tile of the per-picture kernels' second round


def _big_prop(want_starts=None, carried=None, band=None):
    def prop(px):
        assert px.shape[:2] == (BIG_H, BIG_W) and -(-BIG_W * BIG_H // TILE) == BIG_TILES
        res = vm.residuals(px)
        starts = run_starts(res)
        lit, ref, m = vm.tokens(res)
        if want_starts is not None:
            assert list(starts) == want_starts, list(starts[:8])
        if carried is not None:
            # tile 256 has no run start of its own in front of its first pixels: what they are is decided by a start in round one
            assert starts[starts <= ROUND][-1] == carried < ROUND and m[ROUND] == ROUND - carried
        data = vm.encode(px)
        bits, data_bit = pixel_bits(px, data)
        per_tile = np.add.reduceat(bits, np.arange(0, len(bits), TILE))
        assert len(per_tile) == BIG_TILES and per_tile[:256].sum() > 0 and per_tile[256] > 0, "both rounds of the scan carry bits"
        payload = len(data) - 20
        assert (data_bit + int(bits.sum()) + 7) // 8 in (payload, payload - 1)
        if band is not None:
            assert per_tile[255] > 8 * (ROUND - band) and per_tile[256] > 8 * (BIG_W * BIG_H - ROUND)
    return prop


def _step(p, c):
    """flat up to pixel p, another flat colour from p on: one run start at p"""
    def build():
        res = np.zeros((BIG_W * BIG_H, 4), np.uint8)
        res[p:] = (0, 3, 9, 250) if c == 3 else (7, 3, 9, 250)
        return from_residuals(res, BIG_W, BIG_H, c)
    return build


def _odd_pixel(p):
    """one colour but for pixel p"""
    def build():
        px = np.full((BIG_H, BIG_W, 4), (90, 120, 30, 255), np.uint8)
        px[p // BIG_W, p % BIG_W] = (91, 119, 33, 200)
        return px
    return build


add("tiles257_step_in_tile_255", _step(ROUND - 1, 3), _big_prop([0, ROUND - 1], carried=ROUND - 1))
add("tiles257_step_in_tile_256", _step(ROUND, 4), _big_prop([0, ROUND]))
# (pixel 256 x 4096 - 1 is the first of the last row: nothing lies below it, so the odd pixel makes two run starts and no more)
add("tiles257_odd_pixel_in_tile_255", _odd_pixel(ROUND - 1), _big_prop([0, 1, ROUND - 1, ROUND]))
add("tiles257_odd_pixel_in_tile_256", _odd_pixel(ROUND), _big_prop([0, 1, ROUND, ROUND + 1]))
BAND = ROUND - 2000           # noise from here to the end; the run that starts on tile 255's last pixel reaches 3 pixels into tile 256


def _band():
    n = BIG_W * BIG_H
    res = np.zeros((n, 4), np.uint8)
    res[BAND:] = np.random.default_rng(257).integers(0, 256, (n - BAND, 4), dtype=np.uint8)
    res[ROUND - 1:ROUND + 3] = (1, 2, 3, 4)
    return from_residuals(res, BIG_W, BIG_H)


def _band_prop(px):
    _big_prop(carried=ROUND - 1, band=BAND)(px)
    lit, ref, m = vm.tokens(vm.residuals(px))
    assert list(m[ROUND - 2:ROUND + 4]) == [0, 0, 1, 2, 3, 0] and ref[ROUND + 2] and not ref[ROUND - 1:ROUND + 2].any()
    assert lit[BAND:ROUND].all()


add("tiles257_noise_band", _band, _band_prop)

# ---- codes -----------------------------------------------------------------------------------------------------------------------


def codes_of(px):
    return vm.parse(vm.encode(px))["codes"]


def _one_pixel(k):
    vals = (0, 1, 130, 255)
    res = np.array([[vals[(j + k) % 4] for j in range(4)]], np.uint8)

    def prop(px):
        assert px.shape == (1, 1, 4) and np.array_equal(vm.residuals(px), res)
        # red, blue, alpha, and green (which has no length symbol here): simple codes of the one symbol
        assert [c["simple"] for c in codes_of(px)[:4]] == [[int(res[0, 2])], [int(res[0, 1])], [int(res[0, 3])], [int(res[0, 0])]]
    return (lambda: from_residuals(res, 1, 1)), prop


for _k in range(4):     # every channel's residual is 0, 1, 130 and 255 in turn: the simple code's 1-bit and 8-bit forms
    add("one_pixel_%d" % _k, *_one_pixel(_k))


def _two_green_prop(px):
    res = vm.residuals(px)
    lit, ref, m = vm.tokens(res)
    hists = vm.histograms(res, lit, ref, m)
    assert lit.sum() == 1 and ref.sum() == 1 and (hists[0] > 0).sum() == 2 and (hists[0][256:] > 0).sum() == 1
    codes = codes_of(px)
    assert sorted(x for x in codes[0]["lengths"] if x) == [1, 1]
    assert all("simple" in c for c in codes[1:])


add("two_green_symbols_black", lambda: np.zeros((1, 2, 3), np.uint8), _two_green_prop)
add("two_green_symbols_ramp", lambda: from_residuals(np.full((9, 4), 7, np.uint8), 3, 3), _two_green_prop)


def _one_cl_symbol():
    i = np.arange(256 * 16)
    return from_residuals(np.stack([5 * i, 3 * i, i, 7 * i], axis=1) & 255, 256, 16)


def _one_cl_symbol_prop(px):
    assert vm.tokens(vm.residuals(px))[0].all()
    codes = codes_of(px)
    for k in (1, 2, 3):     # 256 symbols of 16 uses each: 256 lengths of 8, written with a code-length code of one symbol and no bits
        assert codes[k]["lengths"] == [8] * 256 and [x for x in codes[k]["cl_lengths"] if x] == [1]
    assert codes[0]["lengths"] == [8] * 256 + [0] * 24 and sorted(x for x in codes[0]["cl_lengths"] if x) == [1, 1]


add("one_code_length_symbol", _one_cl_symbol, _one_cl_symbol_prop)

FIB = [1, 1]
while len(FIB) < 20:
    FIB.append(FIB[-1] + FIB[-2])
FOLD15_SHAPE = (110, 161)
FOLD15_SEED = 15             # any seed does once equal neighbours are swapped apart; this one is what the figures below are for
assert sum(FIB) == FOLD15_SHAPE[0] * FOLD15_SHAPE[1] == 17710


def swap_apart(res, rng):
    """swaps whole tuples (every channel's histogram stays) until no two neighbours are equal"""
    key = res.view(np.uint32).reshape(len(res))
    for _ in range(100):
        bad = np.flatnonzero(key[1:] == key[:-1]) + 1
        if not len(bad):
            return res
        for i in bad:
            j = int(rng.integers(0, len(key)))
            key[i], key[j] = key[j], key[i]
    raise AssertionError("neighbours stay equal")


def _fold15():
    w, h = FOLD15_SHAPE
    rng = np.random.default_rng(FOLD15_SEED)
    res = np.zeros((w * h, 4), np.uint8)
    for k in range(4):      # Fibonacci counts on 20 symbols, symbols and order chosen per channel
        res[:, k] = rng.permutation(np.repeat(rng.choice(256, 20, replace=False), FIB).astype(np.uint8))
    return from_residuals(swap_apart(res, rng), w, h)


def _fold15_prop(px):
    res = vm.residuals(px)
    lit, ref, m = vm.tokens(res)
    assert lit.all()
    codes = codes_of(px)
    for k, hist in enumerate(vm.histograms(res, lit, ref, m)):
        assert sorted(hist[hist > 0]) == FIB
        assert vm.unlimited_depth(hist) == 19 and max(codes[k]["lengths"]) == 15, k


add("fold_to_15_bits", _fold15, _fold15_prop)

# symbols per code length 0 .. 15 (a random search's find): 256 symbols, Kraft sum 1, 2^(15 - l) uses each = 32,768 literals;
# as a histogram of code lengths its unlimited depth is 8
FOLD7_PROFILE = [0, 0, 0, 1, 2, 0, 2, 17, 108, 73, 16, 2, 5, 30, 0, 0]
FOLD7_SHAPE = (256, 128)
assert sum(FOLD7_PROFILE) == 256 and sum(n << (15 - l) for l, n in enumerate(FOLD7_PROFILE)) == 32768 == FOLD7_SHAPE[0] * FOLD7_SHAPE[1]


def _fold7():
    w, h = FOLD7_SHAPE
    rng = np.random.default_rng(7)
    counts = np.concatenate([[1 << (15 - l)] * n for l, n in enumerate(FOLD7_PROFILE) if n]).astype(np.int64)
    res = np.zeros((w * h, 4), np.uint8)
    res[:, 0] = np.where(np.arange(w * h) & 1, 200, 3)       # alpha alternates: no two neighbours are equal
    for k in (1, 2, 3):
        res[:, k] = rng.permutation(np.repeat(rng.permutation(256), counts).astype(np.uint8))
    return from_residuals(res, w, h)


def _fold7_prop(px):
    res = vm.residuals(px)
    lit, ref, m = vm.tokens(res)
    assert lit.all()
    codes = codes_of(px)
    for k in (0, 1, 2):
        lengths = codes[k]["lengths"]
        clh = np.bincount(lengths, minlength=19)
        assert list(clh[:16]) == [24 if k == 0 else 0] + FOLD7_PROFILE[1:]
        assert vm.unlimited_depth(clh) > 7 and max(codes[k]["cl_lengths"]) == 7, k
    assert sorted(x for x in codes[3]["lengths"] if x) == [1, 1]


add("fold_to_7_bits", _fold7, _fold7_prop)

# ---- the header's 14-bit fields at their end ----------------------------------------------------------------------------------------


def _limit(w, h, c):
    def prop(px):
        hdr = vm.parse(vm.encode(px))
        assert (hdr["width"], hdr["height"]) == (w, h) and max(w, h) == 16384 == 1 << 14
    return (lambda: np.random.default_rng(w + c).integers(0, 256, (h, w, c), dtype=np.uint8)), prop


for _w, _h in ((16384, 1), (1, 16384)):
    for _c in (4, 1):
        add("limit_%dx%d_c%d" % (_w, _h, _c), *_limit(_w, _h, _c))

# ---- noise of 97 x 43 (two tiles) whose payload length n has n mod 4 = 0, 1, 2, 3 -------------------------------------------------------
# the frame kernel's dword copy, its tail and the pad byte behind an odd n.  Noise, because the file is then longer than the 4 w h
# bytes of pixels which a device batch wants of every destination: only such a file can be given a capacity of exactly its length.
# Seeds found by trying 0, 1, 2, ...: n = 16856, 16853, 16854, 16851.
ALIGNMENT_SEEDS = {0: 1, 1: 0, 2: 2, 3: 7}
ALIGNMENT_SHAPE = (97, 43)


def _alignment(r):
    w, h = ALIGNMENT_SHAPE

    def prop(px):
        data = vm.encode(px)
        n = int.from_bytes(data[16:20], "little")
        assert n % 4 == r and len(data) == 20 + n + (n & 1) >= 4 * w * h and w * h > TILE
    return (lambda: np.random.default_rng(ALIGNMENT_SEEDS[r]).integers(0, 256, (h, w, 4), dtype=np.uint8)), prop


for _r in range(4):
    add("payload_4n_plus_%d" % _r, *_alignment(_r))

NAMES = list(CASES)
# what the destinations off alignment are tried with: the four above and a file of 15 + 1 bytes behind its 20 of headers
ALIGNMENT_CASES = ["payload_4n_plus_%d" % r for r in range(4)] + ["one_pixel_0"]
