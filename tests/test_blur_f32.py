"""The two f32 blur routes behind the window-tile matrix-pipe kernel: blur_tile_kernel (csrc/fl_blur.hip; f32 in LDS tiles) and the
generic two passes (csrc/fl_resample.hip), which production gets whenever the window-tile planner refuses a geometry (sigma >= 30 on
pictures taller than ~128 rows) and every no_wtile / no_mfma A/B run uses.

The arithmetic of both is one fused multiply-add per tap, pinned bit for bit by the oracle's ARITH_FMA mode; what can go wrong is
indexing -- job, tile, band, halo, prefetch ring -- so the pictures are noise (synth.uniform: a slip shows in every byte), the shapes
sit on the thresholds of csrc/fl_blur.h, and batches run the kernel's job numbering with more than one picture.  Bars: bit-exact
against ARITH_FMA and within parity.TOL_LSB of ARITH_REF; a batched result equals the same request sent alone, which has cleared those
bars.  Every test reads the three route counters (flgpu_debug_get "blur_wtile_launches", "blur_tile_launches",
"blur_generic_launches") around its launches: which kernel ran is asserted, never assumed."""
import numpy as np
import pytest

import oracle_lib
import parity
import synth
import wtile_model

ROUTES = ("blur_wtile_launches", "blur_tile_launches", "blur_generic_launches")
WTILE, TILE, GENERIC = (1, 0, 0), (0, 1, 0), (0, 0, 1)

# ---- csrc/fl_blur.h, mirrored: lanes per workgroup, column tiles, LDS bytes ----
BLUR_MAXTAPS, BLUR_TY, BLUR_LDS_MAX = 128, 8, 150 * 1024


def taps(fl, n, sigma):
    """The longest window of the Gaussian axis the runtime builds for n samples."""
    return int(fl.debug_axis_table(n, n, gaussian=True, sigma=sigma)[1].max())


def tiles_at(w, t, lanes):
    cap = lanes - (t - 1)
    return (w + cap - 1) // cap


def lanes_of(w, t):
    return min((256, 384, 512), key=lambda lanes: (tiles_at(w, t, lanes) * lanes, lanes))   # (the first of equal costs, as blur_threads)


def lds_bytes(w, channels, vtaps, htaps):
    ms = 4 if channels == 3 else channels
    wv = ((BLUR_TY + vtaps) * BLUR_TY + 3) & ~3
    return 4 * (wv + BLUR_TY * (lanes_of(w, htaps) + BLUR_MAXTAPS) * ms + htaps * min(w, 2 * htaps))


def host_route(fl, h, w, channels, sigma, wtile):
    """The route plan_blur / add_blur_launch (csrc/fl_batch.cpp) give one picture sent alone, derived without a device."""
    if wtile and wtile_model.run(None, blur_sigma=sigma, shape=(h, w, channels)) is not None:
        return WTILE
    vt, ht = taps(fl, h, sigma), taps(fl, w, sigma)
    return TILE if max(vt, ht) <= BLUR_MAXTAPS and lds_bytes(w, channels, vt, ht) <= BLUR_LDS_MAX else GENERIC


# ---- the counters ----
class routed:
    """with routed(st) as r: ... ; r.moved = how far the three route counters moved, (wtile, tile, generic).  Their sum moves exactly as
    stats()["blur_launches"] does."""

    def __init__(self, st):
        self.st = st

    def __enter__(self):
        self.before = [self.st.debug_get(k) for k in ROUTES]
        self.launches = self.st.stats()["blur_launches"]
        return self

    def __exit__(self, *exc):
        self.moved = tuple(self.st.debug_get(k) - b for k, b in zip(ROUTES, self.before))
        if exc[0] is None:
            assert sum(self.moved) == self.st.stats()["blur_launches"] - self.launches, self.moved
        return False


def check_f32(oracle, got, img, sigma):
    want = np.asarray(oracle.blur(img, sigma, arith=oracle_lib.ARITH_FMA))
    assert got.size == want.size == img.size
    assert np.array_equal(got, want.reshape(got.shape)), f"not bit-exact vs the fused oracle: maxdiff {parity.maxdiff(got, want.reshape(got.shape))}"
    assert parity.maxdiff(got, np.asarray(oracle.blur(img, sigma, arith=oracle_lib.ARITH_REF)).reshape(got.shape)) <= parity.TOL_LSB


_ALONE = {}   # (h, w, c, sigma, index) -> the blur sent alone on blur_tile_kernel, after it cleared the oracle's bars


def picture(h, w, c, index):
    return synth.uniform(h, w, c, index=index)


def tile_alone(fl, st, oracle, h, w, c, sigma, index):
    key = (h, w, c, sigma, index)
    if key not in _ALONE:
        img = picture(h, w, c, index)
        with st.switches(no_wtile=1), routed(st) as r:
            got = st.process_pixels(img, fl.make_params(blur_sigma=sigma))
        assert r.moved == TILE, f"meant to run on blur_tile_kernel: counters moved {r.moved}"
        check_f32(oracle, got, img, sigma)
        _ALONE[key] = got
    return _ALONE[key]


# ---- (a) one picture on blur_tile_kernel ----
SINGLE = [  # (h, w, sigma, channel counts)
    (9, 216, 10.0, (1, 2, 3, 4)),     # the widest one-tile picture at 256 lanes
    (9, 217, 10.0, (1, 2, 3, 4)),     # the first width at 384 lanes
    (9, 433, 10.0, (1, 2, 3, 4)),     # the 512-lane instantiation
    (9, 900, 10.0, (1, 2, 3, 4)),     # two tiles of 512 lanes: the halo across the tile border
    (9, 650, 10.0, (1, 2, 3, 4)),     # two tiles of 384 lanes
    (1, 64, 10.0, (1, 2, 3, 4)),      # bands: one row; ...
    (7, 64, 10.0, (1, 2, 3, 4)),      # ... a partial band alone;
    (8, 64, 10.0, (1, 2, 3, 4)),      # ... one whole band;
    (9, 64, 10.0, (1, 2, 3, 4)),      # ... a whole band and one row;
    (13, 64, 10.0, (1, 2, 3, 4)),     # ... windows of 13 rows: one more than the prefetch ring
    (61, 64, 10.0, (1, 2, 3, 4)),     # ... windows of 48 rows = 4 rings in the interior, cut to other lengths at both borders; a last band of 5 rows
    (40, 70, 0.3, (1, 2, 3, 4)),      # windows shorter than the ring: 3 taps,
    (40, 70, 1.0, (1, 2, 3, 4)),      # 5 taps,
    (40, 70, 3.0, (1, 2, 3, 4)),      # 13 taps
    (5, 7, 10.0, (1, 2, 3, 4)),       # the picture smaller than the window on both axes
    (1, 1, 10.0, (1, 2, 3, 4)),       # one pixel
    (140, 150, 31.75, (1,)),          # the longest windows the kernel takes: 127 taps (sigma 32 has 129)
]
SINGLE_CASES = [(h, w, s, c) for h, w, s, cs in SINGLE for c in cs]


def test_the_single_picture_cases_cover_the_kernels_instantiations(fl):
    """Host side: what the case list above claims to reach, recomputed with the rules of csrc/fl_blur.h."""
    seen = set()
    for h, w, s, c in SINGLE_CASES:
        assert host_route(fl, h, w, c, s, wtile=False) == TILE, (h, w, s, c)
        ht = taps(fl, w, s)
        seen.add((lanes_of(w, ht), min(tiles_at(w, ht, lanes_of(w, ht)), 2), c))
    assert {k[0] for k in seen} == {256, 384, 512} and {k[1] for k in seen} == {1, 2}
    assert {(lanes, c) for lanes, _, c in seen} == {(lanes, c) for lanes in (256, 384, 512) for c in (1, 2, 3, 4)}
    assert {(lanes_of(w, taps(fl, w, 10.0)), tiles_at(w, taps(fl, w, 10.0), lanes_of(w, taps(fl, w, 10.0)))) for w in (216, 217, 433, 900, 650)} == \
        {(256, 1), (384, 1), (512, 1), (512, 2), (384, 2)}
    assert taps(fl, 150, 31.75) == taps(fl, 140, 31.75) == 127 and taps(fl, 300, 32.0) == 129
    assert [taps(fl, 40, s) for s in (0.3, 1.0, 3.0)] == [3, 5, 13]   # against the kernel's ring of 12 rows
    # the groups of the batch tests
    assert {lanes_of(w, taps(fl, w, 10.0)) for w in (230, 300, 340, 217, 344)} == {384}
    assert {lanes_of(300, taps(fl, 300, s)) for s in (10.0, 14.3, 20.0)} == {384}
    # the demotion test: B does not fit the kernel's LDS, A2 shares its launch key (lanes, channels), A does not
    assert host_route(fl, 200, 300, 4, 30.0, wtile=False) == GENERIC and taps(fl, 300, 30.0) == 121 <= BLUR_MAXTAPS
    assert lanes_of(300, 121) == lanes_of(433, 41) == 512 and lanes_of(216, 41) == 256
    assert host_route(fl, 200, 433, 4, 10.0, wtile=False) == host_route(fl, 200, 216, 4, 10.0, wtile=False) == TILE


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,sigma,c", SINGLE_CASES)
def test_one_picture_on_the_tile_kernel(fl, gpu_state, oracle, h, w, sigma, c):
    got = tile_alone(fl, gpu_state, oracle, h, w, c, sigma, index=h + w + c)
    assert got.size == h * w * c


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,sigma", [(h, w, s) for h, w, s, cs in SINGLE if 3 in cs])
def test_the_generic_passes_give_the_tile_kernels_bytes(fl, gpu_state, oracle, h, w, sigma):
    want = tile_alone(fl, gpu_state, oracle, h, w, 3, sigma, index=h + w + 3)
    with gpu_state.switches(force_generic=1), routed(gpu_state) as r:
        got = gpu_state.process_pixels(picture(h, w, 3, h + w + 3), fl.make_params(blur_sigma=sigma))
    assert r.moved == GENERIC
    assert np.array_equal(got, want)


# ---- (b) channel shortcuts on a letterboxed result ----
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(grayscale=True, fill=(9, 9, 9)),        # grey on a grey fill: one channel filtered, <4, 1>
                                dict(grayscale=True, fill=(200, 10, 10)),    # grey on a coloured fill: <4, 3>
                                dict()])                                     # colour: <4, 3>
def test_letterboxed_results_filter_one_or_three_of_four_channels(fl, gpu_state, oracle, kw):
    """150 x 100 into 240 x 170: the picture becomes 240 x 160 and is framed (a 240 x 160 target would be met exactly and leave a
    Luma8 / Rgb8 picture without a frame), so the blur sees an opaque Rgba8 picture and filters one or three of its four channels."""
    img = synth.uniform(100, 150, 3, index=31)
    kw = dict(kw, w=240, h=170, blur_sigma=10.0)
    with gpu_state.switches(no_mfma=1), routed(gpu_state) as r:
        got, used = parity.device_pixels(fl, gpu_state, img, **kw)
    assert r.moved == TILE and not used
    assert got.shape == (170, 240, 4) and (got[..., 3] == 255).all()
    parity.check_pixels(oracle, got, img, False, **parity.oracle_kwargs(kw))   # f32 throughout: bit-exact vs ARITH_FMA, 1 LSB vs ARITH_REF


# ---- (c) batches ----
def batch_on_the_tile_kernel(fl, st, oracle, pics, launches):
    """pics: (h, w, c, sigma, index).  One batch under no_wtile: `launches` launches of blur_tile_kernel, every result the bytes of the
    same request sent alone."""
    alone = [tile_alone(fl, st, oracle, *p) for p in pics]
    with st.switches(no_wtile=1), routed(st) as r:
        outs = st.process_batch([picture(h, w, c, index) for h, w, c, _, index in pics], [fl.make_params(blur_sigma=s) for _, _, _, s, _ in pics])
    assert r.moved == (0, launches, 0)
    for k, (a, b) in enumerate(zip(alone, outs)):
        assert np.array_equal(a, np.asarray(b).reshape(a.shape)), f"picture {k} of the batch {pics[k]} differs from the same request sent alone"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 7, 8, 9, 17])
def test_batch_of_equal_pictures_is_one_launch(fl, gpu_state, oracle, n):
    """The kernel's job numbering (sets of 8 pictures, one per XCD): a last set of 2, 7, none, 1 and 1 after two full ones."""
    batch_on_the_tile_kernel(fl, gpu_state, oracle, [(40, 300, 3, 10.0, 100 + k) for k in range(n)], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, -1])
def test_batch_of_different_sizes_in_one_launch(fl, gpu_state, oracle, order):
    """The grid follows the group's largest picture: the workgroups past a smaller picture's tiles x bands leave at once."""
    pics = [(40, 230, 3, 10.0, 1), (9, 300, 3, 10.0, 2), (61, 340, 3, 10.0, 3), (8, 217, 3, 10.0, 4), (13, 344, 3, 10.0, 5)]
    batch_on_the_tile_kernel(fl, gpu_state, oracle, pics[::order], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, -1])
def test_batch_of_different_sigmas_in_one_launch(fl, gpu_state, oracle, order):
    """Per-picture taps and table sizes under the group's one LDS size."""
    pics = [(40, 300, 3, 10.0, 6), (40, 300, 3, 14.3, 7), (40, 300, 3, 20.0, 8)]
    batch_on_the_tile_kernel(fl, gpu_state, oracle, pics[::order], 1)


@pytest.mark.gpu
def test_batch_of_two_lane_counts_and_two_channel_counts_is_four_launches(fl, gpu_state, oracle):
    pics = [(9, 433, 3, 10.0, 9), (9, 216, 1, 10.0, 10), (9, 433, 1, 10.0, 11), (9, 216, 3, 10.0, 12), (9, 433, 3, 10.0, 13), (9, 216, 1, 10.0, 14)]
    assert len({(lanes_of(w, taps(fl, w, s)), c) for _, w, c, s, _ in pics}) == 4
    batch_on_the_tile_kernel(fl, gpu_state, oracle, pics, 4)


# ---- (d) the hand-over at large sigma, default switches ----
HANDOVER = [  # (h, w, sigma, channels, route): the routes follow from csrc/fl_batch.cpp, csrc/fl_blur.h and the window-tile planner
    (200, 300, 28.0, 1, WTILE), (200, 300, 28.0, 4, WTILE),
    (200, 300, 30.0, 1, TILE),        # 121 taps at 512 lanes: 141,736 bytes of LDS
    (200, 300, 30.0, 2, GENERIC),     # ... 162,216 bytes: above the kernel's 150 KiB
    (200, 300, 30.0, 3, GENERIC), (200, 300, 30.0, 4, GENERIC),   # ... 203,176 bytes
    (200, 300, 32.0, 1, GENERIC), (200, 300, 32.0, 4, GENERIC),   # 129 taps
    (200, 300, 40.0, 1, GENERIC), (200, 300, 40.0, 4, GENERIC),   # 161 taps
    (60, 77, 30.0, 1, WTILE), (60, 77, 30.0, 4, WTILE),           # the window-tile kernel refuses the window, not the sigma
]


def test_the_hand_over_cases_are_what_the_host_planners_say(fl):
    for h, w, s, c, route in HANDOVER:
        assert host_route(fl, h, w, c, s, wtile=True) == route, (h, w, s, c)
    assert {r for *_, r in HANDOVER} == {WTILE, TILE, GENERIC}


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,sigma,c,route", HANDOVER)
def test_hand_over_at_large_sigma(fl, gpu_state, oracle, h, w, sigma, c, route):
    img = picture(h, w, c, index=int(sigma) + c)
    with routed(gpu_state) as r:
        got = gpu_state.process_pixels(img, fl.make_params(blur_sigma=sigma))
    assert r.moved == route
    if route == WTILE:
        parity.check_pixels(oracle, got, img, True, **parity.oracle_kwargs(dict(blur_sigma=sigma)))
    else:
        check_f32(oracle, got, img, sigma)


# ---- (e) a group is demoted as a whole ----
@pytest.mark.gpu
def test_one_picture_that_does_not_fit_sends_its_group_to_the_generic_passes(fl, gpu_state, oracle):
    """add_blur_launch: blur_tiled is an AND over the pictures of a launch, and a launch is keyed by (lanes, channels).  B (121 taps, 512
    lanes, 203,176 bytes of LDS) goes to the generic passes; A2 shares its key and goes with it, byte for byte what blur_tile_kernel
    gives it alone; A keys to 256 lanes and keeps its kernel."""
    st = gpu_state
    a, a2, b = (200, 216, 4, 10.0, 41), (200, 433, 4, 10.0, 42), (200, 300, 4, 30.0, 43)
    want_a, want_a2 = tile_alone(fl, st, oracle, *a), tile_alone(fl, st, oracle, *a2)
    img_b = picture(200, 300, 4, 43)
    with st.switches(no_wtile=1), routed(st) as r:
        want_b = st.process_pixels(img_b, fl.make_params(blur_sigma=30.0))
    assert r.moved == GENERIC
    check_f32(oracle, want_b, img_b, 30.0)
    want = {a: want_a, a2: want_a2, b: want_b}
    for pics, moved in (([a2, b], GENERIC), ([b, a2], GENERIC), ([a, b], (0, 1, 1)), ([b, a], (0, 1, 1)), ([a, a2, b], (0, 1, 1))):
        with st.switches(no_wtile=1), routed(st) as r:
            outs = st.process_batch([picture(h, w, c, i) for h, w, c, _, i in pics], [fl.make_params(blur_sigma=s) for _, _, _, s, _ in pics])
        assert r.moved == moved, (pics, r.moved)
        for p, out in zip(pics, outs):
            assert np.array_equal(want[p], np.asarray(out).reshape(want[p].shape)), (p, pics)
