"""Pictures that meet their letterbox frame inside a matrix-pipe kernel.

1. The framed one-channel blur (csrc/fl_batch.cpp Work::luma_mid): a grey picture on a grey frame with a blur.  Stage 1 leaves the
   bare Luma8 picture (rw x rh, tightly packed) and resample_wtile_kernel<1, 6, WAVES> reads it through a virtual frame (fl_wtile.hip
   fetch(), `framed`: jb.cx / cy / rw / rh / fill), filters one channel and expands it to Rgba8 in its store.  Only single-register-set
   plans have that source; other plans fall back to the Rgba8 blur of the framed picture, and so does every grey picture under the
   switch `no_luma_mid`.  Cases: pillarboxes at column offsets whose 16-byte pieces straddle the picture's edge, letterboxes, odd sizes,
   pictures narrower than one piece, every sigma of the query's range and some only the ABI reaches, both wave counts of the
   instantiation, the fallback, and Rgba8 tiles of more K-steps than the registers hold (walked uncached, fly()).
2. Mixed placements in one launch: pictures that resize to the same size share a launch whatever their frames (assign_items groups
   by plan; the window-tile launches by plan too), so per-picture pitch, offset and fill must not leak from one picture to the next.

Host side (no device): the cases are checked against the planner -- the product's own table builder, run by oracle/wtile_model.cpp --
so that each route the tests claim to cover is the one the planner picks.  Device side: the bars of tests/parity.py against the CPU
oracle, the host model of the kernel's tables, and equality with the same request sent alone."""
import re
import threading

import numpy as np
import pytest

import oracle_lib
import parity
import synth
import wtile_model

LDS_4_WAVES = 78 * 1024       # fl_wtile.hip launch_wtile: single-register-set plans up to this much LDS run 4 waves per workgroup
NKMAX_ONE_SET = 6             # K-steps a single register set holds (fl_wtile.h kWtOperandRegs)

# (id, source shape (h, w, c), request).  Grey pictures on grey frames; a comment gives the placement plan_output computes (checked
# in test_cases_are_the_geometries_they_claim).
FRAMED = [
    ("cx1", (200, 296, 3), dict(w=240, h=160, grayscale=True, blur_sigma=10.0, fill=(0, 0, 0))),          # 237 x 160 at x 1
    ("cx7", (200, 281, 3), dict(w=240, h=160, grayscale=True, blur_sigma=11.0, fill=(255, 255, 255))),    # 225 at x 7
    ("cx15", (200, 261, 3), dict(w=240, h=160, grayscale=True, blur_sigma=12.0, fill=(128, 128, 128))),   # 209 at x 15
    ("cx17", (200, 256, 3), dict(w=240, h=160, grayscale=True, blur_sigma=13.0, fill=(9, 9, 9))),         # 205 at x 17
    ("cx33", (200, 216, 3), dict(w=240, h=160, grayscale=True, blur_sigma=14.0, fill=(200, 200, 200))),   # 173 at x 33
    ("one_px_narrower", (200, 299, 3), dict(w=240, h=160, grayscale=True, blur_sigma=15.0, fill=(77, 77, 77))),  # 239 at x 0
    ("letterbox_rh13", (26, 480, 3), dict(w=240, h=160, grayscale=True, blur_sigma=16.0, fill=(0, 0, 0))),        # 240 x 13 at y 73
    ("letterbox_rh25", (49, 480, 3), dict(w=240, h=160, grayscale=True, blur_sigma=17.0, fill=(255, 255, 255))),  # 240 x 25 at y 67
    ("letterbox_rh17", (34, 480, 3), dict(w=240, h=160, grayscale=True, blur_sigma=18.0, fill=(128, 128, 128))),  # 240 x 17 at y 71
    ("narrow_10px", (1000, 50, 3), dict(w=300, h=200, grayscale=True, blur_sigma=19.0, fill=(40, 40, 40))),       # 10 x 200 at x 145
    ("flat_15rows", (50, 1000, 3), dict(w=300, h=200, grayscale=True, blur_sigma=20.0, fill=(255, 255, 255))),    # 300 x 15 at y 92
    ("luma8_inverse", (200, 281, 1), dict(w=240, h=160, inverse=True, blur_sigma=10.0, fill=(60, 60, 60))),       # 225 at x 7
    ("luma8", (200, 256, 1), dict(w=240, h=160, blur_sigma=12.0, fill=(255, 255, 255))),                          # 205 at x 17
    ("sigma3_abi", (200, 261, 3), dict(w=240, h=160, grayscale=True, blur_sigma=3.0, fill=(128, 128, 128))),
    ("sigma5_abi", (200, 281, 1), dict(w=240, h=160, blur_sigma=5.0, fill=(0, 0, 0))),
    ("sigma26_8waves", (400, 611, 3), dict(w=300, h=200, grayscale=True, blur_sigma=26.0, fill=(128, 128, 128))),  # 300 x 196 at y 2
    ("wide_8waves", (400, 627, 3), dict(w=640, h=400, grayscale=True, blur_sigma=10.0, fill=(90, 90, 90))),         # 627 x 400 at x 6
    ("fallback_small", (60, 77, 3), dict(w=100, h=60, grayscale=True, blur_sigma=10.0, fill=(255, 255, 255))),     # 77 x 60 at x 11
    ("fallback_uncached", (200, 281, 3), dict(w=240, h=160, grayscale=True, blur_sigma=25.0, fill=(30, 30, 30))),
    ("uncached_sigma24", (200, 261, 3), dict(w=240, h=160, grayscale=True, blur_sigma=24.0, fill=(0, 0, 0))),               # 209 at x 15
]
FRAMED_IDS = [c[0] for c in FRAMED]
CASE = {c[0]: c for c in FRAMED}


def _plan(fl, shape, kw):
    p = fl.plan_output(fl.make_params(**kw), shape[1], shape[0], shape[2])
    return dict(rw=p.resized_w, rh=p.resized_h, cx=p.place_x, cy=p.place_y, ow=p.out_w, oh=p.out_h, lb=bool(p.letterboxed), oc=p.out_c)


def _model_plan(ow, oh, c, sigma):
    r = wtile_model.run(None, blur_sigma=sigma, shape=(oh, ow, c))
    return None if r is None else r[1]


def route(fl, shape, kw, no_luma_mid=False):
    """What csrc/fl_batch.cpp asks for a grey-on-grey blur: ("luma", one-channel plan) if that plan exists with ONE register set,
    else ("rgba", the Rgba8 plan) if that exists, else ("vector", None).  Plans of the out_w x out_h frame, as the planner builds them."""
    g = _plan(fl, shape, kw)
    one = _model_plan(g["ow"], g["oh"], 1, kw["blur_sigma"])
    if not no_luma_mid and one is not None and one["nslot"] == 1:
        return "luma", one, None
    four = _model_plan(g["ow"], g["oh"], 4, kw["blur_sigma"])
    return ("rgba", four, one) if four is not None else ("vector", None, one)


# ---------------------------------------------------------------------------------------------------------------- host side

def test_cases_are_the_geometries_they_claim(fl):
    """The placements the case list promises, as plan_output computes them (no device)."""
    seen = {k: _plan(fl, s, kw) for k, s, kw in FRAMED}
    assert all(g["lb"] and g["oc"] == 4 for g in seen.values())
    pillar = {k: g for k, g in seen.items() if g["cx"] > 0 and g["cy"] == 0}
    letter = {k: g for k, g in seen.items() if g["cy"] > 0 and g["cx"] == 0}
    assert {1, 7, 15, 17, 33} <= {g["cx"] for g in pillar.values()}, "frame column offsets whose 16-byte pieces straddle the picture's edge"
    assert {k for k, g in seen.items() if g["cx"] % 16} >= {"cx1", "cx7", "cx15", "cx17", "cx33", "narrow_10px"}
    assert len(letter) >= 3 and any(g["rh"] % 2 for g in letter.values())
    assert any(g["rw"] % 2 for g in pillar.values())
    assert seen["one_px_narrower"]["rw"] == seen["one_px_narrower"]["ow"] - 1
    assert seen["narrow_10px"]["rw"] < 16, "a picture narrower than one 16-byte piece"
    assert {int(kw["blur_sigma"]) for _, _, kw in FRAMED} >= set(range(10, 21)), "every sigma the query allows"
    fills = {kw["fill"][0] for _, _, kw in FRAMED}
    assert {0, 255} <= fills and any(0 < f < 255 for f in fills)
    assert all(kw["fill"][0] == kw["fill"][1] == kw["fill"][2] for _, _, kw in FRAMED), "grey frames only"
    assert any(s[2] == 1 and kw.get("inverse") for _, s, kw in FRAMED)


def test_cases_cover_every_route_of_the_framed_blur(fl):
    """Picked by the planner, not by hope: get_wtile_plan(..., 0, 0, out_w, out_h, 1) for luma_mid, the Rgba8 plan where that has more
    than one register set.  Covered: the one-channel plan on 4 waves and on 8, the fallback, and Rgba8 tiles of more K-steps than a
    register set holds (walked uncached).  A one-channel blur never has such tiles: the vertical window (kWtMaxKV = 4 K-steps, sigma
    <= ~26) runs out long before the horizontal one does (16 + 4 sigma bytes)."""
    kinds = {}
    for k, s, kw in FRAMED:
        r, plan, one = route(fl, s, kw)
        assert r != "vector", f"{k}: meant to stay on the window-tile kernel"
        kinds[k] = r
        if r == "luma":
            assert plan["nkh_max"] <= NKMAX_ONE_SET
        else:
            assert one is not None and one["nslot"] != 1
        r4, four, _ = route(fl, s, kw, no_luma_mid=True)
        assert r4 == "rgba", f"{k}: the Rgba8 route of no_luma_mid is meant to stay on the window-tile kernel"
    eight = {k for k, s, kw in FRAMED if kinds[k] == "luma" and route(fl, s, kw)[1]["lds_bytes"] > LDS_4_WAVES}
    assert eight == {"wide_8waves", "sigma26_8waves"}, eight                                   # (the rest: 4 waves)
    assert kinds["fallback_small"] == "rgba" and kinds["fallback_uncached"] == "rgba" and kinds["uncached_sigma24"] == "luma"
    for k in ("fallback_uncached", "uncached_sigma24"):   # (the first by default, the second under no_luma_mid)
        _, s, kw = CASE[k]
        _, four, _ = route(fl, s, kw, no_luma_mid=True)
        assert four["nslot"] == 1 and four["nkh_max"] > four["nkmax"], (k, four)
    assert sum(1 for k, s, kw in FRAMED if kinds[k] == "luma" and kw["blur_sigma"] < 10) >= 2   # ABI-only sigmas below the query's range
    assert sum(1 for k, s, kw in FRAMED if kw["blur_sigma"] > 20) >= 3                          # ... and above it


# the persistent matrix-pipe launch of mixed frames: 96 x 1024 Rgb8 sources (3072-byte rows: two strips) resized to 256 x 24 in
# frames that grow on one axis, every picture's fill different from its neighbours'
MIX_N, MIX_H, MIX_W = 300, 96, 1024


def mixed_frame_requests():
    kws = []
    for k in range(MIX_N):
        d = 1 + (k * 7) % 9
        v = (k * 97 + 13) % 256
        fill = (v, (v + 85) % 256, (v + 170) % 256)
        kws.append(dict(w=256 + d, h=24, fill=fill) if k % 2 == 0 else dict(w=256, h=24 + d, fill=fill))
    return kws


def test_mixed_frames_take_the_uniform_persistent_branch(fl):
    """The mixed-frame batch below is one plan for assign_items: all pictures resize to 256 x 24 (the frame plays no part), and at 256
    workgroups the assignment is uniform with whole rounds of pictures AND banded leftovers -- so the device test sees light
    transitions between pictures of different frames and bands of one picture on several workgroups."""
    kws = mixed_frame_requests()
    offs = set()
    for kw in kws:
        pl = fl.plan_output(fl.make_params(**kw), MIX_W, MIX_H, 3)
        assert (pl.resized_w, pl.resized_h) == (256, 24) and pl.letterboxed
        offs.add((pl.out_w, pl.place_x, pl.place_y))
    assert len({o[0] for o in offs}) >= 5 and len({o[1] for o in offs}) >= 4 and len({o[2] for o in offs}) >= 4
    assert all(kws[k]["fill"][0] != kws[k + 1]["fill"][0] for k in range(MIX_N - 1))
    d = fl.debug_mfma_plan(MIX_W, MIX_H, 3, 256, 24)
    assert d is not None and d["strips"] == 2
    job, strip, t0, t1, lists = fl.debug_assign_items(MIX_N, d["strips"], d["tiles"], 256)
    whole = (t1 - t0) == d["tiles"]
    assert whole.sum() >= 2 * 256 and (~whole).sum() > 0, "uniform: whole rounds of pictures (R >= 1) and banded leftovers"
    for first, cnt in lists:
        ks = np.arange(first, first + cnt)
        assert len(set(strip[ks][whole[ks]])) <= 1
        assert len(set(job[ks][whole[ks]])) == whole[ks].sum(), "a workgroup walks from one picture into the NEXT one"


# ---------------------------------------------------------------------------------------------------------------- device side

def _request(fl, st, img, kw):
    return st.process_pixels(img, fl.make_params(**kw))


def _far_from_picture(fl, g, sigma):
    """Frame pixels whose blur window does not reach the picture in one of the two passes: their value is the fill's, wherever the
    reference gets exactly that (the separable blur sums a constant row or column there)."""
    vl, vc, _ = fl.debug_axis_table(g["oh"], g["oh"], gaussian=True, sigma=sigma)
    hl, hc, _ = fl.debug_axis_table(g["ow"], g["ow"], gaussian=True, sigma=sigma)
    vl, vc, hl, hc = (a.astype(np.int64) for a in (vl, vc, hl, hc))
    rows_far = (vl + vc <= g["cy"]) | (vl >= g["cy"] + g["rh"])
    cols_far = (hl + hc <= g["cx"]) | (hl >= g["cx"] + g["rw"])
    return rows_far[:, None] | cols_far[None, :]


def _model_bar(got, model, what):
    """tests/test_wtile.py test_device_equals_the_host_model_of_its_tables, blur bar: every byte within 1, at most 2e-5 of them off
    (at least one allowed: on a picture of fewer than 50,000 bytes a rate bar would otherwise forbid the one tip it allows per 50,000)."""
    assert got.shape == model.shape, (got.shape, model.shape)
    d = got.astype(np.int16) - model.astype(np.int16)
    n = int((d != 0).sum())
    assert int(np.abs(d).max()) <= 1, f"{what}: more than 1 LSB from the host model of the kernel's tables"
    assert n <= max(1, 2e-5 * d.size), f"{what}: {n} of {d.size} bytes differ from the host model"


def _check_framed(fl, st, oracle, img, kw, got, want_ref, g):
    okw = parity.oracle_kwargs(kw)
    parity.check_pixels(oracle, got, img, True, **okw)
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all(), "R == G == B"
    assert (got[..., 3] == 255).all()
    fill = kw["fill"][0]
    far = _far_from_picture(fl, g, kw["blur_sigma"]) & (want_ref[..., 0] == fill)
    if g["ow"] - g["rw"] + g["oh"] - g["rh"] >= 4 * kw["blur_sigma"] + 4:
        assert far.any()
    bad = far & (got[..., 0] != fill)
    assert not bad.any(), f"{int(bad.sum())} far frame pixels are not the fill, first at {np.argwhere(bad)[0]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", FRAMED_IDS)
def test_framed_blur_against_oracle_and_model(fl, gpu_state, oracle, case):
    """One grey-on-grey blur: the oracle's bars, grey output, the frame away from the picture exactly the fill, and the device's bytes
    against the host model of the planner's tables applied to stage 1's picture (the same request without blur) -- a wrong cx / cy /
    rw / rh or a wrong byte merge of a partial piece shows up there as a wrong border, not as 1 LSB.  Then the other route
    (`no_luma_mid`: the Rgba8 blur of the framed picture) under the same bars, and within 1 LSB of the first."""
    _, shape, kw = CASE[case]
    img = synth.uniform(*shape, index=sum(shape) + int(kw["blur_sigma"]))
    g = _plan(fl, shape, kw)
    sigma = kw["blur_sigma"]
    want_ref = oracle.process_pixels(img, arith=oracle_lib.ARITH_REF, **parity.oracle_kwargs(kw))
    stage1 = _request(fl, gpu_state, img, dict(kw, blur_sigma=0.0))
    results = {}
    for no_luma_mid in (0, 1):
        r, plan, _ = route(fl, shape, kw, no_luma_mid=bool(no_luma_mid))
        gpu_state.debug_set("no_luma_mid", no_luma_mid)
        before = gpu_state.stats()
        got = _request(fl, gpu_state, img, kw)
        after = gpu_state.stats()
        assert after["blur_launches"] == before["blur_launches"] + 1
        assert after["wtile_launches"] > before["wtile_launches"], "the blur is meant to run on the window-tile kernel"
        _check_framed(fl, gpu_state, oracle, img, kw, got, want_ref, g)
        if r == "luma":
            model, _ = wtile_model.run(stage1[..., :1], blur_sigma=sigma)
            _model_bar(got[..., :1], model, f"{case} one channel")
        else:
            model, _ = wtile_model.run(stage1, blur_sigma=sigma)
            _model_bar(got, model, f"{case} Rgba8")
        results[no_luma_mid] = got
    assert parity.maxdiff(results[0], results[1]) <= parity.TOL_LSB


PLAN_LINE = re.compile(r"window-tile plan (\d+)x(\d+) -> rows \[0,\+(\d+)\) cols \[0,\+(\d+)\) x (\d): ok (\d), M-tiles \d+, strips \d+, "
                       r"registers (\d+) x (\d+), LDS (\d+)")


@pytest.mark.gpu
@pytest.mark.parametrize("case,no_luma_mid,want", [
    ("cx15", 0, "luma4"), ("wide_8waves", 0, "luma8"), ("sigma26_8waves", 0, "luma8"),
    ("fallback_small", 0, "rgba"), ("fallback_uncached", 0, "rgba_uncached"), ("uncached_sigma24", 1, "rgba_uncached")])
def test_route_is_proved_by_the_plan_lines(fl, capfd, case, no_luma_mid, want):
    """The blur plans the library builds, as its `debug_mfma` switch prints them, on a fresh context (a context builds a plan once):
    the one-channel line `x 1: ok 1, ... registers 1 x 6` with the LDS that picks 4 or 8 waves; for the fallback a one-channel plan of
    another register split and then the Rgba8 plan `x 4: ok 1`; with no_luma_mid the Rgba8 plan alone."""
    from conftest import require_device
    require_device()
    _, shape, kw = CASE[case]
    g = _plan(fl, shape, kw)
    img = synth.uniform(*shape, index=3)
    with fl.State(device=0) as st:
        st.debug_set("debug_mfma", 1)
        st.debug_set("no_luma_mid", no_luma_mid)
        capfd.readouterr()
        st.process_pixels(img, fl.make_params(**kw))
        err = capfd.readouterr().err
    lines = [m for m in PLAN_LINE.finditer(err) if (int(m[1]), int(m[2]), int(m[3]), int(m[4])) == (g["ow"], g["oh"], g["oh"], g["ow"])]
    print(case, "no_luma_mid" if no_luma_mid else "", [m[0] for m in lines])
    by_c = {int(m[5]): m for m in lines}
    if want.startswith("luma"):
        m = by_c[1]
        assert (m[6], m[7], m[8]) == ("1", "1", "6") and 4 not in by_c
        assert (int(m[9]) > LDS_4_WAVES) == (want == "luma8"), m[0]
    else:
        if no_luma_mid:
            assert 1 not in by_c
        else:
            assert by_c[1][6] == "1" and (by_c[1][7], by_c[1][8]) != ("1", "6"), "the one-channel plan has more than one register set"
        m = by_c[4]
        assert (m[6], m[7], m[8]) == ("1", "1", "6"), m[0]
        if want == "rgba_uncached":
            _, four, _ = route(fl, shape, kw, no_luma_mid=True)
            assert four["nkh_max"] > int(m[8]), "tiles of more K-steps than the register set holds"


LUMA_MIX = ["cx1", "cx7", "cx17", "cx33", "letterbox_rh13", "narrow_10px", "luma8_inverse", "sigma3_abi", "one_px_narrower"]


def _alone(fl, st, oracle, keys, imgs, check_some=True):
    out = []
    for n, (k, img) in enumerate(zip(keys, imgs)):
        _, shape, kw = CASE[k]
        got = _request(fl, st, img, kw)
        if check_some and n % 3 == 0:
            parity.check_pixels(oracle, got, img, True, **parity.oracle_kwargs(kw))
        out.append(got)
    return out


@pytest.mark.gpu
def test_framed_blurs_of_different_frames_share_one_launch(fl, gpu_state, oracle):
    """Framed one-channel blurs of different geometries, sigmas and fills travel in ONE window-tile launch (blur_groups by plan kind):
    each picture is byte for byte what it is alone -- on 4 waves, and again with an 8-wave picture in the launch."""
    keys = LUMA_MIX
    imgs = [synth.uniform(*CASE[k][1], index=40 + n) for n, k in enumerate(keys)]
    assert all(route(fl, CASE[k][1], CASE[k][2])[0] == "luma" for k in keys)
    alone = _alone(fl, gpu_state, oracle, keys, imgs)
    for extra in ([], ["wide_8waves"]):
        ks = keys + extra
        ims = imgs + [synth.uniform(*CASE[k][1], index=90) for k in extra]
        want = alone + _alone(fl, gpu_state, oracle, extra, ims[len(keys):], check_some=False)
        before = gpu_state.stats()["blur_launches"]
        got = gpu_state.process_batch(ims, [fl.make_params(**CASE[k][2]) for k in ks])
        assert gpu_state.stats()["blur_launches"] == before + 1, "one framed blur launch"
        for k, a, b in zip(ks, want, got):
            assert np.array_equal(np.asarray(b).reshape(a.shape), a), k


@pytest.mark.gpu
def test_framed_blurs_through_the_queue_from_16_threads(fl, gpu_state, oracle):
    """The same mix as single requests of 16 caller threads (the queue batches them as they come): the bytes of each request alone."""
    keys = LUMA_MIX * 2
    imgs = [synth.uniform(*CASE[k][1], index=40 + n) for n, k in enumerate(keys)]
    alone = _alone(fl, gpu_state, oracle, keys, imgs, check_some=False)
    got = [None] * len(keys)
    errors = []

    def worker(t):
        try:
            for i in range(t, len(keys), 16):
                got[i] = _request(fl, gpu_state, imgs[i], CASE[keys[i]][2])
        except Exception as e:   # (re-raised on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i, k in enumerate(keys):
        assert np.array_equal(got[i], alone[i]), (i, k)


@pytest.mark.gpu
def test_window_tile_resamples_of_different_frames_share_one_launch(fl, gpu_state, oracle):
    """540 x 960 Rgb8 in frames of different sizes and fills, one launch: a 600 x 338 picture in frames of different heights (one plan),
    and a 601 x 338 one in frames of different widths (the second plan of the launch: different pitch and first column).  Every picture
    is byte for byte what it is alone, its frame its own fill."""
    frames = [(600, 338 + d) for d in (1, 2, 5, 8, 13, 20, 62)] + [(601 + d, 338) for d in (1, 2, 7, 16)]   # (all letterboxed)
    imgs = [synth.uniform(540, 960, 3, index=60 + k) for k in range(len(frames))]
    ps = []
    for k, (w, h) in enumerate(frames):
        v = (k * 71 + 5) % 256
        ps.append(dict(w=w, h=h, fill=(v, 255 - v, (v * 3) % 256)))
    for kw in ps:
        pl = fl.plan_output(fl.make_params(**kw), 960, 540, 3)
        assert (pl.resized_w, pl.resized_h) == ((600, 338) if kw["w"] == 600 else (601, 338)) and pl.letterboxed
    before = gpu_state.stats()["wtile_launches"]
    got = gpu_state.process_batch(imgs, [fl.make_params(**kw) for kw in ps])
    assert gpu_state.stats()["wtile_launches"] == before + 1
    for k, (img, kw) in enumerate(zip(imgs, ps)):
        a, used = parity.device_pixels(fl, gpu_state, img, **kw)
        assert used
        b = np.asarray(got[k]).reshape(a.shape)
        assert np.array_equal(a, b), kw
        pl = fl.plan_output(fl.make_params(**kw), 960, 540, 3)
        frame = np.ones(b.shape[:2], bool)
        frame[pl.place_y:pl.place_y + pl.resized_h, pl.place_x:pl.place_x + pl.resized_w] = False
        assert (b[frame] == np.array(list(kw["fill"]) + [255], np.uint8)).all(), kw
        if k % 3 == 0:
            parity.check_pixels(oracle, b, img, True, **parity.oracle_kwargs(kw))


@pytest.mark.gpu
def test_persistent_matrix_pipe_launch_of_mixed_frames(fl, gpu_state, oracle):
    """test_uniform_batch_on_persistent_workgroups with per-picture frames: 300 pictures resized to 256 x 24 in frames 257-265 wide or
    25-33 high, each fill different from its neighbours'.  They share one launch whose workgroups walk from picture to picture by the
    light transition (the outgoing picture's destination, pitch, first pixel and fill kept in the two-slot LDS context) -- every
    picture, the banded leftovers and the first and last of every workgroup's list included, is what it is alone, and its frame is its
    own fill."""
    import torch
    kws = mixed_frame_requests()
    ps = [fl.make_params(**kw) for kw in kws]
    imgs = [synth.uniform(MIX_H, MIX_W, 3, index=700 + k) for k in range(MIX_N)]
    plans = [fl.plan_output(p, MIX_W, MIX_H, 3) for p in ps]
    stride = (max(int(pl.out_bytes) for pl in plans) + 255) // 256 * 256
    src = torch.from_numpy(np.stack(imgs)).cuda()
    dst = torch.zeros((MIX_N, stride), dtype=torch.uint8, device="cuda")
    before = gpu_state.stats()["mfma_launches"]
    gpu_state.process_batch_device([src.data_ptr() + k * MIX_H * MIX_W * 3 for k in range(MIX_N)], [(MIX_H, MIX_W, 3)] * MIX_N, ps,
                                   [dst.data_ptr() + k * stride for k in range(MIX_N)], [stride] * MIX_N)
    gpu_state.batch_results()
    assert gpu_state.stats()["mfma_launches"] == before + 1
    out = dst.cpu().numpy()
    for k in range(MIX_N):
        pl, kw = plans[k], kws[k]
        got = out[k, :int(pl.out_bytes)].reshape(pl.out_h, pl.out_w, 4)
        frame = np.ones((pl.out_h, pl.out_w), bool)
        frame[pl.place_y:pl.place_y + 24, pl.place_x:pl.place_x + 256] = False
        assert (got[frame] == np.array(list(kw["fill"]) + [255], np.uint8)).all(), (k, kw)
        alone, used = parity.device_pixels(fl, gpu_state, imgs[k], **kw)
        assert used and np.array_equal(got, alone), (k, kw)
        if k in (0, 1, 151, MIX_N - 1):
            parity.check_pixels(oracle, got, imgs[k], True, **parity.oracle_kwargs(kw))
