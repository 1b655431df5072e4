"""FLGPU_FE_WEBP_LOSSY_LF, _I4_LF, _AP_LF and _I4_AP_LF on the device: the lossy WebP coder with a loop filter level picked by filtering
and measuring four candidates.  Every file equals the restated encoder's (tests/vp8_lf_model.py) on the planes the same request
returns with FLGPU_FE_WEBP420 -- which libwebp decodes to exactly the model's filtered reconstruction
(tests/test_webp_lossy_filter_host.py) --, the cost words the filter launch leaves are the model's, the library's own decoder
reads each file back to the filtered reconstruction, and the front ends beside them still write their bytes."""
import io
import threading

import numpy as np
import pytest

import synth
import vp8_ap_cases
import vp8_ap_model as ap
import vp8_i4_model as m4
import vp8_lf_cases as cases_mod
import vp8_lib
import vp8_model as vm

Q = "w=300&h=200&webp=true&quality=75"
VARIANTS = cases_mod.VARIANTS
IDS = ("i16", "b_pred", "i16_probs", "b_pred_probs")


def _fe(fl, i4, adapt):
    return fl.vp8_front_end(i4, adapt, lf=True)


def _twin(fl, i4, adapt):
    return fl.vp8_front_end(i4, adapt)


def _max_out(w, h, i4, adapt):
    return ap.max_out_bytes(w, h, i4) if adapt else (m4.max_out_bytes(w, h) if i4 else vm.max_out_bytes(w, h))


def _planes(fl, st, img, **kw):
    return st.process_pixels(img, fl.make_params(front_end=fl.FE_WEBP420, **kw))


def _model_of(fl, st, img, key, i4, adapt, base=None, **kw):
    """The model's (file, reconstruction, filtered reconstruction, stats) for the request: its planes are what the same request
    returns with FE_WEBP420."""
    pl = _planes(fl, st, img, **kw)
    return cases_mod.model("dev:" + key, pl.y, pl.u, pl.v, kw["quality"], pl.a if pl.has_alpha else None, i4, adapt, base), pl


@pytest.fixture(scope="module")
def big():
    return synth.photo(1080, 1920, 3, index=3)


@pytest.fixture()
def forced(gpu_state):
    """set(base): forces the base level (None: from the quantiser); the default is back when the test ends."""
    def set_base(base):
        gpu_state.debug_set("vp8_filter_base", -1 if base is None else base)
    yield set_base
    gpu_state.debug_set("vp8_filter_base", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("i4,adapt", VARIANTS, ids=IDS)
def test_every_corpus_file_costs_and_choice_equal_the_model_and_decode_to_its_filtered_reconstruction(fl, gpu_state, forced, i4, adapt):
    assert gpu_state.debug_get("vp8_filter_base") == -1
    bad, bad_costs, bad_decode, chosen = [], [], [], set()
    for name, img, q, base in cases_mod.corpus():
        forced(base)
        p = fl.make_params(quality=q, front_end=_fe(fl, i4, adapt))
        data = gpu_state.process_pixels(img, p)
        costs = gpu_state.debug_vp8_filter_costs(img, p)
        forced(None)
        (want, rec, shown, stats), pl = _model_of(fl, gpu_state, img, cases_mod.analysis_key(name), i4, adapt, base, quality=q)
        h, w = img.shape[:2]
        assert isinstance(data, bytes) and len(data) <= _max_out(w, h, i4, adapt), name
        assert pl.has_alpha == name.endswith("_a") == (data[12:16] == b"VP8X"), name
        if costs != dict(levels=stats["levels"], D=stats["D"], chosen=stats["chosen"]):
            bad_costs.append((name, costs, stats["levels"], stats["D"], stats["chosen"]))
        if data != want:
            bad.append(name)
            continue
        chosen.add(stats["levels"].index(stats["chosen"]) if stats["base"] else -1)
        info = fl.vp8_info(data)
        assert (info["filter_level"], info["filter_type"], info["sharpness"]) == (stats["chosen"], 0, 0), name
        # libwebp, and the library's own decoder (flgpu_decode_webp_lossy's kernels): the filtered planes, then the pixels
        theirs_yuv, theirs = vp8_lib.decode_yuv(data), vp8_lib.decode_rgba(data)
        got = gpu_state.debug_vp8_planes(data, filtered=True)
        unfiltered = gpu_state.debug_vp8_planes(data, filtered=False)
        pixels = gpu_state.decode_webp_lossy(data)
        if (not all(np.array_equal(g, r) for g, r in zip(theirs_yuv, shown)) or not all(np.array_equal(g, r) for g, r in zip(got, shown))
                or not all(np.array_equal(g, r) for g, r in zip(unfiltered, rec)) or not np.array_equal(pixels, theirs[..., :pixels.shape[2]])):
            bad_decode.append(name)
        # L0 = 0, or level 0 chosen: the twin's file byte for byte
        if stats["chosen"] == 0:
            assert data == gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=_twin(fl, i4, adapt))), name
    assert not bad_costs, bad_costs
    assert not bad, bad
    assert not bad_decode, bad_decode
    # (flgpu_get_stats resolves the pending HIP-event pairs; the filter launch is inside the lossy WebP encoder's)
    assert chosen == {-1, 0, 1, 2, 3} and gpu_state.stats()["frontend_launches"] > 0 and gpu_state.debug_get("webp_lossy_ns") > 0


@pytest.mark.gpu
def test_the_forced_base_only_moves_the_loop_filtered_families(fl, gpu_state, forced):
    img, q = dict((n, (i, q)) for n, i, q, _ in cases_mod.corpus())["photo_64x48_q1"]
    before = {fe: gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe)) for fe in fl.FE_WEBP_LOSSY_ALL}
    forced(10)
    after = {fe: gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe)) for fe in fl.FE_WEBP_LOSSY_ALL}
    forced(None)
    for fe in (fl.FE_WEBP_LOSSY, fl.FE_WEBP_LOSSY_I4, fl.FE_WEBP_LOSSY_AP, fl.FE_WEBP_LOSSY_I4_AP):
        assert before[fe] == after[fe] and fl.vp8_info(after[fe])["filter_level"] == 0, fe
    for fe in (fl.FE_WEBP_LOSSY_LF, fl.FE_WEBP_LOSSY_I4_LF, fl.FE_WEBP_LOSSY_AP_LF, fl.FE_WEBP_LOSSY_I4_AP_LF):
        assert fl.vp8_info(before[fe])["filter_level"] in (26, 51, 63) and fl.vp8_info(after[fe])["filter_level"] in (5, 10, 15), fe  # of {0, 26, 51, 63} / {0, 5, 10, 15}
    with pytest.raises(fl.FanlinError):
        gpu_state.debug_vp8_filter_costs(img, fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY))


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state, big):
    corpus = {name: (img, q) for name, img, q, base in cases_mod.corpus() if base is None}
    small = big[:500, :700].copy()
    # (name or None, picture, params, family); loop-filtered pictures of different content and size stand next to each other in all
    # four families, where one picture's working copies or cost words leaking into the next would show
    names = ("noise_64x48_q30", "photo_300x200_q30", "flat_64x48_q75", "photo_1x1_q1", "photo_16x144_q1", "patchwork_64x48_q30_a",
             "photo_64x48_q99", "wave32_64x48_q30", "noise_128x16_q50")
    jobs = []
    for k, n in enumerate(names):
        for i4, adapt in (VARIANTS[k % 4], VARIANTS[(k + 1) % 4]):
            jobs.append((n, corpus[n][0], fl.make_params(quality=corpus[n][1], front_end=_fe(fl, i4, adapt)), (i4, adapt)))
    old = []
    for n, (i4, adapt) in (("noise_64x48_q30", (False, False)), ("wave32_64x48_q30", (True, False)), ("photo_300x200_q30", (False, True)),
                           ("patchwork_64x48_q30_a", (True, True))):
        old.append((n, corpus[n][0], fl.make_params(quality=corpus[n][1], front_end=_twin(fl, i4, adapt)), (i4, adapt)))
    for fe, q in ((fl.FE_JPEG, 75), (fl.FE_PNG, 75), (fl.FE_WEBP_LOSSLESS, 100), (fl.FE_NONE, 75), (fl.FE_WEBP420, 75), (fl.FE_WEBP_LOSSY, 30),
                  (fl.FE_WEBP_LOSSY_I4, 99), (fl.FE_WEBP_LOSSY_AP, 30), (fl.FE_WEBP_LOSSY_I4_AP, 75), (fl.FE_WEBP_LOSSY_LF, 30),
                  (fl.FE_WEBP_LOSSY_I4_AP_LF, 75)):
        jobs.append((None, small, fl.make_params(300, 200, quality=q, front_end=fe), None))
    everything = jobs + old
    order = np.random.default_rng(11).permutation(len(everything))  # the eight lossy WebP families interleaved in the caller's order
    everything = [everything[i] for i in order]
    images, params = [j[1] for j in everything], [j[2] for j in everything]
    alone = [gpu_state.process_pixels(i, p) for i, p in zip(images, params)]
    outs = gpu_state.process_batch(images, params)
    for k, (got, want) in enumerate(zip(outs, alone)):
        fe = params[k].front_end
        if fe == fl.FE_NONE:
            assert np.array_equal(got, want), k
        elif fe == fl.FE_WEBP420:
            assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in "yuva") and got.has_alpha == want.has_alpha, k
        else:
            assert isinstance(got, bytes) and got == want, (k, fe)
    for k, (name, img, p, fam) in enumerate(everything):
        if name is None:
            continue
        if p.front_end >= fl.FE_WEBP_LOSSY_LF:
            assert outs[k] == _model_of(fl, gpu_state, img, name, fam[0], fam[1], quality=p.quality)[0][0], (name, fam)
        else:  # the four old families still give their models' bytes
            pl = _planes(fl, gpu_state, img, quality=p.quality)
            want = vp8_ap_cases.model("lfdev:" + name, pl.y, pl.u, pl.v, p.quality, pl.a if pl.has_alpha else None, fam[0], fam[1])[0]
            assert outs[k] == want and fl.vp8_info(outs[k])["filter_level"] == 0, (name, fam)
    # two loop-filtered neighbours of different content, in both orders
    pair = [(n, corpus[n][0], fl.make_params(quality=corpus[n][1], front_end=fl.FE_WEBP_LOSSY_LF)) for n in ("noise_64x48_q30", "photo_300x200_q30")]
    for a, b in ((0, 1), (1, 0)):
        got = gpu_state.process_batch([pair[a][1], pair[b][1]], [pair[a][2], pair[b][2]])
        assert got[0] == _model_of(fl, gpu_state, pair[a][1], pair[a][0], False, False, quality=pair[a][2].quality)[0][0]
        assert got[1] == _model_of(fl, gpu_state, pair[b][1], pair[b][0], False, False, quality=pair[b][2].quality)[0][0]


@pytest.mark.gpu
def test_the_query_level_route(fl, gpu_state, big):
    from PIL import Image
    lossy, i4b, probs, filt = fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER
    pl = None
    for i4, adapt in VARIANTS:
        want = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=_fe(fl, i4, adapt)))
        (model, _, _, stats), pl = _model_of(fl, gpu_state, big, "big", i4, adapt, w=300, h=200, quality=75)
        assert want == model and stats["base"] == 8
        old = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=_twin(fl, i4, adapt)))
        bits = lossy | filt | (i4b if i4 else 0) | (probs if adapt else 0)
        for q, fmt, content in ((Q, fl.IN_PNG, fl.Format(fl.ACCEPT_WEBP | bits)), (Q, fl.IN_JPEG, fl.Format(fl.ACCEPT_WEBP | bits)),
                                ("w=300&h=200&quality=75", fl.IN_WEBP, fl.Format(bits))):
            mime, kind, body = gpu_state.process_image(big, q, content, input_format=fmt)
            assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body == want, (i4, adapt, q)
        # without the new bit: the twin's file
        mime, kind, body = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | (bits & ~filt)), input_format=fl.IN_PNG)
        assert kind == fl.RESULT_WEBP_STREAM and body == old and (body == want) == (stats["chosen"] == 0)
    # the new bit alone, and with every other bit but _LOSSY: the planes
    for bits in (filt, filt | i4b, filt | probs, filt | i4b | probs):
        mime, kind, planes = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | bits), input_format=fl.IN_PNG)
        assert kind == fl.RESULT_WEBP_PLANES and all(np.array_equal(getattr(planes, f), getattr(pl, f)) for f in "yuva")
    # an output over FE_WEBP_LOSSY_I4_AP's limit (120 x 68 macroblocks) with all bits: FE_WEBP_LOSSY_AP_LF's file
    every = fl.Format(fl.ACCEPT_WEBP | lossy | i4b | probs | filt)
    mime, kind, body = gpu_state.process_image(big, "webp=true&quality=30", every, input_format=fl.IN_PNG)
    assert kind == fl.RESULT_WEBP_STREAM and body == gpu_state.process_pixels(big, fl.make_params(quality=30, front_end=fl.FE_WEBP_LOSSY_AP_LF))
    assert fl.vp8_info(body)["filter_level"] in (0, 8, 16, 24) and vp8_lib.decode_yuv(body)[0].shape == (1080, 1920)
    # file sources: a JPEG file through the query-level entry point gives the stream its decoded pixels give
    img = synth.photo(360, 640, 3, index=41)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=90)
    for i4, adapt in VARIANTS:
        content = fl.Format(fl.ACCEPT_WEBP | lossy | filt | (i4b if i4 else 0) | (probs if adapt else 0))
        mime, kind, body = gpu_state.process_jpeg(b.getvalue(), Q, content)
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM)
        assert body == gpu_state.process_jpeg_pixels(b.getvalue(), fl.make_params(300, 200, quality=75, front_end=_fe(fl, i4, adapt))), (i4, adapt)


@pytest.mark.gpu
def test_sixteen_concurrent_callers_get_identical_bytes(fl, gpu_state, big):
    kinds = [fl.FE_WEBP_LOSSY_LF, fl.FE_WEBP_LOSSY_I4_AP_LF, fl.FE_WEBP_LOSSY, fl.FE_WEBP_LOSSY_AP_LF, fl.FE_WEBP_LOSSY_I4_AP, fl.FE_WEBP_LOSSY_I4_LF,
             fl.FE_WEBP_LOSSY_AP, fl.FE_WEBP_LOSSY_I4]
    want = {fe: gpu_state.process_pixels(big, fl.make_params(300, 200, quality=30, front_end=fe)) for fe in set(kinds)}
    assert want[fl.FE_WEBP_LOSSY_LF] == _model_of(fl, gpu_state, big, "big30", False, False, w=300, h=200, quality=30)[0][0]
    assert want[fl.FE_WEBP_LOSSY_I4_AP_LF] == _model_of(fl, gpu_state, big, "big30", True, True, w=300, h=200, quality=30)[0][0]
    got, errors = [None] * 16, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=30, front_end=kinds[i % 8]))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        assert got[i] == want[kinds[i % 8]], i


@pytest.mark.gpu
@pytest.mark.parametrize("i4,adapt", VARIANTS, ids=IDS)
def test_a_destination_one_byte_short(fl, gpu_state, i4, adapt):
    corpus = {name: (img, q) for name, img, q, base in cases_mod.corpus()}
    img, q = corpus["patchwork_64x48_q30_a"]
    p = fl.make_params(quality=q, front_end=_fe(fl, i4, adapt))
    full = gpu_state.process_pixels(img, p)
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # a batch with one too-small stream: no bytes claimed for it and none written, neither into it nor past its capacity (every
    # destination is a slice of one buffer with a guard behind it); its neighbours delivered intact
    lib = fl.load_library()
    cap, guard = int(fl.plan_output(p, 64, 48, 4).max_out_bytes), 64
    caps = [cap, len(full) - 1, cap]
    offs = [0, cap + guard, cap + guard + len(full) - 1 + guard]
    buf = np.full(offs[2] + cap + guard, 0xA5, np.uint8)
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(img.ctypes.data, img.nbytes, 64, 48, 4, 0) for _ in range(3)])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(buf.ctypes.data + o, cp, 0, 0, 0, 0) for o, cp in zip(offs, caps)])
    ps = (fl.flgpu_params * 3)(p, p, p)
    assert lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts) == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0 and (buf[offs[1]:offs[1] + caps[1]] == 0xA5).all(), "no partial file"
    for i in range(3):
        assert (buf[offs[i] + caps[i]:offs[i] + caps[i] + guard] == 0xA5).all(), "nothing past the capacity"
    for i in (0, 2):
        assert buf[offs[i]:offs[i] + dsts[i].bytes].tobytes() == full
