"""FLGPU_FE_WEBP_LOSSY_AP and FLGPU_FE_WEBP_LOSSY_I4_AP on the device: the lossy WebP coder with per-picture coefficient
probabilities.  Every file equals the restated encoder's (tests/vp8_ap_model.py) on the planes the same request returns with
FLGPU_FE_WEBP420 -- which libwebp decodes to exactly the non-adaptive front end's reconstruction
(tests/test_webp_lossy_probs_host.py) --, the library's own decoder reads it back to that reconstruction, and the front ends
beside it still write their bytes."""
import io
import threading

import numpy as np
import pytest

import synth
import vp8_ap_cases
import vp8_cases
import vp8_i4_cases
import vp8_ap_model as ap
import vp8_lib

Q = "w=300&h=200&webp=true&quality=75"


def _fe(fl, i4):
    return fl.vp8_front_end(i4, ap=True)


def _planes(fl, st, img, **kw):
    return st.process_pixels(img, fl.make_params(front_end=fl.FE_WEBP420, **kw))


def _model_of(fl, st, img, key, i4, adapt=True, **kw):
    """The model's (file, reconstruction, stats) for the request: its planes are what the same request returns with FE_WEBP420."""
    pl = _planes(fl, st, img, **kw)
    return vp8_ap_cases.model("dev:" + key, pl.y, pl.u, pl.v, kw["quality"], pl.a if pl.has_alpha else None, i4, adapt), pl


@pytest.fixture(scope="module")
def big():
    return synth.photo(1080, 1920, 3, index=3)


@pytest.mark.gpu
@pytest.mark.parametrize("i4", (False, True), ids=("i16", "b_pred"))
def test_every_corpus_file_equals_the_model_and_decodes_to_its_reconstruction(fl, gpu_state, i4):
    bad, bad_decode, updates = [], [], 0
    for name, img, q in vp8_ap_cases.corpus(i4):
        data = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=_fe(fl, i4)))
        (want, rec, stats), pl = _model_of(fl, gpu_state, img, name, i4, quality=q)
        h, w = img.shape[:2]
        assert isinstance(data, bytes) and len(data) <= ap.max_out_bytes(w, h, i4), name
        assert pl.has_alpha == name.endswith("_a") == (data[12:16] == b"VP8X"), name
        if data != want:
            bad.append(name)
            continue
        updates += len(stats["updated"])
        # libwebp, and the library's own decoder (flgpu_decode_webp_lossy's kernels): the planes, then the pixels
        theirs_yuv, theirs = vp8_lib.decode_yuv(data), vp8_lib.decode_rgba(data)
        got = gpu_state.debug_vp8_planes(data, filtered=True)
        pixels = gpu_state.decode_webp_lossy(data)
        if (not all(np.array_equal(g, r) for g, r in zip(theirs_yuv, rec)) or not all(np.array_equal(g, r) for g, r in zip(got, rec))
                or not np.array_equal(pixels, theirs[..., :pixels.shape[2]])):
            bad_decode.append(name)
    assert not bad, bad
    assert not bad_decode, bad_decode
    assert updates > 0 and gpu_state.stats()["frontend_launches"] > 0 and gpu_state.debug_get("webp_lossy_ns") > 0


@pytest.mark.gpu
def test_a_flat_picture_is_the_non_adaptive_front_ends_file(fl, gpu_state):
    flat = {False: dict((n, (i, q)) for n, i, q in vp8_cases.corpus())["flat_64x48_q75"],
            True: dict((n, (i, q)) for n, i, q in vp8_i4_cases.corpus())["edges0_48x48_q1"]}  # (the second has coded macroblocks and no update)
    for i4, (img, q) in flat.items():
        old = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY_I4 if i4 else fl.FE_WEBP_LOSSY))
        assert gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=_fe(fl, i4))) == old, i4


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state, big):
    c16 = {name: (img, q) for name, img, q in vp8_ap_cases.corpus(False)}
    c4 = {name: (img, q) for name, img, q in vp8_ap_cases.corpus(True)}
    small = big[:500, :700].copy()
    # (name or None, picture, params); adaptive pictures of different content and size stand next to each other in both families,
    # where a table shared between pictures, or one picture's counters leaking into the next, would show
    jobs = [(n, c16[n][0], fl.make_params(quality=c16[n][1], front_end=fl.FE_WEBP_LOSSY_AP), False)
            for n in ("noise_64x48_q99", "photo_300x200_q75", "flat_64x48_q75", "photo_1x1_q75_a", "photo_16x144_q99", "ramp_v_64x48_q75")]
    jobs += [(n, c4[n][0], fl.make_params(quality=c4[n][1], front_end=fl.FE_WEBP_LOSSY_I4_AP), True)
             for n in ("patchwork_64x48_q30_a", "photo_300x200_q30", "noise_16x64_q99", "edges0_48x48_q1", "noise_128x16_q30")]
    for fe, q in ((fl.FE_JPEG, 75), (fl.FE_WEBP_LOSSY_I4, 30), (fl.FE_PNG, 75), (fl.FE_WEBP_LOSSLESS, 100), (fl.FE_NONE, 75), (fl.FE_WEBP420, 75),
                  (fl.FE_WEBP_LOSSY, 30), (fl.FE_WEBP_LOSSY_I4, 99), (fl.FE_WEBP_LOSSY, 75), (fl.FE_WEBP_LOSSY_AP, 30), (fl.FE_WEBP_LOSSY_I4_AP, 99)):
        jobs.append((None, small, fl.make_params(300, 200, quality=q, front_end=fe), None))
    order = np.random.default_rng(7).permutation(len(jobs))  # the four lossy WebP families interleaved in the caller's order
    jobs = [jobs[i] for i in order]
    images, params = [j[1] for j in jobs], [j[2] for j in jobs]
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
    for k, (name, img, p, i4) in enumerate(jobs):
        if name is not None:
            assert outs[k] == _model_of(fl, gpu_state, img, name, i4, quality=p.quality)[0][0], name
    # the same batch in the other order of the two neighbours
    pair = [j for j in jobs if j[0] in ("noise_64x48_q99", "photo_300x200_q75")]
    for a, b in ((0, 1), (1, 0)):
        got = gpu_state.process_batch([pair[a][1], pair[b][1]], [pair[a][2], pair[b][2]])
        assert got[0] == _model_of(fl, gpu_state, pair[a][1], pair[a][0], False, quality=pair[a][2].quality)[0][0]
        assert got[1] == _model_of(fl, gpu_state, pair[b][1], pair[b][0], False, quality=pair[b][2].quality)[0][0]


@pytest.mark.gpu
def test_the_query_level_route(fl, gpu_state, big):
    from PIL import Image
    lossy, i4b, probs = fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS
    want = {}
    for i4 in (False, True):
        want[i4] = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=_fe(fl, i4)))
        (model, _, stats), pl = _model_of(fl, gpu_state, big, "big", i4, w=300, h=200, quality=75)
        assert want[i4] == model and stats["updated"]
        old = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY_I4 if i4 else fl.FE_WEBP_LOSSY))
        assert old == _model_of(fl, gpu_state, big, "big", i4, adapt=False, w=300, h=200, quality=75)[0][0] and len(want[i4]) < len(old)
        bits = lossy | probs | (i4b if i4 else 0)
        for q, fmt, content in ((Q, fl.IN_PNG, fl.Format(fl.ACCEPT_WEBP | bits)), (Q, fl.IN_JPEG, fl.Format(fl.ACCEPT_WEBP | bits)),
                                ("w=300&h=200&quality=75", fl.IN_WEBP, fl.Format(bits))):
            mime, kind, body = gpu_state.process_image(big, q, content, input_format=fmt)
            assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body == want[i4], (i4, q)
        # without the new bit: the non-adaptive file
        mime, kind, body = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | (bits & ~probs)), input_format=fl.IN_PNG)
        assert kind == fl.RESULT_WEBP_STREAM and body == old
    # the new bit alone, and with only _I4: the planes
    for bits in (probs, probs | i4b):
        mime, kind, planes = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | bits), input_format=fl.IN_PNG)
        assert kind == fl.RESULT_WEBP_PLANES and all(np.array_equal(getattr(planes, f), getattr(pl, f)) for f in "yuva")
    # an output over FE_WEBP_LOSSY_I4_AP's limit (120 x 68 macroblocks) with all three bits: FE_WEBP_LOSSY_AP's file
    every = fl.Format(fl.ACCEPT_WEBP | lossy | i4b | probs)
    mime, kind, body = gpu_state.process_image(big, "webp=true&quality=30", every, input_format=fl.IN_PNG)
    assert kind == fl.RESULT_WEBP_STREAM and body == gpu_state.process_pixels(big, fl.make_params(quality=30, front_end=fl.FE_WEBP_LOSSY_AP))
    # file sources: a JPEG file through the query-level entry point gives the stream its decoded pixels give
    img = synth.photo(360, 640, 3, index=41)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=90)
    for i4 in (False, True):
        content = fl.Format(fl.ACCEPT_WEBP | lossy | probs | (i4b if i4 else 0))
        mime, kind, body = gpu_state.process_jpeg(b.getvalue(), Q, content)
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM)
        assert body == gpu_state.process_jpeg_pixels(b.getvalue(), fl.make_params(300, 200, quality=75, front_end=_fe(fl, i4))), i4


@pytest.mark.gpu
def test_sixteen_concurrent_callers_get_identical_bytes(fl, gpu_state, big):
    kinds = [fl.FE_WEBP_LOSSY_AP, fl.FE_WEBP_LOSSY_I4_AP, fl.FE_WEBP_LOSSY, fl.FE_WEBP_LOSSY_AP]
    want = {fe: gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fe)) for fe in set(kinds)}
    assert want[fl.FE_WEBP_LOSSY_AP] == _model_of(fl, gpu_state, big, "big", False, w=300, h=200, quality=75)[0][0]
    assert want[fl.FE_WEBP_LOSSY_I4_AP] == _model_of(fl, gpu_state, big, "big", True, w=300, h=200, quality=75)[0][0]
    got, errors = [None] * 16, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=kinds[i % 4]))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        assert got[i] == want[kinds[i % 4]], i


@pytest.mark.gpu
@pytest.mark.parametrize("i4", (False, True), ids=("i16", "b_pred"))
def test_a_destination_one_byte_short(fl, gpu_state, i4):
    corpus = {name: (img, q) for name, img, q in vp8_ap_cases.corpus(i4)}
    img, q = corpus["patchwork_64x48_q30_a" if i4 else "photo_64x48_q1_a"]
    p = fl.make_params(quality=q, front_end=_fe(fl, i4))
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
