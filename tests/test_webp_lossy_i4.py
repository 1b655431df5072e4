"""FLGPU_FE_WEBP_LOSSY_I4 on the device: the lossy WebP coder whose macroblocks may be B_PRED.  Every file equals the restated
encoder's (tests/vp8_i4_model.py) on the planes the same request returns with FLGPU_FE_WEBP420 -- which libwebp decodes to exactly
the model's reconstruction (tests/test_webp_lossy_i4_host.py) --, the library's own decoder reads it back to that reconstruction,
and FLGPU_FE_WEBP_LOSSY beside it still writes tests/vp8_model.py's bytes."""
import threading

import numpy as np
import pytest

import synth
import vp8_cases
import vp8_i4_cases
import vp8_i4_model as m4
import vp8_lib

Q = "w=300&h=200&webp=true&quality=75"


def _planes(fl, st, img, **kw):
    return st.process_pixels(img, fl.make_params(front_end=fl.FE_WEBP420, **kw))


def _model_of(fl, st, img, key, **kw):
    """The I4 model's (file, reconstruction, stats) for the request: its planes are what the same request returns with FE_WEBP420."""
    pl = _planes(fl, st, img, **kw)
    return vp8_i4_cases.model(key, pl.y, pl.u, pl.v, kw["quality"], pl.a if pl.has_alpha else None), pl


@pytest.fixture(scope="module")
def big():
    return synth.photo(1080, 1920, 3, index=3)


@pytest.mark.gpu
def test_every_corpus_file_equals_the_model_and_decodes_to_its_reconstruction(fl, gpu_state):
    bad, bad_decode, any_i4 = [], [], False
    for name, img, q in vp8_i4_cases.corpus():
        data = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY_I4))
        (want, rec, stats), pl = _model_of(fl, gpu_state, img, "dev:" + name, quality=q)
        h, w = img.shape[:2]
        assert isinstance(data, bytes) and len(data) <= m4.max_out_bytes(w, h), name
        assert pl.has_alpha == name.endswith("_a") == (data[12:16] == b"VP8X"), name
        if data != want:
            bad.append(name)
            continue
        any_i4 |= bool(stats["i4"].any())
        # the library's own decoder (flgpu_decode_webp_lossy's kernels): the planes before colour conversion, then the pixels
        got = gpu_state.debug_vp8_planes(data, filtered=True)
        pixels = gpu_state.decode_webp_lossy(data)
        theirs = vp8_lib.decode_rgba(data)
        if not all(np.array_equal(g, r) for g, r in zip(got, rec)) or not np.array_equal(pixels, theirs[..., :pixels.shape[2]]):
            bad_decode.append(name)
    assert not bad, bad
    assert not bad_decode, bad_decode
    # (stats() resolves the pending HIP events; the I4 launches are timed under the same counter)
    assert any_i4 and gpu_state.stats()["frontend_launches"] > 0 and gpu_state.debug_get("webp_lossy_ns") > 0


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state, big):
    corpus = {name: (img, q) for name, img, q in vp8_i4_cases.corpus()}
    picks = ["photo_1x1_q75_a", "photo_300x200_q75", "patchwork_64x48_q30_a", "noise_48x48_q99", "photo_16x144_q30", "flat_48x48_q75",
             "edges22_33x15_q30", "noise_128x16_q30"]
    images = [corpus[n][0] for n in picks]
    params = [fl.make_params(quality=corpus[n][1], front_end=fl.FE_WEBP_LOSSY_I4) for n in picks]
    # the same pictures through the I16-only coder, interleaved with everything else a batch can hold
    old = ["photo_300x200_q75", "photo_17x17_q30_a", "noise_64x48_q99"]
    old_corpus = {name: (img, q) for name, img, q in vp8_cases.corpus()}
    for n in old:
        images.append(old_corpus[n][0])
        params.append(fl.make_params(quality=old_corpus[n][1], front_end=fl.FE_WEBP_LOSSY))
    small = big[:500, :700].copy()
    for fe, q in ((fl.FE_JPEG, 75), (fl.FE_WEBP_LOSSY_I4, 30), (fl.FE_PNG, 75), (fl.FE_WEBP_LOSSLESS, 100), (fl.FE_NONE, 75), (fl.FE_WEBP420, 75),
                  (fl.FE_WEBP_LOSSY, 30), (fl.FE_WEBP_LOSSY_I4, 99)):
        images.append(small)
        params.append(fl.make_params(300, 200, quality=q, front_end=fe))
    order = np.random.default_rng(4).permutation(len(images))  # the two lossy WebP families interleaved in the caller's order
    images, params = [images[i] for i in order], [params[i] for i in order]
    names = [(picks + old + [None] * 8)[i] for i in order]
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
    for k, n in enumerate(names):
        if n is None:
            continue
        pl = _planes(fl, gpu_state, images[k], quality=params[k].quality)
        a = pl.a if pl.has_alpha else None
        if params[k].front_end == fl.FE_WEBP_LOSSY_I4:
            assert outs[k] == vp8_i4_cases.model("dev:" + n, pl.y, pl.u, pl.v, params[k].quality, a)[0], n
        else:
            assert outs[k] == vp8_cases.model("dev:" + n, pl.y, pl.u, pl.v, params[k].quality, a)[0], n


@pytest.mark.gpu
def test_the_query_level_route(fl, gpu_state, big):
    p = fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY_I4)
    i4 = gpu_state.process_pixels(big, p)
    (want, _, stats), pl = _model_of(fl, gpu_state, big, "dev:big", w=300, h=200, quality=75)
    assert i4 == want and stats["i4"].any()
    i16 = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY))
    assert i16 == vp8_cases.model("dev:big", pl.y, pl.u, pl.v, 75, None)[0] and len(i4) < len(i16)
    both = fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4)
    for q, fmt, content in ((Q, fl.IN_PNG, both), (Q, fl.IN_JPEG, both),
                            ("w=300&h=200&quality=75", fl.IN_WEBP, fl.Format(fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4))):
        mime, kind, body = gpu_state.process_image(big, q, content, input_format=fmt)
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body == i4, q
    # only the old bit: today's file; only the new one: the planes
    mime, kind, body = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY), input_format=fl.IN_PNG)
    assert kind == fl.RESULT_WEBP_STREAM and body == i16
    mime, kind, planes = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY_I4), input_format=fl.IN_PNG)
    assert kind == fl.RESULT_WEBP_PLANES and all(np.array_equal(getattr(planes, f), getattr(pl, f)) for f in "yuva")
    # an output over the I4 limit (120 x 68 macroblocks) with both bits: FE_WEBP_LOSSY's file
    mime, kind, body = gpu_state.process_image(big, "webp=true&quality=30", both, input_format=fl.IN_PNG)
    assert kind == fl.RESULT_WEBP_STREAM and body == gpu_state.process_pixels(big, fl.make_params(quality=30, front_end=fl.FE_WEBP_LOSSY))


@pytest.mark.gpu
def test_sixteen_concurrent_callers_get_identical_bytes(fl, gpu_state, big):
    kinds = [fl.FE_WEBP_LOSSY_I4, fl.FE_WEBP_LOSSY, fl.FE_JPEG, fl.FE_WEBP_LOSSY_I4]
    want = {fe: gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fe)) for fe in set(kinds)}
    assert want[fl.FE_WEBP_LOSSY_I4] == _model_of(fl, gpu_state, big, "dev:big", w=300, h=200, quality=75)[0][0]
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
def test_a_destination_one_byte_short(fl, gpu_state):
    corpus = {name: (img, q) for name, img, q in vp8_i4_cases.corpus()}
    img, q = corpus["patchwork_64x48_q30_a"]
    p = fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY_I4)
    full = gpu_state.process_pixels(img, p)
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # a batch with one too-small stream: no bytes claimed for it and none written, its neighbours delivered intact
    lib = fl.load_library()
    cap = int(fl.plan_output(p, 64, 48, 4).max_out_bytes)
    caps = [cap, len(full) - 1, cap]
    outs = [np.full(cp, 0xA5, np.uint8) for cp in caps]
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(img.ctypes.data, img.nbytes, 64, 48, 4, 0) for _ in range(3)])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(o.ctypes.data, o.nbytes, 0, 0, 0, 0) for o in outs])
    ps = (fl.flgpu_params * 3)(p, p, p)
    assert lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts) == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0 and (outs[1] == 0xA5).all(), "no partial file"
    for i in (0, 2):
        assert outs[i][:dsts[i].bytes].tobytes() == full
