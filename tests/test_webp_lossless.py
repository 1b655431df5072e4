"""FLGPU_FE_WEBP_LOSSLESS: the finished lossless WebP file from the device for the WebP arm at quality 100 (reference
src/handler.rs:286-292, image's lossless encoder after into_rgba8()).  Host half: routing and sizing of the new front end,
and the restated stream (tests/vp8l_model.py) checked against the system's libwebp.  Device half: every stream decodes to
into_rgba8() of the request's FE_NONE pixels and equals the model's bytes, on every entry path."""
import ctypes as C
import io
import threading

import numpy as np
import pytest

import synth
import vp8l_model as vm

Q = "w=300&h=200&webp=true&quality=100"


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


def _jpeg_file(h=120, w=160):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(synth.photo(h, w, 3, index=41)).save(b, format="JPEG", quality=90)
    return b.getvalue()


def _plan_jpeg(fl, data, query, flags):
    lib = fl.load_library()
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_jpeg_plan(data, len(data), query.encode(), flags, C.byref(plan), C.byref(k))
    return rc, k.value, plan


# ---------------------------------------------------------------------------------------------------- host side --

def test_the_bit_turns_the_q100_webp_arm_into_the_stream(fl):
    webp = fl.Format.from_accept_header("image/webp").flags
    for fmt in (fl.IN_PNG, fl.IN_JPEG, fl.IN_OTHER, fl.IN_WEBP):
        for q in ("quality=100", "quality=255"):
            query = f"w=300&h=200&webp=true&{q}"
            rc, kind, plan = _plan(fl, query, webp | fl.ENCODE_WEBP_LOSSLESS, fmt)
            assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM, (fmt, q)
            assert (plan.out_w, plan.out_h, plan.out_c) == (300, 200, 4)
            assert plan.out_bytes == 4 * 300 * 200 and plan.max_out_bytes == vm.max_out_bytes(300, 200)
            # without the bit: the pixels, exactly as before
            rc, kind, plan = _plan(fl, query, webp, fmt)
            assert rc == fl.OK and kind == fl.RESULT_PIXELS and plan.out_bytes == plan.max_out_bytes == 300 * 200 * 4
    # a WebP source that stays WebP (no negotiation needed), crop keeps the source's channels
    rc, kind, plan = _plan(fl, "w=300&h=200&crop=true&quality=100", fl.ENCODE_WEBP_LOSSLESS, fl.IN_WEBP, c=3)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.out_c == 3
    assert plan.out_bytes == 4 * 300 * 200 and plan.max_out_bytes == vm.max_out_bytes(300, 200)
    assert _plan(fl, "w=300&h=200&crop=true&quality=100", 0, fl.IN_WEBP, c=3)[1] == fl.RESULT_PIXELS
    # a JPEG file
    data = _jpeg_file()
    rc, kind, plan = _plan_jpeg(fl, data, Q, webp | fl.ENCODE_WEBP_LOSSLESS)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == vm.max_out_bytes(300, 200)
    rc, kind, plan = _plan_jpeg(fl, data, Q, webp)
    assert rc == fl.OK and kind == fl.RESULT_PIXELS


def test_the_bit_leaves_every_other_outcome_alone(fl):
    for extra in (0, fl.ENCODE_PNG):
        both = fl.Format.from_accept_header("image/webp,image/avif").flags | fl.ENCODE_WEBP_LOSSLESS | extra
        png_kind = fl.RESULT_PNG_STREAM if extra else fl.RESULT_PIXELS
        assert _plan(fl, "w=300&h=200", both, fl.IN_JPEG)[1] == fl.RESULT_JPEG_STREAM
        assert _plan(fl, "w=300&h=200", both, fl.IN_PNG)[1] == png_kind
        assert _plan(fl, "w=300&h=200&quality=100", both, fl.IN_PNG)[1] == png_kind
        assert _plan(fl, "w=300&h=200&webp=true", both, fl.IN_PNG)[1] == fl.RESULT_WEBP_PLANES
        assert _plan(fl, "w=300&h=200&webp=true&quality=99", both, fl.IN_PNG)[1] == fl.RESULT_WEBP_PLANES
        assert _plan(fl, "w=300&h=200&quality=99", both, fl.IN_WEBP)[1] == fl.RESULT_WEBP_PLANES
        assert _plan(fl, "w=300&h=200&avif=true&quality=100", both, fl.IN_PNG)[1] == fl.RESULT_PIXELS
        assert _plan(fl, Q, both, fl.IN_GIF_FRAME)[1] == fl.RESULT_PIXELS
        assert _plan(fl, "w=300&h=200&quality=100", both, fl.IN_OTHER)[1] == fl.RESULT_PIXELS
        assert _plan(fl, "", both, fl.IN_WEBP)[1] == fl.RESULT_AS_IS
        assert _plan(fl, "w=9999&h=9999&webp=true&quality=100", both, fl.IN_PNG)[0] == fl.ERR_PARSE
    # a client that does not accept WebP: the arm is not taken
    assert _plan(fl, Q, fl.ENCODE_WEBP_LOSSLESS, fl.IN_PNG)[1] == fl.RESULT_PIXELS


def test_outputs_over_16384_keep_the_pixels(fl):
    flags = fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSLESS
    for w, h in ((16385, 4), (4, 16385), (20000, 20)):
        for f in (flags, fl.ACCEPT_WEBP):
            rc, kind, plan = _plan(fl, "webp=true&quality=100", f, fl.IN_PNG, w=w, h=h, c=3)
            assert rc == fl.OK and kind == fl.RESULT_PIXELS and (plan.out_w, plan.out_h) == (w, h)
    rc, kind, plan = _plan(fl, "webp=true&quality=100", flags, fl.IN_PNG, w=16384, h=4, c=3)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == vm.max_out_bytes(16384, 4)


def test_plan_output_admits_front_end_6_and_not_5_or_7(fl):
    lib = fl.load_library()
    for w, h, c in ((1, 1, 1), (300, 200, 4), (301, 7, 3), (5000, 1, 2), (1, 16384, 3), (3840, 2160, 3)):
        plan = fl.plan_output(fl.make_params(front_end=fl.FE_WEBP_LOSSLESS), w, h, c)
        assert (plan.out_w, plan.out_h, plan.out_c) == (w, h, c)
        assert plan.out_bytes == 4 * w * h and plan.max_out_bytes == 1024 + (15 * w * h + 1) // 2
    for fe in (5, 7, 8):
        p, plan = fl.make_params(front_end=fe), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), 64, 64, 3, C.byref(plan)) == fl.ERR_INVALID_ARG, fe
    for w, h in ((16385, 1), (1, 16385)):
        p, plan = fl.make_params(front_end=fl.FE_WEBP_LOSSLESS), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), w, h, 3, C.byref(plan)) == fl.ERR_UNSUPPORTED


def _noise(h, w, c, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def model_corpus():
    cols = np.zeros((20, 30, 3), np.uint8)
    cols[:, 1::2] = 255
    alpha = synth.photo(60, 70, 4, index=43)
    alpha[..., 3] = (np.arange(70)[None, :] * 3 + np.arange(60)[:, None]) % 256
    return [
        ("photo_letterbox", synth.photo(200, 300, 4, index=42)),
        ("gradient", (np.arange(256, dtype=np.uint8)[None, :, None] + np.zeros((40, 1, 3), np.uint8))),
        ("noise", _noise(64, 64, 4)),
        ("flat_1x5000", np.full((1, 5000, 3), 9, np.uint8)),
        ("zeros_3x3", np.zeros((3, 3, 4), np.uint8)),
        ("columns", cols),
        ("gray", synth.photo(50, 60, 1, index=44)),
        ("luma_alpha", synth.photo(51, 61, 2, index=45)),
        ("alpha", alpha),
        ("1x1", np.array([[[1, 2, 3, 4]]], np.uint8)),
    ]


def test_the_model_is_a_valid_encoder(fl):
    assert vm.have_decoder(), "libwebp (or Pillow with WebP) is needed to check the streams"
    for name, px in model_corpus():
        data = vm.encode(px)
        h, w = px.shape[:2]
        assert len(data) <= vm.max_out_bytes(w, h), name
        assert np.array_equal(vm.decode_rgba(data), vm.into_rgba8(px)), name


def test_the_header_reads_back(fl):
    for name, px in model_corpus():
        h, w, c = px.shape
        hdr = vm.parse(vm.encode(px))
        assert (hdr["signature"], hdr["width"], hdr["height"], hdr["alpha"], hdr["version"]) == (0x2F, w, h, 1, 0), name
        (sg,), (pred, bits, cache, sub) = hdr["transforms"]
        assert sg == "subtract-green" and pred == "predictor" and bits == 9 and cache == 0
        assert [s["simple"] for s in sub] == [[2], [0], [0], [0], [0]]
        assert hdr["colour_cache"] == 0 and hdr["meta_prefix"] == 0
        assert hdr["codes"][4] == {"simple": [1]}
        res = vm.residuals(px)
        lit, ref, m = vm.tokens(res)
        hists = vm.histograms(res, lit, ref, m)
        for k, code in enumerate(hdr["codes"][:4]):
            used = np.flatnonzero(hists[k])
            if len(used) <= 1:
                assert code == {"simple": [int(used[0]) if len(used) else 0]}, (name, k)
                continue
            assert code["num_cl"] == 19 and code["max_symbol"] == vm.ALPHABETS[k]
            lengths = code["lengths"]
            assert [i for i, x in enumerate(lengths) if x] == list(used), (name, k)
            assert max(lengths) <= 15 and sum(2.0 ** -x for x in lengths if x) == 1.0
            assert max(code["cl_lengths"][16:]) == 0 and max(code["cl_lengths"]) <= 7
        if c in (1, 3):
            assert hdr["codes"][3] == {"simple": [0]}, name   # opaque: every alpha residual is 0


def test_runs_follow_the_4097_rule():
    res = np.zeros((10000, 4), np.uint8)
    res[5000] = 7
    lit, ref, m = vm.tokens(res)
    assert list(np.flatnonzero(lit)) == [0, 4097, 5000, 5001, 9098]
    ends = np.flatnonzero(ref)
    assert list(ends) == [4096, 4999, 9097, 9999] and list(m[ends]) == [4096, 902, 4096, 901]


# ---------------------------------------------------------------------------------------------------- corpus --

def corpus():
    """(name, source picture, make_params kwargs)."""
    big = synth.photo(1080, 1920, 3, index=3)
    big4 = synth.photo(1080, 1920, 4, index=4)
    alpha = synth.photo(90, 130, 4, index=46)
    alpha[..., 3] = (np.arange(130)[None, :] * 2 + np.arange(90)[:, None] * 5) % 256
    flat = np.full((150, 130, 3), 61, np.uint8)
    flat[70:72, 10:20] = 200
    out = [(f"photo{c}", synth.photo(120, 160, c, index=c), {}) for c in (1, 2, 3, 4)]
    out += [
        ("alpha", alpha, {}),
        ("1080p_letterbox", big, dict(w=300, h=200)),
        ("1080p_crop", big, dict(w=300, h=200, crop=True)),
        ("1080p_gray_rgb", big, dict(w=300, h=200, crop=True, grayscale=True)),
        ("1080p_gray_rgba", big4, dict(w=300, h=200, crop=True, grayscale=True)),
        ("1080p_gray_blur", big, dict(w=300, h=200, crop=True, grayscale=True, blur_sigma=4.0)),
        ("odd", synth.photo(77, 131, 3, index=7), {}),
        ("odd4", synth.photo(33, 99, 4, index=8), dict(w=51, h=33)),
        ("1x1", synth.photo(1, 1, 4, index=9), {}),
        ("1x5000", synth.photo(1, 5000, 3, index=10), {}),
        ("5000x1", synth.photo(5000, 1, 2, index=11), {}),
        ("flat_1x5000", np.full((1, 5000, 3), 9, np.uint8), {}),
        ("flat_runs", flat, {}),
        ("flat_4097", np.full((1, 4097 * 3 + 5, 4), 33, np.uint8), {}),
        ("zeros_3x3", np.zeros((3, 3, 4), np.uint8), {}),
        ("edges_checker", synth.edges(200, 300, 4)["checker"], {}),
        ("noise", _noise(200, 300, 4), {}),
    ]
    return out


@pytest.fixture(scope="module")
def streams(fl, gpu_state):
    """name -> (stream, the FE_NONE pixels, params kwargs, source)."""
    res = {}
    for name, img, kw in corpus():
        px = gpu_state.process_pixels(img, fl.make_params(**kw))
        data = gpu_state.process_pixels(img, fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS, **kw))
        res[name] = (data, px, kw, img)
    return res


@pytest.mark.gpu
def test_every_stream_decodes_to_the_fe_none_pixels_and_equals_the_model(fl, streams):
    assert vm.have_decoder()
    bad = []
    for name, (data, px, kw, img) in streams.items():
        h, w, c = px.shape
        assert isinstance(data, bytes) and len(data) <= vm.max_out_bytes(w, h), name
        if not np.array_equal(vm.decode_rgba(data), vm.into_rgba8(px)):
            bad.append(("pixels", name))
        if data != vm.encode(px):
            bad.append(("model", name))
    assert not bad, bad


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state):
    import torch
    img = synth.photo(1080, 1920, 4, index=21)
    p = fl.make_params(300, 200, quality=100, front_end=fl.FE_WEBP_LOSSLESS)
    alone = gpu_state.process_pixels(img, p)
    px = gpu_state.process_pixels(img, fl.make_params(300, 200))
    assert alone == vm.encode(px)
    # 32 concurrent callers through the queue, mixed with JPEG, PNG and pixels
    kinds = [fl.FE_WEBP_LOSSLESS, fl.FE_JPEG, fl.FE_PNG, fl.FE_NONE]
    want = {fe: gpu_state.process_pixels(img, fl.make_params(300, 200, quality=100, front_end=fe)) for fe in kinds}
    got, errors = [None] * 32, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(img, fl.make_params(300, 200, quality=100, front_end=kinds[i % 4]))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(32)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(32):
        fe = kinds[i % 4]
        if fe == fl.FE_NONE:
            assert np.array_equal(got[i], want[fe])
        else:
            assert got[i] == want[fe], (i, fe)
    assert want[fl.FE_WEBP_LOSSLESS] == alone
    # flgpu_transform_batch, with JPEG, PNG and pixel neighbours
    small = img[:500, :700].copy()
    outs = gpu_state.process_batch([img, small, img, img, img],
                                   [p, fl.make_params(300, 200), fl.make_params(300, 200, quality=100, front_end=fl.FE_JPEG),
                                    fl.make_params(300, 200, quality=100, front_end=fl.FE_PNG), p])
    assert outs[0] == alone and outs[4] == alone
    assert outs[2] == want[fl.FE_JPEG] and outs[3] == want[fl.FE_PNG]
    assert np.array_equal(outs[1], gpu_state.process_pixels(small, fl.make_params(300, 200)))
    # flgpu_transform_batch_device + flgpu_batch_results
    n = 3
    src = [torch.from_numpy(img).cuda() for _ in range(n)]
    cap = int(fl.plan_output(p, 1920, 1080, 4).max_out_bytes)
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
    gpu_state.process_batch_device([t.data_ptr() for t in src], [(1080, 1920, 4)] * n, p, [t.data_ptr() for t in dst], [cap] * n,
                                   stream=torch.cuda.current_stream().cuda_stream)
    res = gpu_state.batch_results()
    for i in range(n):
        flags, nbytes = res[i]
        assert flags & fl.IMG_ENCODED
        assert dst[i][:nbytes].cpu().numpy().tobytes() == alone
    # a context of two shards (both on device 0)
    with fl.State(devices=[0, 0]) as two:
        outs = two.process_batch([img] * 4, [p] * 4)
        assert all(o == alone for o in outs)
        assert two.process_pixels(img, p) == alone
    # State::process_image with the opt-in bit: negotiated, quality=255, a WebP source
    accept = fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSLESS)
    for q, fmt, content in ((Q, fl.IN_PNG, accept), ("w=300&h=200&webp=true&quality=255", fl.IN_JPEG, accept),
                            ("w=300&h=200&quality=100", fl.IN_WEBP, fl.Format(fl.ENCODE_WEBP_LOSSLESS))):
        mime, kind, body = gpu_state.process_image(img, q, content, input_format=fmt)
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body == alone, q
    mime, kind, body = gpu_state.process_image(img, Q, fl.Format(fl.ACCEPT_WEBP), input_format=fl.IN_PNG)
    assert kind == fl.RESULT_PIXELS and np.array_equal(body, px)


@pytest.mark.gpu
def test_process_jpeg_gives_the_stream(fl, gpu_state):
    data = _jpeg_file(360, 640)
    accept = fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSLESS)
    mime, kind, body = gpu_state.process_jpeg(data, Q, accept)
    assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM)
    mime, kind, px = gpu_state.process_jpeg(data, Q, fl.Format(fl.ACCEPT_WEBP))
    assert kind == fl.RESULT_PIXELS
    assert np.array_equal(vm.decode_rgba(body), vm.into_rgba8(px))
    assert body == vm.encode(px)
    assert body == gpu_state.process_jpeg_pixels(data, fl.make_params(300, 200, quality=100, front_end=fl.FE_WEBP_LOSSLESS))


@pytest.mark.gpu
def test_too_small_destinations(fl, gpu_state):
    img = synth.photo(200, 300, 3, index=31)
    p = fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS)
    full = gpu_state.process_pixels(img, p)
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # incompressible pictures still fit max_out_bytes exactly
    for c in (3, 4):
        noise = _noise(64, 64, c, seed=9)
        plan = fl.plan_output(p, 64, 64, c)
        data = gpu_state.process_pixels(noise, p, capacity=-int(plan.max_out_bytes))
        assert np.array_equal(vm.decode_rgba(data), vm.into_rgba8(noise)) and data == vm.encode(noise)
    # a batch with one too-small stream: its neighbours are delivered intact
    lib = fl.load_library()
    cap = int(fl.plan_output(p, 300, 200, 3).max_out_bytes)
    caps = [cap, len(full) - 1, cap]
    outs = [np.zeros(cp, np.uint8) for cp in caps]
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(img.ctypes.data, img.nbytes, 300, 200, 3, 0) for _ in range(3)])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(o.ctypes.data, o.nbytes, 0, 0, 0, 0) for o in outs])
    ps = (fl.flgpu_params * 3)(p, p, p)
    rc = lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts)
    assert rc == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0
    for i in (0, 2):
        assert outs[i][:dsts[i].bytes].tobytes() == full
