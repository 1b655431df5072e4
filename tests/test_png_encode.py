"""FLGPU_FE_PNG: the finished PNG file from the device (reference src/handler.rs:264-273, PngEncoder with
FilterType::Adaptive).  Host half: routing and sizing of the new front end.  Device half: every stream is taken apart
here -- chunk sequence and CRCs, IHDR, zlib header, inflate to the end with the Adler-32 checked, the filter bytes
against a numpy restatement of the png crate's adaptive rule, the pixels against FLGPU_FE_NONE -- over a corpus that
covers every channel count, odd and degenerate sizes, flat, edge and incompressible pictures and the three levels."""
import ctypes as C
import io
import struct
import threading
import zlib

import numpy as np
import pytest

import synth
from png_enc_model import SEG, check_stream, chunks_of, filter_rows, filtered_bytes, max_out_bytes, unfilter  # noqa: F401


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


# ---------------------------------------------------------------------------------------------------- host side --

def test_png_input_with_the_opt_in_bit_gets_the_png_stream(fl):
    rc, kind, plan = _plan(fl, "w=300&h=200", fl.ENCODE_PNG, fl.IN_PNG)
    assert rc == fl.OK and kind == fl.RESULT_PNG_STREAM
    assert (plan.out_w, plan.out_h, plan.out_c) == (300, 200, 4)
    assert plan.out_bytes == filtered_bytes(300, 200, 4)
    assert plan.max_out_bytes == max_out_bytes(300, 200, 4)
    # without the bit: the pixels, exactly as before
    rc, kind, plan = _plan(fl, "w=300&h=200", 0, fl.IN_PNG)
    assert rc == fl.OK and kind == fl.RESULT_PIXELS and plan.out_bytes == plan.max_out_bytes == 300 * 200 * 4


def test_the_bit_leaves_every_other_outcome_alone(fl):
    both = fl.Format.from_accept_header("image/webp,image/avif").flags | fl.ENCODE_PNG
    assert _plan(fl, "w=300&h=200", both, fl.IN_JPEG)[1] == fl.RESULT_JPEG_STREAM
    assert _plan(fl, "w=300&h=200", both, fl.IN_GIF_FRAME)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200&webp=true", both, fl.IN_PNG)[1] == fl.RESULT_WEBP_PLANES
    assert _plan(fl, "w=300&h=200&avif=true", both, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200", both, fl.IN_OTHER)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200", both, fl.IN_WEBP)[1] == fl.RESULT_WEBP_PLANES
    assert _plan(fl, "", both, fl.IN_PNG)[1] == fl.RESULT_AS_IS
    assert _plan(fl, "w=9999&h=9999", both, fl.IN_PNG)[0] == fl.ERR_PARSE


def test_plan_output_admits_front_end_4_only(fl):
    lib = fl.load_library()
    for w, h, c in ((1, 1, 1), (300, 200, 4), (301, 7, 3), (4000, 1, 2), (3840, 2160, 3)):
        plan = fl.plan_output(fl.make_params(front_end=fl.FE_PNG), w, h, c)
        assert plan.out_bytes == filtered_bytes(w, h, c) and plan.max_out_bytes == max_out_bytes(w, h, c)
    p = fl.make_params(front_end=5)
    plan = fl.flgpu_plan()
    assert lib.flgpu_plan_output(C.byref(p), 64, 64, 3, C.byref(plan)) == fl.ERR_INVALID_ARG


# (the stream checker and the filter model: png_enc_model.py)

# ---------------------------------------------------------------------------------------------------- corpus --

def _noise(h, w, c, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def corpus():
    """(name, source picture, make_params kwargs)."""
    big = synth.photo(1080, 1920, 3, index=3)
    big4 = synth.photo(1080, 1920, 4, index=4)
    out = []
    for c in (1, 2, 3, 4):
        out.append((f"photo{c}", synth.photo(120, 160, c, index=c), {}))
    out += [
        ("1080p_letterbox", big, dict(w=300, h=200)),
        ("1080p_crop", big, dict(w=300, h=200, crop=True)),
        ("1080p_gray_rgb", big, dict(w=300, h=200, crop=True, grayscale=True)),
        ("1080p_gray_rgba", big4, dict(w=300, h=200, crop=True, grayscale=True)),
        ("1080p_blur", big, dict(w=300, h=200, blur_sigma=10.0)),
        ("odd", synth.photo(77, 131, 3, index=7), {}),
        ("odd4", synth.photo(33, 99, 4, index=8), dict(w=51, h=33)),
        ("1x1", synth.photo(1, 1, 4, index=9), {}),
        ("1x4000", synth.photo(4000, 1, 3, index=10), {}),
        ("4000x1", synth.photo(1, 4000, 2, index=11), {}),
        ("edges_checker", synth.edges(200, 300, 4)["checker"], {}),
        ("edges_impulse", synth.edges(200, 300, 3)["impulse"], {}),
        ("flat", np.full((200, 300, 4), 77, np.uint8), {}),
        ("noise", _noise(200, 300, 4), {}),
    ]
    return out


@pytest.fixture(scope="module")
def streams(fl, gpu_state):
    """name -> (quality -> stream, the FE_NONE pixels, params kwargs, source)."""
    res = {}
    for name, img, kw in corpus():
        px = gpu_state.process_pixels(img, fl.make_params(**kw))
        per_q = {}
        for q in (30, 75, 95):
            per_q[q] = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_PNG, **kw))
        res[name] = (per_q, px, kw, img)
    return res


@pytest.mark.gpu
def test_every_stream_is_a_valid_png_of_the_fe_none_pixels(fl, streams):
    bars, over = [], []
    totals = {30: 0, 75: 0}
    for name, (per_q, px, kw, img) in streams.items():
        h, w, c = px.shape
        for q, data in per_q.items():
            assert isinstance(data, bytes)
            assert len(data) <= max_out_bytes(w, h, c), name
            z, raw = check_stream(data, px, q)
            if q == 75:
                ref = len(zlib.compress(raw, 6))
                bars.append((name, len(z), ref))
                if len(z) > 1.10 * ref + 1024:
                    over.append(("default", name, len(z), ref))
            if q == 95:
                ref = len(zlib.compress(raw, 1))
                if len(z) > 1.20 * ref + 1024:
                    over.append(("fast", name, len(z), ref))
            if q in totals:
                totals[q] += len(z)
    print("default-level stream / zlib -6:", ", ".join(f"{n} {a}/{b}" for n, a, b in bars))
    assert not over, over
    assert totals[30] <= totals[75], totals


@pytest.mark.gpu
def test_noise_takes_the_stored_fallback(fl, streams):
    per_q, px, _, _ = streams["noise"]
    h, w, c = px.shape
    f = filtered_bytes(w, h, c)
    for q, data in per_q.items():
        z = b"".join(b for t, b in chunks_of(data)[1:-1])
        assert len(z) <= f + 5 * ((f + SEG - 1) // SEG) * 2 + 6, len(z)   # stored blocks: no growth beyond their headers
        assert len(data) <= max_out_bytes(w, h, c)


@pytest.mark.gpu
def test_a_4k_source(fl, gpu_state):
    img = synth.photo(2160, 3840, 3, index=12)
    data = gpu_state.process_pixels(img, fl.make_params(front_end=fl.FE_PNG))
    check_stream(data, img, 75)


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state):
    import torch
    img = synth.photo(1080, 1920, 4, index=21)
    p = fl.make_params(300, 200, quality=75, front_end=fl.FE_PNG)
    alone = gpu_state.process_pixels(img, p)
    check_stream(alone, gpu_state.process_pixels(img, fl.make_params(300, 200)), 75)
    # 32 concurrent callers through the queue, PNG mixed with JPEG, WebP planes and pixels
    kinds = [fl.FE_PNG, fl.FE_JPEG, fl.FE_WEBP420, fl.FE_NONE]
    want = {fe: gpu_state.process_pixels(img, fl.make_params(300, 200, quality=75, front_end=fe)) for fe in kinds}
    got, errors = [None] * 32, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(img, fl.make_params(300, 200, quality=75, front_end=kinds[i % 4]))
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
        if fe == fl.FE_WEBP420:
            assert np.array_equal(got[i].y, want[fe].y) and np.array_equal(got[i].u, want[fe].u)
        elif fe == fl.FE_NONE:
            assert np.array_equal(got[i], want[fe])
        else:
            assert got[i] == want[fe]
    assert want[fl.FE_PNG] == alone
    # flgpu_transform_batch
    outs = gpu_state.process_batch([img, img[:500, :700].copy(), img], [p, fl.make_params(300, 200), p])
    assert outs[0] == alone and outs[2] == alone
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
    # State::process_image with the opt-in bit
    mime, kind, body = gpu_state.process_image(img, "w=300&h=200", fl.Format(fl.ENCODE_PNG), input_format=fl.IN_PNG)
    assert (mime, kind) == ("image/png", fl.RESULT_PNG_STREAM) and body == alone
    mime, kind, body = gpu_state.process_image(img, "w=300&h=200", fl.Format(0), input_format=fl.IN_PNG)
    assert kind == fl.RESULT_PIXELS and isinstance(body, np.ndarray)


@pytest.mark.gpu
def test_too_small_destinations(fl, gpu_state):
    img = synth.photo(200, 300, 3, index=31)
    p = fl.make_params(quality=75, front_end=fl.FE_PNG)
    full = gpu_state.process_pixels(img, p)
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # an incompressible picture still fits max_out_bytes exactly
    noise = _noise(64, 64, 4, seed=9)
    plan = fl.plan_output(p, 64, 64, 4)
    data = gpu_state.process_pixels(noise, p, capacity=-int(plan.max_out_bytes))
    check_stream(data, noise, 75)
    # a batch with one too-small PNG: its neighbours are delivered intact
    lib = fl.load_library()
    imgs = [img, img, img]
    caps = [plan_cap := int(fl.plan_output(p, 300, 200, 3).max_out_bytes), len(full) - 1, plan_cap]
    outs = [np.zeros(cp, np.uint8) for cp in caps]
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(a.ctypes.data, a.nbytes, 300, 200, 3, 0) for a in imgs])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(o.ctypes.data, o.nbytes, 0, 0, 0, 0) for o in outs])
    ps = (fl.flgpu_params * 3)(p, p, p)
    rc = lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts)
    assert rc == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0
    for i in (0, 2):
        assert outs[i][:dsts[i].bytes].tobytes() == full
