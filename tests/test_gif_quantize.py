"""GIF files with frames above 256 colours, finished on the device (csrc/fl_gifquant.hip behind flgpu_process_gif with FLGPU_ENCODE_GIF |
FLGPU_ENCODE_GIF_QUANTIZE): the file is held byte for byte against the numpy model (tests/gif_quant_model.py) applied to the pixels
the same call returns without the bits; the model itself is held against Pillow, the library's host decoder and the host twin in
tests/test_gif_quantize_host.py.  Without the new bit the same inputs must still come back as pixels."""
import ctypes
import os
import threading

import numpy as np
import pytest

import gif_enc_cases as ec
import gif_enc_model as em
import gif_quant_cases as qc
import gif_quant_model as qm

pytestmark = pytest.mark.gpu

LENNA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lenna.gif")
_WANT = {}


def both(fl):
    return fl.Format(fl.ENCODE_GIF | fl.ENCODE_GIF_QUANTIZE)


def pixels_of(fl, st, data, query):
    mime, kind, frames = st.process_gif(data, query)
    assert (mime, kind) == ("image/gif", fl.RESULT_PIXELS)
    return np.stack(frames)


def want_of(fl, st, name):
    """(the frames the encoder sees, the model's file, the marked frames): computed once per case"""
    if name not in _WANT:
        data, canvases, c = qc.get(name)
        frames = pixels_of(fl, st, data, c.query)
        if c.query == qc.IDENTITY:
            assert np.array_equal(frames, canvases)
        _WANT[name] = (frames, qm.encode_file(frames), sum(qm.marked(f) for f in frames))
    return _WANT[name]


def shown(frames):
    """what a decoder shows for the model's file: every frame over the one before it (disposal 1), from an empty canvas"""
    canvas = np.zeros(frames[0].shape[:2] + (4,), np.uint8)
    out = []
    for f in frames:
        rgba = qm.to_rgba(f)
        keep = rgba[..., 3] != 0
        canvas[keep] = rgba[keep]
        out.append(canvas.copy())
    return np.stack(out)


@pytest.mark.parametrize("name", qc.CASES)
def test_the_file_equals_the_model(fl, gpu_state, name):
    data, canvases, c = qc.get(name)
    frames, want, marked = want_of(fl, gpu_state, name)
    assert marked >= 1 and want is not None
    if name == "grayscale_256_and_clear":
        assert frames.shape == (1, 10, 30, 2) and em.colours_of(frames[0]) == 257
    if name == "eight_frames_all_marked":
        assert marked == 8
    # with ENCODE_GIF alone: the pixels, and a fallback counted -- nothing changes without the new bit
    before = dict(gpu_state.gif_encode_counters(), q=gpu_state.gif_quantized_frames())
    mime, kind, payload = gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF))
    assert kind == fl.RESULT_PIXELS and np.array_equal(np.stack(payload), frames)
    after = dict(gpu_state.gif_encode_counters(), q=gpu_state.gif_quantized_frames())
    assert {k: after[k] - before[k] for k in after} == dict(gif_encoded=0, gif_encode_fallbacks=1, gif_encoded_bytes=0, q=0)
    # with both: the model's file
    mime, kind, payload = gpu_state.process_gif(data, c.query, both(fl))
    assert (mime, kind) == ("image/gif", fl.RESULT_GIF_STREAM) and isinstance(payload, bytes)
    assert len(payload) == len(want) and payload == want
    moved = dict(gpu_state.gif_encode_counters(), q=gpu_state.gif_quantized_frames())
    assert {k: moved[k] - after[k] for k in moved} == dict(gif_encoded=1, gif_encode_fallbacks=0, gif_encoded_bytes=len(want), q=marked)
    # the library's own decoder reads it back to the model's frames
    assert np.array_equal(gpu_state.decode_gif(payload), shown(frames))


@pytest.mark.parametrize("name", ["colours_256", "tables_of_different_sizes", "transparent_grayscale", "pixels_2S_plus_1"])
def test_no_frame_above_256_colours_gives_the_same_bytes_with_and_without_the_bit(fl, gpu_state, name):
    data, canvases, c = ec.get(name)
    before = gpu_state.gif_quantized_frames()
    a = gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF))
    b = gpu_state.process_gif(data, c.query, both(fl))
    assert a[1] == b[1] == fl.RESULT_GIF_STREAM and a[2] == b[2] and gpu_state.gif_quantized_frames() == before
    if c.query == ec.IDENTITY:
        assert b[2] == em.encode_file(canvases) == qm.encode_file(canvases)


def test_the_new_bit_alone_does_nothing(fl, gpu_state):
    data, canvases, c = qc.get("colours_257")
    before = dict(gpu_state.gif_encode_counters(), q=gpu_state.gif_quantized_frames())
    mime, kind, payload = gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF_QUANTIZE))
    assert kind == fl.RESULT_PIXELS and np.array_equal(np.stack(payload), canvases)
    assert dict(gpu_state.gif_encode_counters(), q=gpu_state.gif_quantized_frames()) == before


def test_lenna_on_a_frame_is_a_stream_that_equals_the_model(fl, gpu_state):
    data = open(LENNA, "rb").read()
    frames = pixels_of(fl, gpu_state, data, "w=300&h=200")
    assert frames.shape == (1, 200, 300, 4) and em.colours_of(frames[0]) > 256        # the picture's 256 and the frame's 32, 32, 32
    mime, kind, payload = gpu_state.process_gif(data, "w=300&h=200", both(fl))
    assert kind == fl.RESULT_GIF_STREAM and payload == qm.encode_file(frames)
    assert fl.gif_info(payload)["supported"] == 1 and np.array_equal(gpu_state.decode_gif(payload), shown(frames))
    err = qm.squared_error(frames[0], qm.to_rgba(frames[0]))
    print("lenna.gif w=300&h=200: %d colours, mean squared error %.4f" % (em.colours_of(frames[0]), err))
    assert err < 1.0                                                                   # 257 colours into 256: two of them share an entry


def test_twice_the_same_bytes(fl, gpu_state):
    for name in ("dark_s1", "one_clear_pixel", "eight_frames_all_marked"):
        data, canvases, c = qc.get(name)
        a = gpu_state.process_gif(data, c.query, both(fl))
        b = gpu_state.process_gif(data, c.query, both(fl))
        assert a[1] == b[1] == fl.RESULT_GIF_STREAM and a[2] == b[2] == want_of(fl, gpu_state, name)[1]


def test_four_threads_on_one_context(fl, gpu_state):
    names = ["colours_272", "fallback_in_the_middle", "eight_frames_all_marked", "ties_between_axes", "pixels_285", "colours_4097"]
    want = {n: want_of(fl, gpu_state, n)[1] for n in names}
    plain = ec.get("frames_70")
    want["frames_70"] = em.encode_file(plain[1])
    errors = []

    def work(k):
        try:
            for r in range(2):
                for n in names[k % 2::2] + names[(k + 1) % 2::2] + ["frames_70"]:
                    data, canvases, c = plain if n == "frames_70" else qc.get(n)
                    mime, kind, payload = gpu_state.process_gif(data, c.query, both(fl))
                    assert kind == fl.RESULT_GIF_STREAM and payload == want[n], n
        except BaseException as e:      # noqa: B036 (an assertion in a thread must reach the test)
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_a_destination_one_byte_short_is_refused_before_any_device_work(fl, gpu_state):
    data, canvases, c = qc.get("colours_272")
    lib = fl.load_library()
    plan, kind, fmt, frames = fl.flgpu_plan(), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint32()
    flags = fl.ENCODE_GIF | fl.ENCODE_GIF_QUANTIZE
    assert lib.flgpu_process_gif_plan(data, len(data), c.query.encode(), flags, ctypes.byref(plan), ctypes.byref(frames), ctypes.byref(kind)) == fl.OK
    need = 64 + frames.value * int(plan.max_out_bytes)
    assert kind.value == fl.RESULT_GIF_STREAM and plan.max_out_bytes == max(plan.out_bytes, em.max_frame_bytes(17 * 16))
    before = (gpu_state.gif_counters(), gpu_state.gif_encode_counters(), gpu_state.gif_quantized_frames())
    out = np.zeros(need, np.uint8)
    dst = fl.flgpu_image(out.ctypes.data, need - 1, 0, 0, 0, 0)
    assert lib.flgpu_process_gif(gpu_state._ctx, data, len(data), c.query.encode(), flags, ctypes.byref(dst), ctypes.byref(plan), ctypes.byref(frames),
                                 ctypes.byref(kind), ctypes.byref(fmt)) == fl.ERR_BUFFER_TOO_SMALL
    assert not out.any() and (gpu_state.gif_counters(), gpu_state.gif_encode_counters(), gpu_state.gif_quantized_frames()) == before
    dst = fl.flgpu_image(out.ctypes.data, need, 0, 0, 0, 0)
    assert lib.flgpu_process_gif(gpu_state._ctx, data, len(data), c.query.encode(), flags, ctypes.byref(dst), ctypes.byref(plan), ctypes.byref(frames),
                                 ctypes.byref(kind), ctypes.byref(fmt)) == fl.OK
    assert kind.value == fl.RESULT_GIF_STREAM and dst.flags & fl.IMG_ENCODED and (dst.width, dst.height) == (17, 16)
    assert out[:dst.bytes].tobytes() == want_of(fl, gpu_state, "colours_272")[1]
