"""GIF files finished on the device (csrc/fl_gif.hip behind flgpu_process_gif with FLGPU_ENCODE_GIF): the file is held byte for
byte against the numpy model (tests/gif_enc_model.py) applied to the pixels the same call returns without the bit; the model's
files are held against the library's own decoder and Pillow in tests/test_gif_encode_host.py.  A file with a frame above 256
colours must come back as exactly those pixels."""
import ctypes
import os
import threading

import numpy as np
import pytest

import gif_enc_cases as ec
import gif_enc_model as em

pytestmark = pytest.mark.gpu

LENNA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lenna.gif")


def run(fl, st, data, query):
    """(the frames without the bit, kind with the bit, payload with the bit)"""
    mime, kind, frames = st.process_gif(data, query)
    assert (mime, kind) == ("image/gif", fl.RESULT_PIXELS)
    mime, kind, payload = st.process_gif(data, query, fl.Format(fl.ENCODE_GIF))
    assert mime == "image/gif"
    return np.stack(frames), kind, payload


def expect(fl, frames, kind, payload):
    """the outcome the frames' colour counts ask for"""
    want = em.encode_file(frames)
    if want is None:
        assert kind == fl.RESULT_PIXELS and np.array_equal(np.stack(payload), frames)
    else:
        assert kind == fl.RESULT_GIF_STREAM and isinstance(payload, bytes)
        assert len(payload) == len(want) and payload == want
    return want


@pytest.mark.parametrize("name", ec.CASES)
def test_the_file_equals_the_model(fl, gpu_state, name):
    data, canvases, c = ec.get(name)
    before = gpu_state.gif_encode_counters()
    frames, kind, payload = run(fl, gpu_state, data, c.query)
    if c.query == ec.IDENTITY:
        assert np.array_equal(frames, canvases)            # the case's properties (tests/test_gif_encode_host.py) are the encoder's input's
    if c.query == "grayscale=true":
        assert frames.shape[-1] == 2
    want = expect(fl, frames, kind, payload)
    assert (want is None) == c.fallback
    after = gpu_state.gif_encode_counters()
    moved = {k: after[k] - before[k] for k in after}
    assert moved == (dict(gif_encoded=0, gif_encode_fallbacks=1, gif_encoded_bytes=0) if c.fallback else
                     dict(gif_encoded=1, gif_encode_fallbacks=0, gif_encoded_bytes=len(want)))
    if want is not None and (frames[..., -1] == 255).all():
        # opaque frames: the library's own decoder gives the frames back
        rgba = frames if frames.shape[-1] == 4 else np.concatenate([frames[..., :1]] * 3 + [frames[..., 1:]], -1)
        assert np.array_equal(gpu_state.decode_gif(payload), rgba)


def test_a_fallback_leaves_the_context_usable(fl, gpu_state):
    data, canvases, c = ec.get("fallback_in_the_middle")
    frames, kind, payload = run(fl, gpu_state, data, c.query)
    assert [em.colours_of(f) for f in frames] == [256, 257, 4] and kind == fl.RESULT_PIXELS
    assert np.array_equal(np.stack(payload), frames)
    for name in ("colours_256", "frames_70"):
        d, cv, cc = ec.get(name)
        assert gpu_state.process_gif(d, cc.query, fl.Format(fl.ENCODE_GIF))[2] == em.encode_file(cv)
    assert np.array_equal(np.stack(gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF))[2]), frames)


def test_twice_the_same_bytes(fl, gpu_state):
    for name in ("noise_256_colours_three_segments", "transparent_grayscale", "pixels_2S_plus_1"):
        data, canvases, c = ec.get(name)
        a = gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF))
        b = gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF))
        assert a[1] == b[1] == fl.RESULT_GIF_STREAM and a[2] == b[2]


def test_four_threads_on_one_context(fl, gpu_state):
    names = ["noise_256_colours_three_segments", "frames_70", "colours_300", "tables_of_different_sizes", "constant_frame", "transparent_partial_first_frame"]
    want = {n: em.encode_file(ec.get(n)[1]) for n in names}
    errors = []

    def work(k):
        try:
            for r in range(3):
                for n in names[k % 2::2] + names[(k + 1) % 2::2]:
                    data, canvases, c = ec.get(n)
                    mime, kind, payload = gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF))
                    if want[n] is None:
                        assert kind == fl.RESULT_PIXELS and np.array_equal(np.stack(payload), canvases), n
                    else:
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
    data, canvases, c = ec.get("tables_of_different_sizes")
    lib = fl.load_library()
    plan, kind, fmt, frames = fl.flgpu_plan(), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint32()
    flags = fl.ENCODE_GIF
    assert lib.flgpu_process_gif_plan(data, len(data), c.query.encode(), flags, ctypes.byref(plan), ctypes.byref(frames), ctypes.byref(kind)) == fl.OK
    need = 64 + frames.value * int(plan.max_out_bytes)
    assert kind.value == fl.RESULT_GIF_STREAM and plan.max_out_bytes == max(plan.out_bytes, em.max_frame_bytes(32 * 16))
    before = (gpu_state.gif_counters(), gpu_state.gif_encode_counters())
    out = np.zeros(need, np.uint8)
    dst = fl.flgpu_image(out.ctypes.data, need - 1, 0, 0, 0, 0)
    assert lib.flgpu_process_gif(gpu_state._ctx, data, len(data), c.query.encode(), flags, ctypes.byref(dst), ctypes.byref(plan), ctypes.byref(frames),
                                 ctypes.byref(kind), ctypes.byref(fmt)) == fl.ERR_BUFFER_TOO_SMALL
    assert not out.any() and (gpu_state.gif_counters(), gpu_state.gif_encode_counters()) == before
    # the same buffer is enough for the call without the bit, which wants frames x out_bytes only
    assert lib.flgpu_process_gif(gpu_state._ctx, data, len(data), c.query.encode(), 0, ctypes.byref(dst), ctypes.byref(plan), ctypes.byref(frames),
                                 ctypes.byref(kind), ctypes.byref(fmt)) == fl.OK and kind.value == fl.RESULT_PIXELS
    dst = fl.flgpu_image(out.ctypes.data, need, 0, 0, 0, 0)
    assert lib.flgpu_process_gif(gpu_state._ctx, data, len(data), c.query.encode(), flags, ctypes.byref(dst), ctypes.byref(plan), ctypes.byref(frames),
                                 ctypes.byref(kind), ctypes.byref(fmt)) == fl.OK
    assert kind.value == fl.RESULT_GIF_STREAM and dst.flags & fl.IMG_ENCODED and (dst.width, dst.height) == (32, 16)
    assert out[:dst.bytes].tobytes() == em.encode_file(canvases)


def test_as_is_and_errors_behave_as_without_the_bit(fl, gpu_state):
    import gif_cases as gc
    data = ec.get("colours_16")[0]
    before = gpu_state.gif_encode_counters()
    assert gpu_state.process_gif(data, "", fl.Format(fl.ENCODE_GIF)) == ("image/gif", fl.RESULT_AS_IS, data)
    for cases, status in ((gc.parse_cases(), fl.ERR_PARSE), (gc.unsupported_cases(), fl.ERR_UNSUPPORTED)):
        name = sorted(cases)[0]
        with pytest.raises(fl.FanlinError) as e:
            gpu_state.process_gif(cases[name], "w=30&h=20", fl.Format(fl.ENCODE_GIF))
        assert e.value.status == status
    assert gpu_state.gif_encode_counters() == before


def test_lenna_cropped_is_a_stream_that_decodes_to_the_pixels(fl, gpu_state):
    data = open(LENNA, "rb").read()
    frames, kind, payload = run(fl, gpu_state, data, "w=300&h=200&crop=true")
    assert frames.shape == (1, 200, 300, 4) and max(em.colours_of(f) for f in frames) <= 256
    expect(fl, frames, kind, payload)
    assert kind == fl.RESULT_GIF_STREAM and np.array_equal(gpu_state.decode_gif(payload), frames)
    assert fl.gif_info(payload)["supported"] == 1


def test_lenna_on_a_frame_follows_its_colour_count(fl, gpu_state):
    data = open(LENNA, "rb").read()
    frames, kind, payload = run(fl, gpu_state, data, "w=300&h=200")
    colours = max(em.colours_of(f) for f in frames)
    print("lenna.gif w=300&h=200:", colours, "colours")
    assert (kind == fl.RESULT_PIXELS) == (colours > 256)      # 256 of the picture and the frame's 32, 32, 32: the NeuQuant branch
    expect(fl, frames, kind, payload)


def test_the_encode_kernels_are_timed(fl, gpu_state):
    data, canvases, c = ec.get("frames_70")
    gpu_state.stats()
    before = gpu_state.debug_get("gif_encode_ns")
    gpu_state.process_gif(data, c.query, fl.Format(fl.ENCODE_GIF))
    gpu_state.stats()                                          # (resolves the pending HIP events)
    assert gpu_state.debug_get("gif_encode_ns") > before
