"""GIF files as sources on the device (csrc/fl_gifdec.hip behind flgpu_decode_gif / flgpu_process_gif): palette lookup,
de-interlacing and the disposal chain are held bit-exact against the numpy model (tests/gif_model.py) applied to the frame list
every file was written from (tests/gif_cases.py); the per-frame pipeline behind it against flgpu_transform_batch fed the model's
frames with the FLGPU_IN_GIF_FRAME parameters, and the reference's lenna.gif against the CPU oracle's Nearest path."""
import ctypes
import os

import numpy as np
import pytest

import gif_cases as gc
import gif_model as gm
import oracle_lib
import synth

pytestmark = pytest.mark.gpu

LENNA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lenna.gif")
PARSE = gc.parse_cases()
UNSUPPORTED = gc.unsupported_cases()


def status_of(fl, fn, *args):
    try:
        fn(*args)
    except fl.FanlinError as e:
        return e.status
    return fl.OK


def test_the_case_list_covers_the_axes():
    """a condition on tests/gif_cases.py, not on the library: the shapes the compose kernel can go wrong at are there"""
    sizes = {(c.width, c.height) for c in (gc.get(n)[2] for n in gc.CASES)}
    assert {(1, 1), (5, 3), (13, 9), (67, 5), (301, 7)} <= sizes           # widths that are no multiple of four pixels a thread
    assert any(w % 4 == 0 for w, h in sizes) and any((w + 3) // 4 * h > 256 for w, h in sizes)   # the 16-byte path; more than one workgroup
    frames = [f for n in gc.CASES for f in gc.get(n)[2].frames]
    assert {f.disposal for f in frames} >= {0, 1, 2, 3, 4, 7}
    assert {f.size[1] for f in frames if f.interlace} >= set(range(1, 10)) | {17}
    assert gc.get("disposal_single_3")[2].frames[0].disposal == 3
    c = gc.get("disposal_2_then_transparent")[2]
    assert c.frames[1].disposal == 2 and c.frames[2].transparent is not None
    assert {len(gc.get(n)[2].frames) for n in gc.CASES if n.startswith("disposal_")} >= {1, 2, 5}


@pytest.mark.parametrize("name", gc.CASES)
def test_decode_equals_the_model(fl, gpu_state, name):
    data, want, c = gc.get(name)
    got = gpu_state.decode_gif(data)
    assert got.shape == want.shape and np.array_equal(got, want)


# query string, and the same request as FLGPU_IN_GIF_FRAME parameters (plan_request: Nearest, no blur, no orientation, FE_NONE)
REQUESTS = [
    ("w=20&h=20", dict(w=20, h=20)),
    ("w=300&h=200", dict(w=300, h=200)),
    ("w=30&h=20&crop=true", dict(w=30, h=20, crop=True)),
    ("w=64&h=20&rgb=1,2,3", dict(w=64, h=20, fill=(1, 2, 3))),
    ("grayscale=true", dict(grayscale=True)),
    ("inverse=true", dict(inverse=True)),
    ("w=50&h=40&grayscale=true&inverse=true&blur=10&webp=true&quality=50", dict(w=50, h=40, grayscale=True, inverse=True, quality=50)),
]


@pytest.mark.parametrize("name", ["disposal_2_then_transparent", "lzw_kwkwk_runs", "canvas_301x7", "random4_07"])
@pytest.mark.parametrize("query,kw", REQUESTS, ids=[q for q, _ in REQUESTS])
def test_process_equals_the_batch_fed_the_models_frames(fl, gpu_state, name, query, kw):
    data, want, c = gc.get(name)
    mime, kind, frames = gpu_state.process_gif(data, query, fl.Format(fl.ACCEPT_WEBP) if "webp" in query else None)
    assert (mime, kind, len(frames)) == ("image/gif", fl.RESULT_PIXELS, len(want))
    params = fl.make_params(filter=fl.FILTER_NEAREST, **kw)
    ref = gpu_state.process_batch([np.ascontiguousarray(f) for f in want], [params] * len(want))
    for got, exp in zip(frames, ref):
        assert got.shape == exp.shape and np.array_equal(got, exp)


def test_an_empty_query_is_as_is(fl, gpu_state):
    data, want, c = gc.get("canvas_13x9")
    before = gpu_state.gif_counters()
    assert gpu_state.process_gif(data, "") == ("image/gif", fl.RESULT_AS_IS, data)
    assert gpu_state.process_gif(data, "rgb=9,9,9&crop=true")[1] == fl.RESULT_AS_IS
    assert gpu_state.gif_counters() == before                                 # nothing was decoded
    unsupported = UNSUPPORTED["frame_beyond_right_edge"]
    assert gpu_state.process_gif(unsupported, "")[1] == fl.RESULT_AS_IS       # as_is never decodes


def test_same_frames_alone_and_after_other_requests(fl, gpu_state):
    names = ["disposal_five_21320", "canvas_300x8", "interlace_h17"]
    alone = {}
    st = fl.State(device=0)
    try:
        for n in names:
            alone[n] = st.decode_gif(gc.get(n)[0])
    finally:
        st.close()
    img = synth.photo(97, 61, 3, index=4)
    for n in names + names[::-1]:
        gpu_state.process_pixels(img, fl.make_params(40, 30))
        gpu_state.decode_gif(gc.get("lzw_fills_table_immediate_clear")[0])
        gpu_state.process_gif(gc.get("canvas_67x5")[0], "w=30&h=20")
        got = gpu_state.decode_gif(gc.get(n)[0])
        assert np.array_equal(got, alone[n]) and np.array_equal(got, gc.get(n)[1]), n


def test_counters_move_by_the_expected_amounts(fl, gpu_state):
    # (that the blob is smaller than the canvases wherever the palettes do not outweigh a toy canvas: tests/test_gif_source_host.py)
    data, want, c = gc.get("tables_local_every_frame")
    blob = fl.debug_gif_blob(data)
    before = gpu_state.gif_counters()
    gpu_state.decode_gif(data)
    after = gpu_state.gif_counters()
    assert {k: after[k] - before[k] for k in after} == dict(gif_sources=1, gif_frames=5, gif_file_bytes=len(data), gif_upload_bytes=len(blob))
    gpu_state.process_gif(data, "w=30&h=20")
    again = gpu_state.gif_counters()
    assert {k: again[k] - after[k] for k in again} == dict(gif_sources=1, gif_frames=5, gif_file_bytes=len(data), gif_upload_bytes=len(blob))


@pytest.mark.parametrize("name,status", [(n, "PARSE") for n in ("bad_signature_magic", "truncated_at_41", "zero_canvas_width", "lzw_code_beyond_next_free",
                                                                 "lzw_fewer_indices_end_code", "no_colour_table_at_all", "unknown_block_introducer")] +
                                        [(n, "UNSUPPORTED") for n in ("no_frames", "frame_zero_width", "frame_beyond_bottom_edge", "min_code_size_9",
                                                                       "index_at_table_size", "frames_4097", "decoded_above_512_mib")])
def test_error_cases_return_their_code_and_leave_the_context_usable(fl, gpu_state, name, status):
    data = PARSE[name] if status == "PARSE" else UNSUPPORTED[name]
    want = fl.ERR_PARSE if status == "PARSE" else fl.ERR_UNSUPPORTED
    lib = fl.load_library()
    before = gpu_state.gif_counters()
    out = np.zeros(4096, np.uint8)
    dst = fl.flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
    frames, kind, fmt, plan = ctypes.c_uint32(), ctypes.c_int(), ctypes.c_int(), fl.flgpu_plan()
    assert lib.flgpu_decode_gif(gpu_state._ctx, data, len(data), ctypes.byref(dst), ctypes.byref(frames)) == want
    big = np.zeros(30 * 20 * 4 * 8, np.uint8)
    dst = fl.flgpu_image(big.ctypes.data, big.nbytes, 0, 0, 0, 0)
    assert lib.flgpu_process_gif(gpu_state._ctx, data, len(data), b"w=30&h=20", 0, ctypes.byref(dst), ctypes.byref(plan), ctypes.byref(frames),
                                 ctypes.byref(kind), ctypes.byref(fmt)) == want
    assert gpu_state.gif_counters() == before and not out.any() and not big.any()     # refused before any device work
    good, frames_want, _ = gc.get("disposal_pair_23")
    assert np.array_equal(gpu_state.decode_gif(good), frames_want)


def test_a_destination_too_small_is_refused(fl, gpu_state):
    data, want, c = gc.get("canvas_13x9")
    lib = fl.load_library()
    out = np.zeros(want.nbytes - 1, np.uint8)
    dst = fl.flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
    frames = ctypes.c_uint32()
    assert lib.flgpu_decode_gif(gpu_state._ctx, data, len(data), ctypes.byref(dst), ctypes.byref(frames)) == fl.ERR_BUFFER_TOO_SMALL
    assert not out.any()


def test_lenna_resized_against_the_cpu_oracle(fl, gpu_state, oracle):
    data = open(LENNA, "rb").read()
    frames = gm.from_blob(fl.debug_gif_blob(data))           # (held against Pillow in tests/test_gif_source_host.py)
    assert np.array_equal(gpu_state.decode_gif(data), frames)
    mime, kind, got = gpu_state.process_gif(data, "w=300&h=200")
    want = oracle.process_pixels(np.ascontiguousarray(frames[0]), 300, 200, filter=oracle_lib.FILTER_NEAREST)
    assert (mime, kind, len(got)) == ("image/gif", fl.RESULT_PIXELS, 1)
    assert got[0].shape == want.shape and np.array_equal(got[0], want)
