"""The GIF encoder without a GPU: what FLGPU_ENCODE_GIF changes in the plans (and what it must not), the numpy model of the file the
device writes (tests/gif_enc_model.py) held against the library's own host decoder and against Pillow, the worst-case bound, and
the conditions on the case list (tests/gif_enc_cases.py) that make the device test (tests/test_gif_encode.py) worth running."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import gif_enc_cases as ec
import gif_enc_model as em
import gif_model as gm
import gif_write as gw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = em.SEG
MODEL_CASES = [n for n in ec.CASES if ec.get(n)[2].query == ec.IDENTITY]
ENCODED = [n for n in MODEL_CASES if not ec.get(n)[2].fallback]


def gif_plan(fl, data, query, flags):
    plan, kind, frames = fl.flgpu_plan(), ctypes.c_int(), ctypes.c_uint32()
    rc = fl.load_library().flgpu_process_gif_plan(data, len(data), query.encode(), flags, ctypes.byref(plan), ctypes.byref(frames), ctypes.byref(kind))
    return rc, kind.value, frames.value, {n: getattr(plan, n) for n, _ in fl.flgpu_plan._fields_}


def luma_alpha(canvases):
    """some LumaA8 frames for the model: the encoder's two-channel input"""
    return np.stack([canvases[..., :3].astype(np.uint32).sum(-1) // 3, canvases[..., 3]], -1).astype(np.uint8)


# ---- routing --------------------------------------------------------------------------------------------------------------------

def test_the_constants_are_mirrored(fl):
    header = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_gif.h")).read()
    seg = int(re.search(r"constexpr uint32_t kGifSegIndices = (\d+);", header).group(1))
    assert seg == S == fl.GIF_SEG_INDICES and seg <= 3838       # 4,096 - 258: a segment cannot fill the table at code size 8
    api = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert re.search(r"#define FLGPU_ENCODE_GIF 0x400u", api) and re.search(r"FLGPU_RESULT_GIF_STREAM = 6\b", api)
    assert (fl.ENCODE_GIF, fl.RESULT_GIF_STREAM) == (0x400, 6)
    assert re.search(r"#define FLGPU_ABI_VERSION 6\b", api)
    for px in (1, S - 1, S, S + 1, 300 * 200):
        assert fl.gif_max_frame_bytes(px) == em.max_frame_bytes(px)
    d = (12 * (S + 1 + 1 + 2) + 7) // 8
    assert em.max_frame_bytes(S + 1) == 8 + 10 + 768 + 1 + d + (d + 254) // 255 + 1


@pytest.mark.parametrize("query,shape", [("w=30&h=20", (30, 20, 4)), ("webp=true", (67, 5, 4)), ("grayscale=true", (67, 5, 2)),
                                         ("w=300&h=200&crop=true", (300, 200, 4))])
def test_the_bit_turns_the_gif_plan_into_a_stream(fl, query, shape):
    import gif_cases as gc
    data = gc.get("canvas_67x5")[0]
    rc0, kind0, frames0, plan0 = gif_plan(fl, data, query, fl.ACCEPT_WEBP)
    rc1, kind1, frames1, plan1 = gif_plan(fl, data, query, fl.ACCEPT_WEBP | fl.ENCODE_GIF)
    w, h, c = shape
    # without the bit exactly as before: pixels, max_out_bytes = out_bytes
    assert (rc0, kind0, frames0, plan0["out_w"], plan0["out_h"], plan0["out_c"], plan0["out_bytes"], plan0["max_out_bytes"]) == \
        (fl.OK, fl.RESULT_PIXELS, 3, w, h, c, w * h * c, w * h * c)
    assert (rc1, kind1, frames1) == (fl.OK, fl.RESULT_GIF_STREAM, 3)
    assert plan1["max_out_bytes"] == max(w * h * c, em.max_frame_bytes(w * h))
    assert {k: v for k, v in plan1.items() if k != "max_out_bytes"} == {k: v for k, v in plan0.items() if k != "max_out_bytes"}


def test_the_bit_changes_nothing_elsewhere(fl):
    import gif_cases as gc
    lib = fl.load_library()
    data = gc.get("canvas_67x5")[0]
    for query in ("", "rgb=9,9,9&crop=true"):                        # as_is
        assert gif_plan(fl, data, query, fl.ENCODE_GIF)[:3] == (fl.OK, fl.RESULT_AS_IS, 3)
    assert gif_plan(fl, data, "w=abc", fl.ENCODE_GIF)[0] == fl.ERR_PARSE
    assert gif_plan(fl, data, "w=10&h=10", fl.ENCODE_GIF)[0] == fl.ERR_PARSE        # the size gate
    img = fl.flgpu_image(None, 0, 64, 48, 4, 0)
    for fmt in (fl.IN_JPEG, fl.IN_PNG, fl.IN_WEBP, fl.IN_OTHER):
        for query in ("w=40&h=30", "w=40&h=30&webp=true&quality=100", "grayscale=true", ""):
            for accept in (0, fl.ACCEPT_WEBP, fl.ACCEPT_WEBP | fl.ENCODE_PNG | fl.ENCODE_WEBP_LOSSLESS):
                got = []
                for flags in (accept, accept | fl.ENCODE_GIF):
                    plan, kind = fl.flgpu_plan(), ctypes.c_int()
                    rc = lib.flgpu_process_image_plan(ctypes.byref(img), 1, query.encode(), flags, fmt, ctypes.byref(plan), ctypes.byref(kind))
                    got.append((rc, kind.value, bytes(plan)))
                assert got[0] == got[1] and got[0][1] != fl.RESULT_GIF_STREAM, (fmt, query, accept)


# ---- conditions on the case list --------------------------------------------------------------------------------------------------

def test_the_case_list_covers_the_axes():
    px = {ec.get(n)[1].shape[1] * ec.get(n)[1].shape[2] for n in MODEL_CASES}
    assert {1, S - 1, S, S + 1, 2 * S + 1} <= px and max(px) <= 128 * 64
    colours = {max(em.colours_of(f) for f in ec.get(n)[1]) for n in MODEL_CASES}
    assert {1, 2, 3, 4, 5, 16, 17, 128, 129, 255, 256, 257, 300} <= colours
    for n in MODEL_CASES:
        data, canvases, c = ec.get(n)
        assert c.fallback == any(em.colours_of(f) > 256 for f in canvases), n
        assert (em.encode_file(canvases) is None) == c.fallback
    assert [em.colours_of(f) for f in ec.get("fallback_in_the_middle")[1]] == [256, 257, 4]
    assert len(ec.get("frames_70")[1]) == 70 and ec.get("frames_70")[1].shape[1:3] == (20, 20)
    bits = [em.palette_of(f)[1] for f in ec.get("tables_of_different_sizes")[1]]
    assert len(set(bits)) >= 4
    assert {ec.get(n)[2].query for n in ec.CASES} >= {"inverse=true", "grayscale=true"}
    first = ec.get("transparent_partial_first_frame")[1][0]
    assert (first[..., 3] == 0).any() and (first[..., 3] != 0).any()           # the first frame does not cover the canvas


def _segments(name, frame=0):
    table, bits, idx, transparent = em.palette_of(ec.get(name)[1][frame])
    return em.frame_segments(idx, max(2, bits)), max(2, bits)


def test_the_lzw_cases_are_what_their_names_say():
    segs, mcs = _segments("noise_256_colours_three_segments")
    assert len(segs) == 3 and mcs == 8
    for codes, _ in segs[:2]:
        assert {w for _, w in codes} == {9, 10, 11, 12}                        # every width inside one segment
    segs, mcs = _segments("noise_4_colours_code_size_2")
    assert mcs == 2 and segs[0][0][0] == (4, 3)                                # the leading clear code at 3 bits
    segs, mcs = _segments("constant_frame")
    assert len(segs) == 4 and all(len(codes) <= 66 for codes, _ in segs)       # match k is k indices long: 64 codes take 2,048 of them
    # closing codes: a clear code and the end code, each once widened and once not
    for name, last, wide in (("clear_code_wide", False, True), ("clear_code_plain", False, False), ("end_code_wide", True, True), ("end_code_plain", True, False)):
        segs, mcs = _segments(name)
        codes, bumped = segs[-1] if last else segs[0]
        assert len(segs) == (1 if last else 2) and bumped == wide, name
        assert codes[-1][0] == (1 << mcs) + (1 if last else 0) and codes[-1][1] - codes[-2][1] == (1 if wide else 0), name
    for name, want in (("data_255", 255), ("data_256", 256), ("data_510", 510), ("data_511", 511)):
        table, bits, idx, transparent = em.palette_of(ec.get(name)[1][0])
        assert len(em.frame_data(idx, max(2, bits))) == want, name


def test_one_segment_is_the_usual_greedy_stream():
    """below S + 1 indices the model's data is what tests/gif_write.py's single-stream encoder writes (the decode tests' witness)"""
    for name in ("pixels_1", "pixels_S_minus_1", "pixels_S", "colours_1", "colours_5", "colours_256", "end_code_wide", "end_code_plain", "data_255"):
        for frame in ec.get(name)[1]:
            table, bits, idx, transparent = em.palette_of(frame)
            assert em.frame_data(idx, max(2, bits)) == gw.lzw_greedy(idx, max(2, bits)), name


# ---- the model's files against the library's own decoder, and against Pillow ------------------------------------------------------------

def check_file(fl, data, frames):
    """the model's file for `frames` decodes, by the library's host half, to the expected records, palettes and indices"""
    F, h, w = len(frames), frames[0].shape[0], frames[0].shape[1]
    info = fl.gif_info(data)
    assert (info["supported"], info["width"], info["height"], info["frames"], info["has_global_table"], info["interlaced_frames"]) == (1, w, h, F, 0, 0)
    assert info["transparent_frames"] == sum(bool((f[..., -1] == 0).any()) for f in frames)
    blob = fl.debug_gif_blob(data)
    buf = np.frombuffer(blob, np.uint8)
    for r, f in zip(gm.blob_records(blob), frames):
        table, bits, idx, transparent = em.palette_of(f)
        assert (r["x"], r["y"], r["w"], r["h"], r["disposal"], r["interlaced"]) == (0, 0, w, h, 1, 0)
        assert np.array_equal(buf[r["idx_off"]:r["idx_off"] + w * h], idx)
        pal = buf[r["pal_off"]:r["pal_off"] + 1024].reshape(256, 4)
        assert np.array_equal(pal, gm.palette_of(table, transparent))
    assert len(data) <= em.max_file_bytes(F, w * h, frames[0].shape[-1])


@pytest.mark.parametrize("name", ENCODED)
def test_model_files_decode_to_the_frames(fl, name):
    data, canvases, c = ec.get(name)
    check_file(fl, em.encode_file(canvases), canvases)


@pytest.mark.parametrize("name", ["transparent_partial_first_frame", "colours_17", "pixels_S_plus_1", "frames_70"])
def test_model_files_of_two_channel_frames(fl, name):
    frames = luma_alpha(ec.get(name)[1])
    data = em.encode_file(frames)
    check_file(fl, data, frames)
    # l, l, l, a: the same file as the four-channel frames of LumaA8::to_rgba8
    assert data == em.encode_file(np.concatenate([frames[..., :1]] * 3 + [frames[..., 1:]], -1))


OPAQUE = [n for n in ENCODED if (ec.get(n)[1][..., 3] == 255).all()]


def test_the_opaque_cases_are_many():
    assert len(OPAQUE) >= 25 and {"noise_256_colours_three_segments", "constant_frame", "clear_code_wide", "end_code_wide", "data_255", "frames_70"} <= set(OPAQUE)


@pytest.mark.parametrize("name", OPAQUE)
def test_pillow_decodes_the_model_files(name):
    """a second witness, on opaque frames only: there a viewer's composition of disposal 1 cannot differ from the frame itself"""
    from PIL import Image, ImageSequence
    data, canvases, c = ec.get(name)
    im = Image.open(io.BytesIO(em.encode_file(canvases)))
    got = np.stack([np.asarray(f.convert("RGBA")) for f in ImageSequence.Iterator(im)])
    assert got.shape == canvases.shape and np.array_equal(got, canvases)
    assert im.info.get("loop") == 0


def test_the_transparent_index_is_that_of_the_last_clear_pixel():
    f = np.full((2, 3, 4), 255, np.uint8)
    f[0, 0] = (9, 9, 9, 0)
    f[1, 1] = (1, 2, 3, 0)          # the last pixel with alpha 0: (1, 2, 3, 0) is the transparent colour, (9, 9, 9, 0) stays a colour of its own
    f[0, 2] = (1, 2, 3, 7)          # alpha != 0 becomes 255
    table, bits, idx, transparent = em.palette_of(f)
    assert em.colours_of(f) == 4 and bits == 2 and transparent == 0
    assert idx.tolist() == [2, 3, 1, 3, 0, 3] and table[:3].tolist() == [[1, 2, 3], [1, 2, 3], [9, 9, 9]]
    body = em.encode_frame(f)
    assert body[:8] == b"\x21\xf9\x04\x05\x00\x00\x00\x00" and body[8:18] == b"\x2c\x00\x00\x00\x00\x03\x00\x02\x00\x81"
    opaque = em.encode_frame(np.full((2, 3, 4), 255, np.uint8))
    assert opaque[:8] == b"\x21\xf9\x04\x04\x00\x00\x00\x00" and opaque[17] == 0x80 and opaque[18 + 6] == 2
