"""File bytes + query string + accept flags -> a planned request: what flgpu_process_{jpeg,png,webp,gif}[_plan] decide before anything is
decoded, the same for every format -- and the one place where JPEG differs.  The statuses are those of the per-format planners this one path
replaced (written down from a dump of their verdicts, not from the code that is tested here).

CPU part: the verdict order on the smallest file of each format, on a file its decoder refuses and on a damaged one, and the plan against
flgpu_process_image_plan on the announced geometry.  GPU part (-m gpu): process_X(file) against process_image(decode_X(file)) at 48 x 32."""
import ctypes as C

import numpy as np
import pytest

import gif_cases
import gif_write as gw
import png_adam7_write
import png_write
import synth
import vp8_src_cases
import vp8l_write as vw
import webp_cases as wc

FORMATS = ("jpeg", "png", "webp", "vp8", "gif")
ORIENTATION = {"jpeg": 6, "png": 1, "webp": 5, "vp8": 7, "gif": 1}   # the EXIF tag the intact files carry (PNG and GIF have none: 1)
POISON = 0xA5


def jpeg_file(oracle, h, w, orientation=None):
    """a baseline JPEG from the oracle's encoder, with an EXIF APP1 segment behind SOI where an orientation is asked for"""
    data = oracle.jpeg_encode(synth.photo(h, w, 3, index=h + w), 85)
    if orientation:
        app1 = vw.exif(orientation, prefix=True)
        data = data[:2] + b"\xff\xe1" + (len(app1) + 2).to_bytes(2, "big") + app1 + data[2:]
    return data


def gif_file(h, w):
    rng = gif_cases.rng_of("file_requests")
    frames = [gw.Frame(0, 0, gif_cases.noise(rng, h, w, 16)), gw.Frame(w // 8, h // 8, gif_cases.noise(rng, h // 2, w // 2, 16), disposal=1, transparent=2)]
    return gw.write_gif(w, h, frames, gif_cases.table(rng, 16))


def intact(fmt, oracle, h, w):
    """(file, announced (width, height, channels)): h x w, with ORIENTATION[fmt] in its EXIF data where the format has any"""
    if fmt == "jpeg":
        return jpeg_file(oracle, h, w, ORIENTATION[fmt]), (w, h, 3)
    if fmt == "png":
        return png_write.write_png(synth.photo(h, w, 3, index=3), 2, filters=[y % 5 for y in range(h)]), (w, h, 3)
    if fmt == "webp":
        return vw.write(wc.noise(h, w, 7), extended=dict(alpha=True, after=[(b"EXIF", vw.exif(ORIENTATION[fmt]))])), (w, h, 4)
    if fmt == "vp8":
        assert (w, h) in ((16, 16), (48, 32))
        return vp8_src_cases.extended(vp8_src_cases.get(f"model_{w}x{h}")["data"], ORIENTATION[fmt]), (w, h, 3)
    return gif_file(h, w), (w, h, 4)


def refused(fmt, oracle):
    """a well-formed file of the format that its device decoder does not take"""
    if fmt == "jpeg":   # SOF9: arithmetic coding
        data = bytearray(jpeg_file(oracle, 16, 24))
        data[data.find(b"\xff\xc0") + 1] = 0xC9
        return bytes(data)
    if fmt == "png":    # Adam7, asked for without DECODE_PNG_ADAM7
        return png_adam7_write.write_png(synth.photo(9, 13, 3, index=2), 2)
    if fmt == "webp":   # the VP8X animation flag
        return vw.write(wc.noise(4, 4, 1), extended=dict(alpha=True, flags=0x02))
    if fmt == "vp8":    # a frame header feature the decoder refuses
        return vp8_src_cases.refused_file("clamp")
    return gif_cases.unsupported_cases()["frame_beyond_right_edge"]


def plan_call(fl, fmt, data, query, flags=0, plan=True, kind=True):
    """(status, result kind, plan) of flgpu_process_<fmt>_plan; the outputs start out poisoned, so what a verdict leaves untouched shows"""
    lib = fl.load_library()
    p, k, frames = fl.flgpu_plan(), C.c_int(-77), C.c_uint32()
    C.memset(C.byref(p), POISON, C.sizeof(p))
    pp, kp, n = C.byref(p) if plan else None, C.byref(k) if kind else None, len(data) if data is not None else 0
    if fmt == "gif":
        st = lib.flgpu_process_gif_plan(data, n, query.encode(), flags, pp, C.byref(frames), kp)
    else:
        st = getattr(lib, "flgpu_process_%s_plan" % ("webp" if fmt == "vp8" else fmt))(data, n, query.encode(), flags, pp, kp)
    return st, k.value, p


def plan_fields(p):
    return tuple(getattr(p, n) for n, _ in p._fields_)


UNTOUCHED = tuple(int.from_bytes(bytes([POISON]) * C.sizeof(t), "little") for t in (C.c_uint32,) * 18 + (C.c_uint64,) * 3)


@pytest.fixture(scope="module")
def files(oracle):
    return {fmt: dict(intact=intact(fmt, oracle, 16, 16), refused=refused(fmt, oracle)) for fmt in FORMATS}


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_damaged_file_is_a_parse_error_whatever_the_query(fl, files, fmt):
    data = files[fmt]["intact"][0]
    for cut in (data[:7], b""):
        for query in ("", "w=300&h=200", "w=oops"):
            assert plan_call(fl, fmt, cut, query)[0] == fl.ERR_PARSE, (len(cut), query)
    assert plan_call(fl, fmt, None, "")[0] == fl.ERR_INVALID_ARG


@pytest.mark.parametrize("which", ("intact", "refused"))
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_query_and_the_size_gate_come_before_the_file_s_support(fl, files, fmt, which):
    data = files[fmt][which]
    data = data[0] if which == "intact" else data
    for query in ("w=oops", "w=9999&h=9999", "w=19&h=20", "h=1001", "webp=true&webp=true"):   # (one side alone: the other defaults to 100)
        st, kind, plan = plan_call(fl, fmt, data, query)
        assert st == fl.ERR_PARSE and kind == -77 and plan_fields(plan) == UNTOUCHED, query


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_refused_file_is_served_as_is_and_nothing_else(fl, files, fmt):
    data = files[fmt]["refused"]
    for query in ("", "rgb=1,2,3", "quality=50&crop=true"):            # as_is: nothing is decoded, the plan is zeroed
        st, kind, plan = plan_call(fl, fmt, data, query, flags=fl.ACCEPT_WEBP | fl.ACCEPT_AVIF)
        assert (st, kind) == (fl.OK, fl.RESULT_AS_IS) and not any(plan_fields(plan)), query
    for query in ("w=300&h=200", "webp=true", "blur=10", "grayscale=true"):
        st, kind, plan = plan_call(fl, fmt, data, query, flags=fl.ACCEPT_WEBP)
        assert st == fl.ERR_UNSUPPORTED, query
        if fmt != "jpeg":
            assert kind == -77 and plan_fields(plan) == UNTOUCHED, query


def test_a_refused_jpeg_alone_is_planned_before_it_is_refused(fl, files):
    """JPEG goes through the planner first and is refused behind it: the plan and the kind are filled beside ERR_UNSUPPORTED, and what the
    planner itself objects to -- null outputs -- wins over the refusal.  PNG / WebP / GIF are refused in front of the planner, behind the
    query's own verdict."""
    st, kind, plan = plan_call(fl, "jpeg", files["jpeg"]["refused"], "w=300&h=200")
    assert (st, kind) == (fl.ERR_UNSUPPORTED, fl.RESULT_JPEG_STREAM)
    assert (plan.src_w, plan.src_h, plan.mid_c, plan.out_w, plan.out_h, plan.out_c, plan.letterboxed) == (24, 16, 3, 300, 200, 3, 0)   # (24 x 16 fills 300 x 200)
    for fmt in FORMATS:
        for query, others in (("w=300&h=200", fl.ERR_UNSUPPORTED), ("w=oops", fl.ERR_PARSE), ("", fl.ERR_INVALID_ARG)):
            want = fl.ERR_INVALID_ARG if fmt == "jpeg" else others
            assert plan_call(fl, fmt, files[fmt]["refused"], query, plan=False)[0] == want, (fmt, query)
            assert plan_call(fl, fmt, files[fmt]["refused"], query, kind=False)[0] == want, (fmt, query)


def test_adam7_is_taken_with_the_flag_and_refused_without(fl, files):
    data = files["png"]["refused"]
    assert plan_call(fl, "png", data, "w=300&h=200")[0] == fl.ERR_UNSUPPORTED
    st, kind, plan = plan_call(fl, "png", data, "w=300&h=200", flags=fl.DECODE_PNG_ADAM7)
    assert (st, kind, plan.src_w, plan.src_h, plan.mid_c) == (fl.OK, fl.RESULT_PIXELS, 13, 9, 3)


QUERIES = ("w=300&h=200", "w=40&h=30&crop=true", "w=24&h=24&webp=true", "w=24&h=24&webp=true&quality=100", "w=24&h=24&avif=true", "grayscale=true", "blur=12&w=20&h=20")


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_plan_is_process_image_s_on_the_announced_geometry(fl, files, fmt):
    """... with that format's FLGPU_IN_* and the file's EXIF orientation (1 where it has none, and for PNG and GIF)"""
    lib = fl.load_library()
    data, (w, h, c) = files[fmt]["intact"]
    input_format = {"jpeg": fl.IN_JPEG, "png": fl.IN_PNG, "webp": fl.IN_WEBP, "vp8": fl.IN_WEBP, "gif": fl.IN_GIF_FRAME}[fmt]
    announced = fl.flgpu_image(None, 0, w, h, c, 0)
    seen = set()
    for flags in (0, fl.ACCEPT_WEBP | fl.ACCEPT_AVIF, fl.ACCEPT_WEBP | fl.ENCODE_PNG | fl.ENCODE_WEBP_LOSSLESS | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4):
        for query in QUERIES:
            st, kind, plan = plan_call(fl, fmt, data, query, flags)
            want, want_kind = fl.flgpu_plan(), C.c_int(-77)
            want_st = lib.flgpu_process_image_plan(C.byref(announced), ORIENTATION[fmt], query.encode(), flags, input_format, C.byref(want), C.byref(want_kind))
            assert (st, kind, plan_fields(plan)) == (want_st, want_kind.value, plan_fields(want)) and st == fl.OK, (query, flags)
            seen.add(kind)
    assert len(seen) >= (1 if fmt == "gif" else 2), seen


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_exif_orientation_reaches_the_plan(fl, oracle, fmt):
    data, (w, h, c) = intact(fmt, oracle, 32, 48)
    plan = plan_call(fl, fmt, data, "grayscale=true")[2]
    assert (plan.src_w, plan.src_h) == ((h, w) if ORIENTATION[fmt] >= 5 else (w, h))


# ---- on the device: the file request against decode + process_image ------------------------------------------------------------------

def same_payload(a, b):
    if isinstance(a, bytes) or a is None:
        return type(a) is type(b) and a == b
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same_payload(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    return type(a) is type(b) and a.has_alpha == b.has_alpha and all(same_payload(getattr(a, n), getattr(b, n)) for n in "yuva")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_process_file_is_decode_then_process_image(fl, gpu_state, oracle, fmt):
    st = gpu_state
    data, (w, h, c) = intact(fmt, oracle, 32, 48)
    process, decode, input_format = {"jpeg": (st.process_jpeg, st.decode_jpeg, fl.IN_JPEG), "png": (st.process_png, st.decode_png, fl.IN_PNG),
                                     "webp": (st.process_webp, st.decode_webp, fl.IN_WEBP), "vp8": (st.process_webp, st.decode_webp_lossy, fl.IN_WEBP),
                                     "gif": (st.process_gif, st.decode_gif, fl.IN_GIF_FRAME)}[fmt]
    content = fl.Format.from_accept_header("image/webp")
    pixels = decode(data)
    assert pixels.shape == ((2, h, w, c) if fmt == "gif" else (h, w, c))
    # half the size, as w=24&h=16 asks -- which the size gate (20..2000 x 20..1000, main.rs:134-138) answers with ERR_PARSE on both paths alike;
    # h=20 is the nearest request that gets through (letterboxed), alone and on the lossless WebP arm
    for query in ("w=24&h=16", "w=24&h=20", "w=24&h=20&webp=true&quality=100"):
        frames = pixels if fmt == "gif" else [pixels]   # every frame of a GIF is a request of its own; the file's result is the list of theirs
        try:
            mime, kind, payload = process(data, query, content)
        except fl.FanlinError as e:
            for frame in frames:
                with pytest.raises(fl.FanlinError) as other:
                    st.process_image(frame, query, content, input_format, ORIENTATION[fmt])
                assert other.value.status == e.status == fl.ERR_PARSE and query == "w=24&h=16"
            continue
        each = [st.process_image(frame, query, content, input_format, ORIENTATION[fmt]) for frame in frames]
        assert all(e[:2] == (mime, kind) for e in each) and kind != fl.RESULT_AS_IS and query != "w=24&h=16", query
        assert same_payload(payload, [e[2] for e in each] if fmt == "gif" else each[0][2]), query


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_as_is_hands_back_what_each_format_does(fl, gpu_state, oracle, fmt):
    data, _ = intact(fmt, oracle, 32, 48)
    process = {"jpeg": gpu_state.process_jpeg, "png": gpu_state.process_png, "webp": gpu_state.process_webp, "vp8": gpu_state.process_webp, "gif": gpu_state.process_gif}[fmt]
    mime = {"jpeg": "image/jpeg", "png": "image/png", "webp": "image/webp", "vp8": "image/webp", "gif": "image/gif"}[fmt]
    assert process(data, "") == (mime, fl.RESULT_AS_IS, None if fmt == "jpeg" else data)   # a JPEG gives None, as process_image does; the others the file
