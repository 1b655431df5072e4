"""PNG sources whose deflate stream the device inflates (FLGPU_IMG_PNG_INFLATE, FLGPU_DECODE_PNG_INFLATE; csrc/fl_inflate.hip): the
kernel's scanlines against zlib.decompress on the host test's corpus, decoded pixels against construction, full requests and batches
against the same requests without the bit, the counters, and broken streams, which end as they end without the bit."""
import ctypes as C
import io
import threading
import zlib

import numpy as np
import pytest

import png_inflate_cases as pc
import png_write as pw

pytestmark = pytest.mark.gpu


def counters(st):
    return {k: st.debug_get(k) for k in ("png_sources", "png_file_bytes", "png_upload_bytes", "png_device_inflates", "png_inflate_retries")}


def delta(st, before):
    return {k: v - before[k] for k, v in counters(st).items()}


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(pc.valid())), ids=[c[0] for c in pc.valid()])
def test_device_scanlines_equal_zlib(gpu_state, k):
    name, data, raw = pc.valid()[k]
    got = gpu_state.debug_png_inflate_device(data)
    if got != raw:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(raw, np.uint8)
        bad = np.flatnonzero(a != b) if a.size == b.size else []
        raise AssertionError(f"{name}: {len(got)} bytes against {len(raw)}; {len(bad)} differ, first at {bad[0] if len(bad) else None}")


def test_every_valid_file_is_inflated_on_the_device_and_none_is_retried(gpu_state, fl):
    """A condition, not a measurement: the fixed-point rule settles every valid stream, so no valid file ever goes back to the host."""
    before = counters(gpu_state)
    upload = 0
    for name, data, raw in pc.valid():
        got = gpu_state.decode_png(data, device_inflate=True)
        assert got.shape == (1, len(raw) - 1, 1) and got.tobytes() == raw[1:], name      # (one row, filter type 0: the pixels are the bytes)
        upload += pc.HEADER_BYTES + len(pw.idat_payload(data)) + pc.PAD
    d = delta(gpu_state, before)
    n = len(pc.valid())
    assert d["png_device_inflates"] == n and d["png_inflate_retries"] == 0 and d["png_sources"] == n, d
    assert d["png_upload_bytes"] == upload and d["png_file_bytes"] == sum(len(c[1]) for c in pc.valid()), d


# ---- pixels ------------------------------------------------------------------------------------------------------------------------

COMBOS = [(ct, d, t) for ct, d in [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)]
          for t in (False, True) if not (t and ct in (4, 6))]


@pytest.mark.parametrize("interlace", [0, 1])
def test_each_colour_type_depth_and_trns(gpu_state, interlace):
    before = counters(gpu_state)
    for k, (ct, depth, trns) in enumerate(COMBOS):
        data, want = pc.picture(ct, depth, 11, 5, 300 + k, trns, interlace, split=[None, 7, "empty"][k % 3])
        got = gpu_state.decode_png(data, adam7=bool(interlace), device_inflate=True)
        assert got.shape == want.shape and np.array_equal(got, want), (ct, depth, trns, interlace)
        assert np.array_equal(got, gpu_state.decode_png(data, adam7=bool(interlace)))
    d = delta(gpu_state, before)
    assert d["png_device_inflates"] == len(COMBOS) and d["png_inflate_retries"] == 0, d


def test_a_picture_of_several_strips_and_blocks(gpu_state):
    data, want = pc.picture(2, 8, 256, 64, 77, level=9)        # noise: 48 KiB of literals, several strips
    assert np.array_equal(gpu_state.decode_png(data, device_inflate=True), want)
    y, x = np.mgrid[0:64, 0:256]
    s = np.stack([(x * 2 + y) % 256, (y * 4) % 256, (x * y) % 256], axis=2)
    data = pw.write_png(s, 2, filters=[4] * 64)
    assert np.array_equal(gpu_state.decode_png(data, device_inflate=True), s.astype(np.uint8))


# ---- full requests, batches, the queue -------------------------------------------------------------------------------------------------

def request_file():
    y, x = np.mgrid[0:64, 0:96]
    s = np.stack([(x * 2 + y) % 256, (y * 4) % 256, (x * y) % 256], axis=2)
    return pw.write_png(s, 2, filters=np.random.default_rng(100).integers(0, 5, 64).tolist())


@pytest.mark.parametrize("encode_png", [False, True])
def test_full_requests_equal_the_same_request_without_the_bit(gpu_state, fl, encode_png):
    data = request_file()
    enc = fl.ENCODE_PNG if encode_png else 0
    before = counters(gpu_state)
    a = gpu_state.process_png(data, "w=30&h=20", fl.Format(enc | fl.DECODE_PNG_INFLATE))
    assert delta(gpu_state, before)["png_device_inflates"] == 1
    b = gpu_state.process_png(data, "w=30&h=20", fl.Format(enc))
    assert a[:2] == b[:2] == ("image/png", fl.RESULT_PNG_STREAM if encode_png else fl.RESULT_PIXELS)
    assert (a[2] == b[2]) if encode_png else np.array_equal(a[2], b[2])
    # as_is never reads the file, with or without the bit
    before = counters(gpu_state)
    assert gpu_state.process_png(data, "quality=80", fl.Format(fl.DECODE_PNG_INFLATE)) == ("image/png", fl.RESULT_AS_IS, data)
    assert delta(gpu_state, before)["png_sources"] == 0


def jpeg_file(seed, w=48, h=40):
    from PIL import Image
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 5 + seed) % 256, (y * 6) % 256, ((x + y) * 3) % 256], axis=2).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def mixed_requests(fl):
    """[(source for process_batch, the same source without the bit, params)]"""
    reqs = []
    for k, (ct, d, w, h, trns, il) in enumerate([(2, 8, 40, 30, False, 0), (3, 4, 33, 70, True, 1), (0, 1, 19, 9, False, 0), (6, 8, 65, 66, False, 1)]):
        data, _ = pc.picture(ct, d, w, h, 400 + k, trns, il)
        p = fl.make_params(20, 10) if k % 2 else fl.make_params()
        reqs.append((fl.InflatePng(data, adam7=bool(il)), fl.Adam7Png(data) if il else data, p))
    plain, _ = pc.picture(2, 8, 50, 20, 410)
    reqs.append((plain, plain, fl.make_params(20, 10)))
    reqs.append((jpeg_file(1), jpeg_file(1), fl.make_params(20, 10)))
    px = np.random.default_rng(99).integers(0, 256, (25, 31, 3)).astype(np.uint8)
    reqs.append((px, px, fl.make_params(20, 10)))
    return reqs


def test_mixed_batch_equals_each_request_alone(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [gpu_state.process_batch([plain], [p])[0] for _, plain, p in reqs]
    before = counters(gpu_state)
    got = gpu_state.process_batch([s for s, _, _ in reqs], [p for _, _, p in reqs])
    d = delta(gpu_state, before)
    for k, (a, b) in enumerate(zip(got, each)):
        assert np.array_equal(a, b), k
    assert d["png_sources"] == 5 and d["png_device_inflates"] == 4 and d["png_inflate_retries"] == 0, d


def test_the_queue_from_eight_threads(gpu_state, fl):
    files = [pc.picture(ct, d, w, h, 500 + k, False, il) for k, (ct, d, w, h, il) in enumerate([(2, 8, 40, 30, 0), (3, 4, 33, 70, 1), (0, 8, 19, 9, 0), (6, 8, 65, 66, 1)])]
    before = counters(gpu_state)
    results, errors = {}, []

    def worker(t):
        try:
            for k in range(len(files)):
                i = (k + t) % len(files)
                results[(t, i)] = gpu_state.decode_png(files[i][0], adam7=True, device_inflate=True)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for (t, i), r in results.items():
        assert np.array_equal(r, files[i][1]), (t, i)
    d = delta(gpu_state, before)
    assert d["png_device_inflates"] == 8 * len(files) and d["png_inflate_retries"] == 0, d


# ---- what the device says no to ------------------------------------------------------------------------------------------------------

def status_of(fl, fn):
    try:
        fn()
    except fl.FanlinError as e:
        return e.status, str(e)
    return 0, ""


@pytest.mark.parametrize("k", range(len(pc.broken())), ids=[c[0] for c in pc.broken()])
def test_broken_streams_end_as_they_end_without_the_bit(gpu_state, fl, k):
    name, data = pc.broken()[k]
    good, want = pc.picture(2, 8, 23, 9, 600)
    plain = status_of(fl, lambda: gpu_state.decode_png(data))
    assert plain[0] in (fl.ERR_PARSE, fl.ERR_UNSUPPORTED), plain
    before = counters(gpu_state)
    assert status_of(fl, lambda: gpu_state.decode_png(data, device_inflate=True)) == plain, name           # status and text
    d = delta(gpu_state, before)
    assert d["png_inflate_retries"] == 1 and d["png_device_inflates"] == 0, d
    before = counters(gpu_state)
    assert status_of(fl, lambda: gpu_state.process_batch([fl.InflatePng(data)], [fl.make_params()]))[0] == plain[0], name  # the batch entry point
    assert delta(gpu_state, before)["png_inflate_retries"] == 1
    with pytest.raises(fl.FanlinError) as e:                                                                # the kernel alone: no host re-run
        gpu_state.debug_png_inflate_device(data)
    assert e.value.status == fl.ERR_PARSE
    assert np.array_equal(gpu_state.decode_png(good, device_inflate=True), want)                           # the next request is served
    # a valid picture beside a broken one in one batch: the batch fails as it fails without the bit
    assert status_of(fl, lambda: gpu_state.process_batch([fl.InflatePng(good), fl.InflatePng(data)], [fl.make_params()] * 2))[0] == plain[0]


def test_the_bit_without_a_png_source_is_an_invalid_argument(gpu_state, fl):
    px = np.zeros((4, 4, 3), np.uint8)
    out = np.zeros(4 * 4 * 3, np.uint8)
    p = fl.make_params()
    for flags in (fl.IMG_PNG_INFLATE, fl.IMG_PNG_INFLATE | fl.IMG_PNG_ADAM7):
        src = fl.flgpu_image(px.ctypes.data, px.nbytes, 4, 4, 3, flags)
        dst = fl.flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
        assert gpu_state._lib.flgpu_transform(gpu_state._ctx, C.byref(src), C.byref(p), C.byref(dst)) == fl.ERR_INVALID_ARG
        assert gpu_state._lib.flgpu_transform_batch(gpu_state._ctx, 1, C.byref(src), C.byref(p), C.byref(dst)) == fl.ERR_INVALID_ARG
    src = fl.flgpu_image(px.ctypes.data, px.nbytes, 4, 4, 3, fl.IMG_PNG_INFLATE)
    dst = fl.flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
    gpu_state._lib.flgpu_transform(gpu_state._ctx, C.byref(src), C.byref(p), C.byref(dst))
    gpu_state._lib.flgpu_last_error.restype = C.c_char_p
    assert b"FLGPU_IMG_PNG_INFLATE without FLGPU_IMG_PNG_SOURCE" in gpu_state._lib.flgpu_last_error(gpu_state._ctx)
