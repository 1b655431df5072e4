"""Lossy WebP sources decoded by the library (FLGPU_IMG_VP8_SOURCE): the boolean coder on the calling thread
(tests/test_vp8_source_host.py), dequantisation, inverse transforms, intra prediction, loop filter, ALPH filters, up-sampling and
YUV -> RGB on the device (csrc/fl_vp8dec.hip).  The arbiter is libwebp -- WebPDecodeYUV for the planes, WebPDecodeRGB / RGBA for the
pixels -- and, for the files of tests/vp8_model.py, the model's own reconstruction; the decode is bit-exact, so every request on a
file is held to equality with the same request on the decoded pixels.  How lanes, waves, rounds and bands share a picture is
in the .hip file alone, out of the host twin's reach: the corpus holds the sizes around every such seam (cases.SCHEDULING;
tests/test_vp8_source_host.py asserts that it does), and they are decoded here."""
import io
import threading

import numpy as np
import pytest

import vp8_model
import vp8_src_cases as cases
import vp8l_model
import webp_cases as wc

pytestmark = pytest.mark.gpu

needs_libwebp = pytest.mark.skipif(not cases.have_libwebp(), reason="libwebp cannot be loaded")
CASES = [pytest.param(n, marks=needs_libwebp) if n in cases.LIBWEBP else n for n in cases.names()]


# ---- decode parity ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_decode_is_bit_exact(gpu_state, fl, name):
    c = cases.get(name)
    info = fl.vp8_info(c["data"])
    # the planes first, without and with the loop filter: a failure names its stage
    before, after = gpu_state.debug_vp8_planes(c["data"], False), gpu_state.debug_vp8_planes(c["data"], True)
    for k, plane in enumerate("YUV"):
        if info["filter_level"] == 0:
            assert np.array_equal(before[k], c["yuv"][k]), f"{plane} plane differs after reconstruction"
        assert np.array_equal(after[k], c["yuv"][k]), f"{plane} plane differs" + (" behind the loop filter" if np.array_equal(before[k], after[k]) is False else "")
    got = gpu_state.decode_webp_lossy(c["data"])
    assert got.shape == (info["height"], info["width"], c["channels"])
    if c["pixels"] is not None:
        assert np.array_equal(got, c["pixels"]), "pixels differ from WebPDecodeRGB / WebPDecodeRGBA"
    if c["channels"] == 4 and name in cases.MODEL:
        assert np.array_equal(got[..., 3], c["alpha"])


# ---- the pixel pipeline behind the decoder ---------------------------------------------------------------------------------------------------

def same(p, q):
    """payloads of process_image: pixels, or the planes for a host WebP encoder"""
    return np.array_equal(p, q) if isinstance(p, np.ndarray) else all(np.array_equal(getattr(p, n), getattr(q, n)) for n in "yuva")


def request_file(orientation=None, alpha=False):
    c = cases.get("model_alpha_filter3" if alpha else "model_48x32")
    return (c["data"] if orientation is None else cases.extended(c["data"], orientation)), c


@pytest.mark.parametrize("kw", [dict(), dict(crop=True), dict(grayscale=True), dict(blur_sigma=2.0)], ids=["resize", "crop", "grayscale", "blur"])
@pytest.mark.parametrize("alpha", [False, True])
def test_a_request_on_the_file_equals_the_request_on_the_decoded_pixels(gpu_state, fl, kw, alpha):
    data, _ = request_file(alpha=alpha)
    pixels = gpu_state.decode_webp_lossy(data)
    p = fl.make_params(30, 20, **kw)
    assert np.array_equal(gpu_state.process_vp8_pixels(data, p), gpu_state.process_pixels(pixels, p))


@pytest.mark.parametrize("query", ["w=30&h=20", "w=30&h=20&crop=true", "w=30&h=20&grayscale=true", "w=30&h=20&blur=2"])
def test_process_webp_on_a_lossy_file_equals_process_image_on_the_decoded_pixels(gpu_state, fl, query):
    data, _ = request_file()
    pixels = gpu_state.decode_webp_lossy(data)
    for q, content in ((query, None), (query + "&webp=true", fl.Format(fl.ACCEPT_WEBP))):
        a, b = gpu_state.process_webp(data, q, content), gpu_state.process_image(pixels, q, content, input_format=fl.IN_WEBP)
        assert a[:2] == b[:2] and a[0] == "image/webp" and same(a[2], b[2])


@pytest.mark.parametrize("orientation", range(1, 9))
def test_process_webp_honours_the_exif_orientation_of_a_lossy_file(gpu_state, fl, orientation):
    data, c = request_file(orientation)
    assert fl.vp8_info(data)["exif_orientation"] == orientation
    pixels = gpu_state.decode_webp_lossy(c["data"])
    assert np.array_equal(gpu_state.decode_webp_lossy(data), pixels)   # flgpu_decode_webp_lossy applies none
    a = gpu_state.process_webp(data, "w=30&h=20")
    b = gpu_state.process_image(pixels, "w=30&h=20", None, input_format=fl.IN_WEBP, orientation=orientation)
    c = gpu_state.process_image(pixels, "w=30&h=20", None, input_format=fl.IN_WEBP, orientation=1)
    assert a[:2] == b[:2] and same(a[2], b[2])
    assert orientation == 1 or not same(a[2], c[2])   # (the orientation changes this picture)


def test_process_webp_as_is_and_size_gate(gpu_state, fl):
    data, _ = request_file()
    assert gpu_state.process_webp(data, "") == ("image/webp", fl.RESULT_AS_IS, data)   # input format WebP: an empty query is as_is
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_webp(data, "w=2001&h=1001")
    assert e.value.status == fl.ERR_PARSE
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_webp(data[:40], "w=30&h=20")
    assert e.value.status == fl.ERR_PARSE


# ---- batches, the queue, shards, counters ---------------------------------------------------------------------------------------------------

def jpeg_file(seed, w=48, h=40):
    from PIL import Image
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 5 + seed) % 256, (y * 6) % 256, ((x + y) * 3) % 256], axis=2).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def png_file():
    import png_write as pw
    s = wc.rng(300).integers(0, 256, (30, 40, 3))
    return pw.write_png(s, 2, filters=wc.rng(301).integers(0, 5, 30).tolist())


LOSSY_IN_BATCH = ["model_48x32", "model_alpha_filter2", "model_partitions8", "model_17x33"] + (
    ["lib_default", "lib_strength0", "lib_skips_bpred", "lib_alpha_raw", "lib_alpha_compressed", "lib_alpha_compressed_filtered", "lib_336x48"] if cases.have_libwebp() else [])


def mixed_requests(fl):
    reqs = [(fl.LossyWebp(cases.get(n)["data"]), fl.make_params(20, 10) if k % 2 else fl.make_params()) for k, n in enumerate(LOSSY_IN_BATCH)]
    reqs.append((wc.get("order_PXGI")[0], fl.make_params(20, 10)))
    reqs.append((jpeg_file(1), fl.make_params(20, 10)))
    reqs.append((png_file(), fl.make_params(20, 10)))
    reqs.append((wc.rng(302).integers(0, 256, (25, 31, 3)).astype(np.uint8), fl.make_params(20, 10)))
    return reqs


def alone(st, fl, src, p):
    if isinstance(src, fl.LossyWebp):
        return st.process_vp8_pixels(bytes(src), p)
    if isinstance(src, bytes):
        return st.process_webp_pixels(src, p) if src[:4] == b"RIFF" else st.process_png_pixels(src, p) if src[:4] == b"\x89PNG" else st.process_jpeg_pixels(src, p)
    return st.process_pixels(src, p)


def test_mixed_batch_equals_each_request_alone_and_counters(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, fl, s, p) for s, p in reqs]
    lossy = [s for s, _ in reqs if isinstance(s, fl.LossyWebp)]
    before, webp_before = gpu_state.vp8_counters(), gpu_state.webp_counters()
    got = gpu_state.process_batch([s for s, _ in reqs], [p for _, p in reqs])
    after, webp_after = gpu_state.vp8_counters(), gpu_state.webp_counters()
    for k, (a, b) in enumerate(zip(got, each)):
        assert np.array_equal(a, b), k
    assert np.array_equal(got[0], gpu_state.decode_webp_lossy(bytes(lossy[0])))   # an identity request is the decoded picture itself
    assert after["vp8_sources"] - before["vp8_sources"] == len(lossy)
    assert after["vp8_file_bytes"] - before["vp8_file_bytes"] == sum(len(s) for s in lossy)
    assert after["vp8_upload_bytes"] - before["vp8_upload_bytes"] == sum(fl.vp8_info(bytes(s))["blob_bytes"] for s in lossy)
    assert webp_after["webp_sources"] - webp_before["webp_sources"] == 1   # the one lossless file: lossy ones do not move it
    with pytest.raises(fl.FanlinError):
        gpu_state.debug_set("vp8_sources", 0)


@needs_libwebp
def test_one_launch_of_pictures_five_orders_of_magnitude_apart(gpu_state, fl):
    """One launch of each kernel over jobs from 1 to 549,120 pixels: with and without a loop filter, with and without an ALPH plane, the
    plane at stride 1 and at stride 4, past a round, a chunk and a band or far short of one.  Every kernel's early return for a job
    that is not its business, and every loop bound taken from the job's own size, leaves the jobs beside it alone."""
    names = ["lib_rounds_1040x528", "model_1x1", "model_alpha_3x1030_filter3", "lib_alpha_1100x3_filter2", "lib_alpha_200x70_filter3", "model_48x32"]
    files = [cases.get(n)["data"] for n in names]
    infos = [fl.vp8_info(d) for d in files]
    assert [(i["width"], i["height"]) for i in infos] == [(1040, 528), (1, 1), (3, 1030), (1100, 3), (200, 70), (48, 32)]
    assert [(i["channels"], i["alpha_compression"], i["alpha_filter"]) for i in infos[2:5]] == [(4, 0, 3), (4, 1, 2), (4, 1, 3)]
    assert {bool(i["filter_level"]) for i in infos} == {False, True} and {i["channels"] for i in infos} == {3, 4}
    each = [gpu_state.process_vp8_pixels(d, fl.make_params()) for d in files]
    before = gpu_state.vp8_counters()["vp8_sources"]
    got = gpu_state.process_batch([fl.LossyWebp(d) for d in files], [fl.make_params()] * len(files))
    assert gpu_state.vp8_counters()["vp8_sources"] - before == len(files)
    for n, a, b in zip(names, got, each):
        assert a.shape == b.shape and np.array_equal(a, b), n
        assert np.array_equal(a, cases.get(n)["pixels"]), n   # (an identity request is the decoded picture itself)


def test_the_same_requests_through_the_queue_from_eight_threads(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, fl, s, p) for s, p in reqs]
    before = gpu_state.vp8_counters()["vp8_sources"]
    results, errors = {}, []

    def worker(t):
        try:
            for k in range(len(reqs)):
                i = (k + t) % len(reqs)
                results[(t, i)] = alone(gpu_state, fl, *reqs[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for (t, i), r in results.items():
        assert np.array_equal(r, each[i]), (t, i)
    assert gpu_state.vp8_counters()["vp8_sources"] - before == 8 * len(LOSSY_IN_BATCH)


def test_the_same_requests_on_two_shards(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, fl, s, p) for s, p in reqs]
    with fl.State(devices=[0, 0]) as two:
        got = two.process_batch([s for s, _ in reqs], [p for _, p in reqs])
        for k, (a, b) in enumerate(zip(got, each)):
            assert np.array_equal(a, b), k
        assert two.vp8_counters()["vp8_sources"] == len(LOSSY_IN_BATCH)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------

def resized(data):
    """RIFF and VP8 chunk sizes repaired after bytes were cut from the end of a simple-format file"""
    data = data + (b"\0" if len(data) & 1 else b"")
    return data[:4] + (len(data) - 8).to_bytes(4, "little") + data[8:16] + (len(data) - 20).to_bytes(4, "little") + data[20:]


def test_errors_leave_the_context_usable(gpu_state, fl):
    c = cases.get("model_48x32")
    good, pixels = c["data"], gpu_state.decode_webp_lossy(c["data"])
    tag = int.from_bytes(good[20:23], "little")
    ext = cases.extended(good)
    bad = [
        (good, (32, 48, 4), fl.ERR_INVALID_ARG),                                                    # the announced shape disagrees with the file
        (good, (48, 32, 3), fl.ERR_INVALID_ARG),
        (resized(good[:len(good) - 300]), None, fl.ERR_PARSE),                                      # the token partitions run dry
        (good[:20] + ((tag & 31) | 40 << 5).to_bytes(3, "little") + good[23:], None, fl.ERR_PARSE),  # the first partition cut short
        (ext[:20] + bytes([ext[20] | 2]) + ext[21:], (32, 48, 3), fl.ERR_UNSUPPORTED),              # animated
        (vp8l_model.encode(np.zeros((32, 48, 4), np.uint8)), (32, 48, 3), fl.ERR_PARSE),            # a lossless file is no lossy one
    ]
    bad += [(cases.refused_file(f), (16, 16, 3), fl.ERR_UNSUPPORTED) for f in cases.REFUSED_FEATURES]   # the refused features, each alone
    before = gpu_state.vp8_counters()["vp8_sources"]
    for k, (data, shape, status) in enumerate(bad):
        with pytest.raises(fl.FanlinError) as e:   # alone ...
            gpu_state.process_vp8_pixels(data, fl.make_params(), shape=shape or (32, 48, 3))
        assert e.value.status == status, k
        if k >= len(bad) - len(cases.REFUSED_FEATURES):
            assert list(cases.REFUSED_FEATURES.values())[k - len(bad)] in str(e.value)   # the text names the refused feature
        if status != fl.ERR_INVALID_ARG:   # ... and in a batch behind a good picture (a batch announces the file's own shape)
            with pytest.raises(fl.FanlinError) as e:
                gpu_state.process_batch([pixels, fl.LossyWebp(data)], [fl.make_params()] * 2)
            assert e.value.status == status, k
        assert np.array_equal(gpu_state.decode_webp_lossy(good), pixels)   # the next request is served
    assert gpu_state.vp8_counters()["vp8_sources"] - before == len(bad)   # only the good ones were decoded


# ---- encoder and decoder check each other -----------------------------------------------------------------------------------------------------

def test_the_lossy_encoder_and_this_decoder_agree_without_libwebp(gpu_state, fl):
    """a lossy source -> w=300&h=200&webp=true with the opt-in encoder -> a file this decoder reads back to the encoder's own
    reconstruction (tests/vp8_model.py restates the encoder)"""
    src = cases.get("model_partitions8")["data"]
    accept = fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY)
    mime, kind, body = gpu_state.process_webp(src, "w=300&h=200&webp=true", accept)
    assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body[:4] == b"RIFF"
    pl = gpu_state.process_vp8_pixels(src, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP420))
    want, rec, _ = vp8_model.encode(pl.y, pl.u, pl.v, 75, pl.a if pl.has_alpha else None)
    assert body == want
    info = fl.vp8_info(body)
    assert (info["width"], info["height"], info["supported"], info["partitions"]) == (300, 200, 1, 8)
    for got, plane in zip(gpu_state.debug_vp8_planes(body), rec):
        assert np.array_equal(got, plane)
    if cases.have_libwebp():
        import vp8_dec_lib
        assert np.array_equal(gpu_state.decode_webp_lossy(body), vp8_dec_lib.decode_pixels(body, 3))
