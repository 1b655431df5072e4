"""PNG sources decoded by the library (FLGPU_IMG_PNG_SOURCE): inflate on the calling thread (tests/test_png_source_host.py), the row
filters undone and palette / sub-byte / tRNS pictures expanded on the device (csrc/fl_pngdec.hip).  The result is determined by the
PNG specification, so every comparison is bit-exact, and the expected pixels come from construction (tests/png_write.py: the
samples a file was written from), not from a decoder."""
import io
import os
import re
import threading
import zlib

import numpy as np
import pytest

import png_write as pw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    text = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_pngdec.h")).read()
    return {k: int(v) for k, v in re.findall(r"(kPd(?:Waves|BandRows|Chunk|Lag)) = (\d+)", text)}


K = kernel_constants()
WAVES, BAND, CHUNK, LAG = K["kPdWaves"], K["kPdBandRows"], K["kPdChunk"], K["kPdLag"]
HEADER_BYTES = 16 * 4 + 256 * 4   # csrc/fl_pngsrc.h PngBlobHeader: what crosses PCIe in front of the scanlines


def rng(seed):
    return np.random.default_rng(seed)


def make(ct, depth, w, h, seed, trns=False):
    """(samples, plte, trns) for a picture of that kind; with tRNS the key is a value the picture really holds."""
    r = rng(seed)
    s = r.integers(0, 1 << depth, (h, w, pw.SAMPLES[ct]))
    plte = r.integers(0, 256, (max(2, (1 << depth) - 3), 3)) if ct == 3 else None   # (three indices lie beyond PLTE: opaque black)
    t = None
    if trns:
        t = {0: [int(s[h // 2, w // 2, 0])], 2: [int(v) for v in s[h // 2, w // 2]], 3: bytes(r.integers(0, 256, max(1, (1 << depth) // 2)).astype(np.uint8))}[ct]
    return s, plte, t


def check(st, ct, depth, w, h, filters, seed=0, trns=False, **kw):
    s, plte, t = make(ct, depth, w, h, seed, trns)
    if filters == "mix":
        filters = rng(seed + 1).integers(0, 5, h).tolist()
    data = pw.write_png(s, ct, depth, filters=filters, plte=plte, trns=t, **kw)
    want = pw.expand(s, ct, depth, plte, t)
    got = st.decode_png(data)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} of {want.size} bytes differ, first at (row, column, channel) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


# ---- filters ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ct", [0, 4, 2, 6])            # bpp 1, 2, 3, 4
@pytest.mark.parametrize("filters", [0, 1, 2, 3, 4, "mix"])
def test_each_filter_type_and_a_mix(gpu_state, ct, filters):
    check(gpu_state, ct, 8, 37, 21, filters, seed=10 + ct)


@pytest.mark.parametrize("filters", [3, 4])
@pytest.mark.parametrize("ct", [0, 4, 2, 6])
def test_average_and_paeth_on_row_zero_and_on_one_pixel_width(gpu_state, ct, filters):
    check(gpu_state, ct, 8, 23, 1, filters, seed=20)     # row 0: the row above is zeros
    check(gpu_state, ct, 8, 1, 23, filters, seed=21)     # one pixel wide: the left neighbour is zero
    check(gpu_state, ct, 8, 1, 1, filters, seed=22)


COMBOS = [(ct, d, t) for ct, d in [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)]
          for t in (False, True) if not (t and ct in (4, 6))]


@pytest.mark.parametrize("ct,depth,trns", COMBOS)
def test_each_colour_type_depth_and_trns(gpu_state, fl, ct, depth, trns):
    check(gpu_state, ct, depth, 29, 13, "mix", seed=30 + ct + depth, trns=trns)


@pytest.mark.parametrize("ct", [0, 3])
@pytest.mark.parametrize("depth", [1, 2, 4])
@pytest.mark.parametrize("w", [1, 3, 11])
def test_sub_byte_widths_that_do_not_fill_the_last_byte(gpu_state, ct, depth, w):
    check(gpu_state, ct, depth, w, 7, "mix", seed=40 + w, trns=True)
    check(gpu_state, ct, depth, w, 7, "mix", seed=41 + w, trns=False)


# ---- sizes: the smallest that cross each boundary of png_unfilter_kernel -----------------------------------------------
# A wave walks its band of BAND rows in chunks of CHUNK steps (one pixel per step); band b runs on wave b % WAVES, LAG chunk steps
# behind band b - 1; a wave takes its next band after max(chunk steps of a band, LAG * WAVES) steps.

WIDTHS = [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
HEIGHTS = [1, 2, BAND - 1, BAND, BAND + 1, WAVES * BAND + 1, 2 * WAVES * BAND + 2]


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("ct", [0, 2, 6])
def test_widths_around_the_chunk(gpu_state, ct, w):
    check(gpu_state, ct, 8, w, BAND + 3, "mix", seed=50 + w)


@pytest.mark.parametrize("h", HEIGHTS)
def test_heights_around_the_band_and_the_round(gpu_state, h):
    check(gpu_state, 2, 8, 3, h, "mix", seed=60 + h)     # (the largest at width 3 to keep it fast)
    check(gpu_state, 0, 8, 3, h, 4, seed=61 + h)


def test_rows_longer_than_a_round_of_lagged_waves(gpu_state):
    # more chunk steps per band than LAG * WAVES: wave 0 is still in band 0 when band WAVES could start, so the round is the band's length
    w = LAG * WAVES * CHUNK + CHUNK + 1
    check(gpu_state, 0, 8, w, WAVES * BAND + 1, "mix", seed=70, level=1)
    check(gpu_state, 3, 4, 2 * w, BAND + 1, "mix", seed=71, level=1, trns=True)


# ---- batches, the queue, counters ----------------------------------------------------------------------------------------

def jpeg_file(seed, w=48, h=40):
    from PIL import Image
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 5 + seed) % 256, (y * 6) % 256, ((x + y) * 3) % 256], axis=2).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def mixed_requests(fl):
    specs = [(2, 8, 40, 30, False), (3, 4, 33, 70, True), (0, 1, 19, 9, False), (6, 8, 65, 66, False), (0, 8, 50, 20, True)]
    reqs = []
    for k, (ct, d, w, h, trns) in enumerate(specs):
        s, plte, t = make(ct, d, w, h, 80 + k, trns)
        data = pw.write_png(s, ct, d, filters=rng(90 + k).integers(0, 5, h).tolist(), plte=plte, trns=t, split=[None, 7, "empty"][k % 3])
        reqs.append((data, fl.make_params(20, 10) if k % 2 else fl.make_params()))
    reqs.append((jpeg_file(1), fl.make_params(20, 10)))
    reqs.append((rng(99).integers(0, 256, (25, 31, 3)).astype(np.uint8), fl.make_params(20, 10)))
    return reqs


def alone(st, src, p):
    if isinstance(src, bytes):
        return st.process_png_pixels(src, p) if src[:8] == pw.SIGNATURE else st.process_jpeg_pixels(src, p)
    return st.process_pixels(src, p)


def upload_bytes(fl, data):
    i = fl.png_info(data)
    samples = pw.SAMPLES[i["color_type"]]
    return HEADER_BYTES + i["height"] * (1 + (i["width"] * samples * i["bit_depth"] + 7) // 8)


def test_mixed_batch_equals_each_request_alone_and_counters(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, s, p) for s, p in reqs]
    pngs = [s for s, _ in reqs if isinstance(s, bytes) and s[:8] == pw.SIGNATURE]
    before = gpu_state.png_counters()
    got = gpu_state.process_batch([s for s, _ in reqs], [p for _, p in reqs])
    after = gpu_state.png_counters()
    for k, (a, b) in enumerate(zip(got, each)):
        assert np.array_equal(a, b), k
    # the identity requests are the decoded pictures themselves
    assert np.array_equal(got[0], gpu_state.decode_png(reqs[0][0]))
    assert after["png_sources"] - before["png_sources"] == len(pngs)
    assert after["png_file_bytes"] - before["png_file_bytes"] == sum(len(s) for s in pngs)
    assert after["png_upload_bytes"] - before["png_upload_bytes"] == sum(upload_bytes(fl, s) for s in pngs)
    # flgpu_reset_stats clears them, flgpu_debug_set refuses them
    with pytest.raises(fl.FanlinError):
        gpu_state.debug_set("png_sources", 0)


def test_the_same_requests_through_the_queue_from_eight_threads(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, s, p) for s, p in reqs]
    before = gpu_state.png_counters()["png_sources"]
    results, errors = {}, []

    def worker(t):
        try:
            for k in range(len(reqs)):
                i = (k + t) % len(reqs)
                results[(t, i)] = alone(gpu_state, *reqs[i])
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
    assert gpu_state.png_counters()["png_sources"] - before == 8 * 5


# ---- full requests ---------------------------------------------------------------------------------------------------------

def request_file():
    y, x = np.mgrid[0:64, 0:96]
    s = np.stack([(x * 2 + y) % 256, (y * 4) % 256, (x * y) % 256], axis=2)
    return pw.write_png(s, 2, filters=rng(100).integers(0, 5, 64).tolist()), s.astype(np.uint8)


@pytest.mark.parametrize("encode_png", [False, True])
def test_process_png_equals_process_image_on_the_decoded_pixels(gpu_state, fl, encode_png):
    from PIL import Image
    data, pixels = request_file()
    content = fl.Format(fl.ENCODE_PNG if encode_png else 0)
    mime, kind, body = gpu_state.process_png(data, "w=30&h=20", content)
    mime2, kind2, body2 = gpu_state.process_image(pixels, "w=30&h=20", content, input_format=fl.IN_PNG)
    assert (mime, kind) == (mime2, kind2) == ("image/png", fl.RESULT_PNG_STREAM if encode_png else fl.RESULT_PIXELS)
    plain = gpu_state.process_pixels(pixels, fl.make_params(30, 20))
    if encode_png:
        assert isinstance(body, bytes) and body == body2
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(body))), plain)   # decodes to the FLGPU_FE_NONE pixels
    else:
        assert np.array_equal(body, body2) and np.array_equal(body, plain)
    # a negotiated container goes the same way
    webp = fl.Format(fl.ACCEPT_WEBP)
    a, b = gpu_state.process_png(data, "w=30&h=20&webp=true", webp), gpu_state.process_image(pixels, "w=30&h=20&webp=true", webp, input_format=fl.IN_PNG)
    assert a[:2] == b[:2] == ("image/webp", fl.RESULT_WEBP_PLANES)
    assert all(np.array_equal(getattr(a[2], n), getattr(b[2], n)) for n in "yuva")


def test_process_png_as_is_and_size_gate(gpu_state, fl):
    data, _ = request_file()
    assert gpu_state.process_png(data, "quality=80") == ("image/png", fl.RESULT_AS_IS, data)     # as_is never decodes: the file itself
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_png(data, "w=2001&h=1001")
    assert e.value.status == fl.ERR_PARSE
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_png(data[:40], "w=30&h=20")
    assert e.value.status == fl.ERR_PARSE


# ---- rejected inputs: they end in the host half, nothing is launched -------------------------------------------------------

def test_unsupported_and_broken_files_leave_the_context_usable(gpu_state, fl):
    from PIL import Image
    good, pixels = request_file()
    s = rng(110).integers(0, 256, (6, 8, 3))
    raw = pw.scanlines(s, 2, 8, 1)
    buf = io.BytesIO()
    Image.fromarray(rng(111).integers(0, 65536, (4, 6)).astype(np.uint16)).save(buf, "PNG")
    bad_adler = zlib.compress(raw)
    bad_adler = bad_adler[:-1] + bytes([bad_adler[-1] ^ 1])
    filter5 = bytearray(raw)
    filter5[25] = 5
    cases = [
        (buf.getvalue(), (4, 6, 1), fl.ERR_UNSUPPORTED),                                          # 16-bit samples
        (pw.write_png(s, 2, interlace=1), (6, 8, 3), fl.ERR_UNSUPPORTED),                         # Adam7
        (pw.assemble(8, 6, 8, 2, zlib.compress(raw + raw[:25])), (6, 8, 3), fl.ERR_UNSUPPORTED),  # one scanline too many
        (pw.assemble(8, 6, 8, 2, bad_adler), (6, 8, 3), fl.ERR_PARSE),
        (pw.assemble(8, 6, 8, 2, zlib.compress(bytes(filter5))), (6, 8, 3), fl.ERR_PARSE),
        (pw.assemble(8, 6, 8, 2, zlib.compress(raw)[:-3]), (6, 8, 3), fl.ERR_PARSE),
        (good[:len(good) // 2], (64, 96, 3), fl.ERR_PARSE),
        (b"not a png at all", (1, 1, 1), fl.ERR_PARSE),
        (good, (64, 96, 4), fl.ERR_INVALID_ARG),                                                  # announced channels do not match the file
        (good, (96, 64, 3), fl.ERR_INVALID_ARG),
    ]
    before = gpu_state.png_counters()["png_sources"]
    for data, shape, status in cases:
        with pytest.raises(fl.FanlinError) as e:
            gpu_state.process_png_pixels(data, fl.make_params(), shape=shape)
        assert e.value.status == status, (shape, status, str(e.value))
        if status != fl.ERR_INVALID_ARG:                                                         # the batch entry point says the same
            with pytest.raises(fl.FanlinError) as e:
                gpu_state.process_batch([data], [fl.make_params()])
            assert e.value.status == status, (shape, status, str(e.value))
        assert np.array_equal(gpu_state.decode_png(good), pixels)                                # the next request is served
    assert "do not match the file" in str(e.value)
    assert gpu_state.png_counters()["png_sources"] - before == len(cases)                         # only the good ones were decoded
