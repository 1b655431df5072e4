"""Adam7-interlaced PNG sources decoded by the library (FLGPU_IMG_PNG_SOURCE | FLGPU_IMG_PNG_ADAM7, FLGPU_DECODE_PNG_ADAM7): inflate on
the calling thread (tests/test_png_adam7_host.py), then on the device one unfilter job per non-empty pass and png_adam7_kernel, which
puts the seven reduced pictures together while it expands the samples (csrc/fl_pngdec.hip).  The result is determined by the PNG
specification, so every comparison is bit-exact, and the expected pixels come from construction (tests/png_adam7_write.py: the samples
a file was written from), not from a decoder.  Many small files go through process_batch as one batch."""
import io
import os
import re
import threading
import zlib

import numpy as np
import pytest

import png_adam7_write as aw
import png_write as pw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    text = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_pngdec.h")).read()
    return {k: int(v) for k, v in re.findall(r"(kPd(?:Waves|BandRows|Chunk|Lag)) = (\d+)", text)}


K = kernel_constants()
WAVES, BAND, CHUNK, LAG = K["kPdWaves"], K["kPdBandRows"], K["kPdChunk"], K["kPdLag"]
HEADER_BYTES = 16 * 4 + 256 * 4   # csrc/fl_pngsrc.h PngBlobHeader: what crosses PCIe in front of the scanlines

COMBOS = [(ct, d, t) for ct, d in [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)]
          for t in (False, True) if not (t and ct in (4, 6))]


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


def mixed(seed):
    """A filter type per pass row, seeded."""
    r = rng(seed)
    return lambda k, ph: r.integers(0, 5, ph).tolist()


def case(ct, depth, w, h, filters, seed=0, trns=False, **kw):
    """(file, expected pixels, label)"""
    s, plte, t = make(ct, depth, w, h, seed, trns)
    if filters == "mix":
        filters = mixed(seed + 1)
    return aw.write_png(s, ct, depth, filters=filters, plte=plte, trns=t, **kw), pw.expand(s, ct, depth, plte, t), (ct, depth, w, h, trns)


def check_batch(st, fl, cases):
    """All the files as ONE flgpu_transform_batch of identity requests."""
    got = st.process_batch([fl.Adam7Png(data) for data, _, _ in cases], [fl.make_params()] * len(cases))
    for g, (_, want, label) in zip(got, cases):
        assert g.shape == want.shape, (label, g.shape, want.shape)
        if not np.array_equal(g, want):
            bad = np.argwhere(g != want)
            raise AssertionError(f"{label}: {len(bad)} of {want.size} bytes differ, first at (row, column, channel) {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[tuple(bad[0])]}")


# ---- geometry: absent passes, one-pixel passes, pass rows of one byte -----------------------------------------------------

@pytest.mark.parametrize("ct,depth,trns", [(2, 8, False), (3, 2, True)])
def test_every_size_up_to_nine_by_nine(gpu_state, fl, ct, depth, trns):
    cases = [case(ct, depth, w, h, "mix", seed=100 + 16 * w + h, trns=trns) for w in range(1, 10) for h in range(1, 10)]
    assert len(cases) == 81
    check_batch(gpu_state, fl, cases)


# ---- colour types and depths: pass widths that leave sub-byte pass rows with unused bits ------------------------------------

@pytest.mark.parametrize("w,h", [(13, 11), (37, 21)])
def test_each_colour_type_depth_and_trns(gpu_state, fl, w, h):
    check_batch(gpu_state, fl, [case(ct, d, w, h, "mix", seed=200 + 8 * ct + d, trns=t) for ct, d, t in COMBOS])


# ---- filters ------------------------------------------------------------------------------------------------------------

def test_each_filter_type_on_every_row_of_every_pass_and_a_mix(gpu_state, fl):
    check_batch(gpu_state, fl, [case(ct, 8, 37, 21, f, seed=300 + ct) for ct in (0, 4, 2, 6) for f in (0, 1, 2, 3, 4, "mix")])   # bpp 1, 2, 3, 4


def test_the_first_row_of_a_pass_has_no_row_above(gpu_state, fl):
    # every pass begins with Up / Average / Paeth over non-zero data: a "row above" taken from the last row of the pass before (or from
    # anywhere but zeros) changes the result.  The rows behind the first are Sub, so the first row's error would spread no further.
    cases = []
    for ct in (0, 4, 2, 6):
        for first in (2, 3, 4):
            s = rng(310 + ct).integers(1, 256, (21, 37, pw.SAMPLES[ct]))                      # no zero sample anywhere
            data = aw.write_png(s, ct, 8, filters=lambda k, ph, first=first: [first] + [1] * (ph - 1))
            cases.append((data, pw.expand(s, ct, 8), (ct, "first row", first)))
    check_batch(gpu_state, fl, cases)


# ---- sizes: the smallest at which a pass crosses each boundary of png_unfilter_kernel ------------------------------------------
# A wave walks its band of BAND rows in chunks of CHUNK steps (one pixel per step); band b runs on wave b % WAVES, LAG chunk steps
# behind band b - 1; a wave takes its next band after max(chunk steps of a band, LAG * WAVES) steps.  Pass 7 is h // 2 rows of w
# pixels, pass 6 (h + 1) // 2 rows of w // 2, pass 1 ceil(h / 8) rows of ceil(w / 8).

def test_pass_heights_around_the_band_and_the_round(gpu_state, fl):
    cases = [case(ct, 8, 5, h, "mix", seed=400 + h) for h in (2 * BAND - 2, 2 * BAND, 2 * BAND + 2) for ct in (2, 0)]     # h // 2 = BAND - 1, BAND, BAND + 1
    cases += [case(ct, 8, 3, 2 * (WAVES * BAND + 1), "mix", seed=410 + ct) for ct in (2, 0)]                             # h // 2 = WAVES * BAND + 1: a wave takes a second band
    cases += [case(ct, 8, 9, 8 * BAND + 1, "mix", seed=420 + ct) for ct in (2, 6)]                                       # ceil(h / 8) = BAND + 1: pass 1 has a second band
    check_batch(gpu_state, fl, cases)


def test_pass_widths_around_the_chunk_and_rows_longer_than_a_round(gpu_state, fl):
    # pass 7 (w pixels a row) and pass 6 (w // 2) around one and two chunks
    widths = sorted({CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1,
                     2 * (CHUNK - 1), 2 * CHUNK + 2, 2 * (2 * CHUNK - 1), 4 * CHUNK, 4 * CHUNK + 2})
    cases = [case(ct, 8, w, 9, "mix", seed=500 + w) for w in widths for ct in (0, 2, 6)]
    # a pass-7 row of more chunk steps than LAG * WAVES: the round is the band's own length
    w = LAG * WAVES * CHUNK + CHUNK + 1
    cases += [case(0, 8, w, 3, "mix", seed=510), case(2, 8, w, 3, "mix", seed=511), case(3, 4, 2 * w, 3, "mix", seed=512, trns=True)]
    check_batch(gpu_state, fl, cases)


# ---- twins: the same samples written interlaced and non-interlaced ---------------------------------------------------------

def twins():
    y, x = np.mgrid[0:64, 0:96]
    s = np.stack([(x * 2 + y) % 256, (y * 4) % 256, (x * y) % 256], axis=2)
    return aw.write_png(s, 2, filters=mixed(600)), pw.write_png(s, 2, filters=rng(601).integers(0, 5, 64).tolist()), s.astype(np.uint8)


def test_twins_decode_and_process_alike(gpu_state, fl):
    inter, plain, pixels = twins()
    assert np.array_equal(gpu_state.decode_png(inter, adam7=True), pixels)
    assert np.array_equal(gpu_state.decode_png(plain), pixels)
    assert np.array_equal(gpu_state.decode_png(plain, adam7=True), pixels)             # the flag changes nothing for a non-interlaced file
    bits = fl.Format(fl.DECODE_PNG_ADAM7)
    for query in ("w=30&h=20", "w=30&h=20&crop=true", "grayscale=true&blur=2"):
        a, b = gpu_state.process_png(inter, query, bits), gpu_state.process_png(plain, query)
        assert a[:2] == b[:2] == ("image/png", fl.RESULT_PIXELS), query
        assert np.array_equal(a[2], b[2]), query
    a = gpu_state.process_png(inter, "w=30&h=20", fl.Format(fl.DECODE_PNG_ADAM7 | fl.ENCODE_PNG))
    b = gpu_state.process_png(plain, "w=30&h=20", fl.Format(fl.ENCODE_PNG))
    assert a[:2] == b[:2] == ("image/png", fl.RESULT_PNG_STREAM)
    assert isinstance(a[2], bytes) and a[2] == b[2]
    # as_is never decodes: the interlaced file itself, with or without the bit
    assert gpu_state.process_png(inter, "quality=80") == ("image/png", fl.RESULT_AS_IS, inter)
    assert gpu_state.process_png(inter, "quality=80", bits) == ("image/png", fl.RESULT_AS_IS, inter)


# ---- batches, the queue, counters ----------------------------------------------------------------------------------------

def jpeg_file(seed, w=48, h=40):
    from PIL import Image
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 5 + seed) % 256, (y * 6) % 256, ((x + y) * 3) % 256], axis=2).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def mixed_requests(fl):
    """Adam7 PNG files, plain PNG files, a JPEG file and pixels: [(source, params)]"""
    specs = [(2, 8, 40, 30, False), (3, 4, 33, 70, True), (0, 1, 19, 9, False), (6, 8, 65, 66, False), (0, 8, 50, 20, True)]
    reqs = []
    for k, (ct, d, w, h, trns) in enumerate(specs):
        s, plte, t = make(ct, d, w, h, 700 + k, trns)
        data = aw.write_png(s, ct, d, filters=mixed(710 + k), plte=plte, trns=t, split=[None, 7, "empty"][k % 3])
        reqs.append((fl.Adam7Png(data), fl.make_params(20, 10) if k % 2 else fl.make_params()))
    for k, (ct, d, w, h, trns) in enumerate(specs[:2]):
        s, plte, t = make(ct, d, w, h, 720 + k, trns)
        reqs.append((pw.write_png(s, ct, d, filters=rng(730 + k).integers(0, 5, h).tolist(), plte=plte, trns=t), fl.make_params(20, 10)))
    reqs.append((jpeg_file(1), fl.make_params(20, 10)))
    reqs.append((rng(799).integers(0, 256, (25, 31, 3)).astype(np.uint8), fl.make_params(20, 10)))
    return reqs


def alone(st, fl, src, p):
    if isinstance(src, fl.Adam7Png):
        return st.process_png_pixels(bytes(src), p, adam7=True)
    if isinstance(src, bytes):
        return st.process_png_pixels(src, p) if src[:8] == pw.SIGNATURE else st.process_jpeg_pixels(src, p)
    return st.process_pixels(src, p)


def upload_bytes(fl, data):
    """The documented arithmetic: the header + the scanlines -- for an Adam7 file the sum over its non-empty passes."""
    i = fl.png_info(data, adam7=True)
    if i["interlaced"]:
        return HEADER_BYTES + aw.scan_bytes(i["width"], i["height"], i["color_type"], i["bit_depth"])
    return HEADER_BYTES + i["height"] * (1 + (i["width"] * pw.SAMPLES[i["color_type"]] * i["bit_depth"] + 7) // 8)


def test_mixed_batch_equals_each_request_alone_and_counters(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, fl, s, p) for s, p in reqs]
    pngs = [bytes(s) for s, _ in reqs if isinstance(s, bytes) and s[:8] == pw.SIGNATURE]
    assert len(pngs) == 7
    before = gpu_state.png_counters()
    got = gpu_state.process_batch([s for s, _ in reqs], [p for _, p in reqs])
    after = gpu_state.png_counters()
    for k, (a, b) in enumerate(zip(got, each)):
        assert np.array_equal(a, b), k
    assert np.array_equal(got[0], gpu_state.decode_png(bytes(reqs[0][0]), adam7=True))    # an identity request is the decoded picture
    assert after["png_sources"] - before["png_sources"] == len(pngs)
    assert after["png_file_bytes"] - before["png_file_bytes"] == sum(len(s) for s in pngs)
    assert after["png_upload_bytes"] - before["png_upload_bytes"] == sum(upload_bytes(fl, s) for s in pngs)


def test_a_non_interlaced_files_upload_bytes_are_unchanged(gpu_state, fl):
    _, plain, _ = twins()
    want = HEADER_BYTES + 64 * (1 + 96 * 3)
    for adam7 in (False, True):
        before = gpu_state.png_counters()
        gpu_state.decode_png(plain, adam7=adam7)
        after = gpu_state.png_counters()
        assert after["png_upload_bytes"] - before["png_upload_bytes"] == want == upload_bytes(fl, plain)
        assert after["png_sources"] - before["png_sources"] == 1


def test_the_same_requests_through_the_queue_from_eight_threads(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, fl, s, p) for s, p in reqs]
    before = gpu_state.png_counters()["png_sources"]
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
    assert gpu_state.png_counters()["png_sources"] - before == 8 * 7


# ---- opt-in, still unsupported, damaged ------------------------------------------------------------------------------------

def expect(fl, status, fn, *args, **kw):
    with pytest.raises(fl.FanlinError) as e:
        fn(*args, **kw)
    assert e.value.status == status, (status, str(e.value))
    return str(e.value)


def test_without_the_bits_an_interlaced_file_is_unsupported_as_before(gpu_state, fl):
    inter, _, pixels = twins()
    text = expect(fl, fl.ERR_UNSUPPORTED, gpu_state.process_png_pixels, inter, fl.make_params(), shape=(64, 96, 3))
    assert "Adam7 interlace" in text                                                        # the text of before
    expect(fl, fl.ERR_UNSUPPORTED, gpu_state.process_batch, [inter], [fl.make_params()])
    expect(fl, fl.ERR_UNSUPPORTED, gpu_state.decode_png, inter)
    expect(fl, fl.ERR_UNSUPPORTED, gpu_state.process_png, inter, "w=30&h=20")
    expect(fl, fl.ERR_UNSUPPORTED, gpu_state.process_png, inter, "w=30&h=20", fl.Format(fl.ENCODE_PNG))
    assert np.array_equal(gpu_state.decode_png(inter, adam7=True), pixels)
    # FLGPU_IMG_PNG_ADAM7 is a flag beside FLGPU_IMG_PNG_SOURCE: on pixels it is an invalid argument
    import ctypes as C
    img = np.ascontiguousarray(pixels)
    out = np.empty(img.nbytes, np.uint8)
    src = fl.flgpu_image(img.ctypes.data, img.nbytes, 96, 64, 3, fl.IMG_PNG_ADAM7)
    dst = fl.flgpu_image(out.ctypes.data, out.nbytes, 0, 0, 0, 0)
    p = fl.make_params()
    assert gpu_state._lib.flgpu_transform(gpu_state._ctx, C.byref(src), C.byref(p), C.byref(dst)) == fl.ERR_INVALID_ARG
    assert np.array_equal(gpu_state.process_pixels(img, fl.make_params()), pixels)


def test_still_unsupported_and_damaged_files_leave_the_context_usable(gpu_state, fl):
    from PIL import Image
    good, _, pixels = twins()
    s = rng(800).integers(0, 256, (11, 13, 3))
    raw = aw.scanlines(s, 2, 8, 1)
    buf = io.BytesIO()
    Image.fromarray(rng(801).integers(0, 65536, (4, 6)).astype(np.uint16)).save(buf, "PNG")
    sixteen = buf.getvalue()[:8] + pw.ihdr(6, 4, 16, 0, 1) + buf.getvalue()[8 + 25:]
    bad_adler = zlib.compress(raw)
    bad_adler = bad_adler[:-1] + bytes([bad_adler[-1] ^ 1])
    filter5 = bytearray(raw)
    filter5[41] = 5                                                                         # the first row of pass 4 (tests/test_png_adam7_host.py)

    def file(stream):
        return pw.assemble(13, 11, 8, 2, stream, interlace=1)

    cases = [
        (sixteen, (4, 6, 1), fl.ERR_UNSUPPORTED),                                             # 16-bit samples, interlaced
        (file(zlib.compress(raw + b"\0")), (11, 13, 3), fl.ERR_UNSUPPORTED),                  # one scanline byte too many
        (file(bad_adler), (11, 13, 3), fl.ERR_PARSE),
        (file(zlib.compress(bytes(filter5))), (11, 13, 3), fl.ERR_PARSE),
        (file(zlib.compress(raw[:-1])), (11, 13, 3), fl.ERR_PARSE),                           # one byte too few
        (file(zlib.compress(raw)[:-3]), (11, 13, 3), fl.ERR_PARSE),
        (good[:len(good) // 2], (64, 96, 3), fl.ERR_PARSE),
        (good, (64, 96, 4), fl.ERR_INVALID_ARG),                                              # announced channels do not match the file
    ]
    assert np.array_equal(gpu_state.decode_png(file(zlib.compress(raw)), adam7=True), s)     # the undamaged file of the cases above
    before = gpu_state.png_counters()["png_sources"]
    for data, shape, status in cases:
        expect(fl, status, gpu_state.process_png_pixels, data, fl.make_params(), shape=shape, adam7=True)
        if status != fl.ERR_INVALID_ARG:                                                     # the batch entry point says the same
            expect(fl, status, gpu_state.process_batch, [fl.Adam7Png(data)], [fl.make_params()])
        assert np.array_equal(gpu_state.decode_png(good, adam7=True), pixels)                # the next request is served
    assert gpu_state.png_counters()["png_sources"] - before == len(cases)                     # only the good ones were decoded
