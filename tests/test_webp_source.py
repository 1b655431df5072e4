"""Lossless WebP sources decoded by the library (FLGPU_IMG_WEBP_SOURCE): prefix codes, LZ77 and colour cache on the calling thread
(tests/test_webp_source_host.py), the predictor, cross-colour, add-green and colour-indexing transforms inverted on the device
(csrc/fl_webpdec.hip).  A VP8L stream decodes to one ARGB picture fixed by the format, so every comparison is bit-exact, and the
expected pixels come from construction (tests/vp8l_write.py: the pixels a file was written from), not from a decoder.  The files
are the ones of tests/webp_cases.py, which the CPU test holds against libwebp and Pillow."""
import io
import threading

import numpy as np
import pytest

import vp8l_model as vm
import vp8l_write as vw
import webp_cases as wc

pytestmark = pytest.mark.gpu

HEADER_BYTES = vw.HEADER_DWORDS * 4


def check(st, name):
    data, want = wc.get(name)
    if want is None:
        want = vm.decode_rgba(data)   # modes 14 and 15: what libwebp makes of them
    got = st.decode_webp(data)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} of {want.size} bytes differ, first at (row, column, channel) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def names(prefix):
    out = [n for n in wc.CASES if n.startswith(prefix)]
    assert out, prefix
    return out


# ---- the predictor transform ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", range(16))
def test_each_predictor_mode(gpu_state, mode):
    check(gpu_state, f"mode{mode}_37x21")   # 14 and 15 against libwebp's decode of the same file


@pytest.mark.parametrize("mode", range(14))
def test_each_mode_on_one_row_one_column_and_one_pixel(gpu_state, mode):
    check(gpu_state, f"mode{mode}_23x1")    # row 0: L everywhere
    check(gpu_state, f"mode{mode}_1x23")    # column 0: T everywhere; the only pixel of a row is also its last
    check(gpu_state, f"mode{mode}_1x1")


@pytest.mark.parametrize("bits", [2, 3])
def test_a_random_mode_per_block(gpu_state, bits):
    check(gpu_state, f"mode_mix_bits{bits}")


@pytest.mark.parametrize("name", names("edge_"))
def test_block_edges(gpu_state, name):
    check(gpu_state, name)


# A wave walks its band of BAND rows in chunks of CHUNK steps (one pixel per step, a row two steps behind the row above it); band b
# runs on wave b % WAVES, LAG chunk steps behind band b - 1; a wave takes its next band after max(chunk steps of a band, LAG * WAVES).

@pytest.mark.parametrize("w", wc.WIDTHS)
def test_widths_around_the_chunk(gpu_state, w):
    check(gpu_state, f"kernel_w{w}")


@pytest.mark.parametrize("h", wc.HEIGHTS)
def test_heights_around_the_band_and_the_round(gpu_state, h):
    check(gpu_state, f"kernel_h{h}")


def test_rows_longer_than_a_round_of_lagged_waves(gpu_state):
    assert (wc.LONG_W + wc.SKEW + wc.CHUNK - 1) // wc.CHUNK > wc.LAG * wc.WAVES
    check(gpu_state, "kernel_long_row")


# ---- the pointwise transforms -------------------------------------------------------------------------------------------------

def test_cross_colour_with_extreme_elements(gpu_state):
    check(gpu_state, "cross_extreme")


def test_add_green(gpu_state):
    check(gpu_state, "add_green")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 256])
def test_palettes_at_widths_that_do_not_fill_the_last_packed_pixel(gpu_state, n):
    for w in (1, 3, 7, 9):
        check(gpu_state, f"palette{n}_w{w}")


@pytest.mark.parametrize("n", [1, 3, 5, 17])
def test_indices_beyond_the_palette_are_transparent_black(gpu_state, n):
    data, want = wc.get(f"palette{n}_beyond")
    assert (want.reshape(-1, 4) == 0).all(axis=1).any()
    check(gpu_state, f"palette{n}_beyond")


def test_every_order_of_every_subset_as_one_batch(gpu_state, fl):
    files = [wc.get("order_" + ("".join("PXGI"[t] for t in o) or "none")) for o in wc.ORDERS]
    assert len(files) == 65
    got = gpu_state.process_batch([d for d, _ in files], [fl.make_params()] * len(files))
    for o, (g, (_, want)) in zip(wc.ORDERS, zip(got, files)):
        assert g.shape == want.shape and np.array_equal(g, want), o


@pytest.mark.parametrize("name", names("channels_"))
def test_channels_follow_the_announced_alpha(gpu_state, fl, name):
    data, want = wc.get(name)
    assert fl.webp_info(data)["channels"] == want.shape[2] == (4 if "alpha1" in name else 3)
    check(gpu_state, name)


@pytest.mark.parametrize("name", names("stream_") + names("extended_"))
def test_entropy_stage_and_container_variants(gpu_state, name):
    check(gpu_state, name)


def test_pillow_corpus(gpu_state):
    for name, data, px in wc.pillow_corpus():
        got = gpu_state.decode_webp(data)
        assert got.shape == px.shape and np.array_equal(got, px), name


# ---- batches, the queue, shards, counters -------------------------------------------------------------------------------------

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


WEBP_IN_BATCH = ["mode_mix_bits2", "order_PXGI", "order_IGXP", "palette5_w9", "channels_alpha0_simple", "stream_groups_cache_refs", "kernel_w65"]


def mixed_requests(fl):
    reqs = [(wc.get(n)[0], fl.make_params(20, 10) if k % 2 else fl.make_params()) for k, n in enumerate(WEBP_IN_BATCH)]
    reqs.append((wc.pillow_corpus()[2][1], fl.make_params(20, 10)))
    reqs.append((jpeg_file(1), fl.make_params(20, 10)))
    reqs.append((png_file(), fl.make_params(20, 10)))
    reqs.append((wc.rng(302).integers(0, 256, (25, 31, 3)).astype(np.uint8), fl.make_params(20, 10)))
    return reqs


def is_webp(s):
    return isinstance(s, bytes) and s[:4] == b"RIFF"


def alone(st, src, p):
    if is_webp(src):
        return st.process_webp_pixels(src, p)
    if isinstance(src, bytes):
        return st.process_png_pixels(src, p) if src[:4] == b"\x89PNG" else st.process_jpeg_pixels(src, p)
    return st.process_pixels(src, p)


def test_mixed_batch_equals_each_request_alone_and_counters(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, s, p) for s, p in reqs]
    webps = [s for s, _ in reqs if is_webp(s)]
    before = gpu_state.webp_counters()
    got = gpu_state.process_batch([s for s, _ in reqs], [p for _, p in reqs])
    after = gpu_state.webp_counters()
    for k, (a, b) in enumerate(zip(got, each)):
        assert np.array_equal(a, b), k
    assert np.array_equal(got[0], wc.get(WEBP_IN_BATCH[0])[1])   # an identity request is the decoded picture itself
    assert after["webp_sources"] - before["webp_sources"] == len(webps)
    assert after["webp_file_bytes"] - before["webp_file_bytes"] == sum(len(s) for s in webps)
    blobs = [fl.debug_webp_residuals(s) for s in webps]
    assert after["webp_upload_bytes"] - before["webp_upload_bytes"] == sum(len(b) for b in blobs)
    for b in blobs:   # header + sub-images + one dword per pixel of the packed width
        H = vw.blob_header(b)
        assert len(b) == H["res_off"] + 4 * H["xsize"] * H["height"] and H["res_off"] >= HEADER_BYTES
    with pytest.raises(fl.FanlinError):
        gpu_state.debug_set("webp_sources", 0)


def test_the_same_requests_through_the_queue_from_eight_threads(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, s, p) for s, p in reqs]
    before = gpu_state.webp_counters()["webp_sources"]
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
    assert gpu_state.webp_counters()["webp_sources"] - before == 8 * sum(1 for s, _ in reqs if is_webp(s))


def test_the_same_requests_on_two_shards(gpu_state, fl):
    reqs = mixed_requests(fl)
    each = [alone(gpu_state, s, p) for s, p in reqs]
    with fl.State(devices=[0, 0]) as two:
        got = two.process_batch([s for s, _ in reqs], [p for _, p in reqs])
        for k, (a, b) in enumerate(zip(got, each)):
            assert np.array_equal(a, b), k
        assert two.webp_counters()["webp_sources"] == sum(1 for s, _ in reqs if is_webp(s))
        assert np.array_equal(two.decode_webp(reqs[1][0]), wc.get(WEBP_IN_BATCH[1])[1])


# ---- full requests ---------------------------------------------------------------------------------------------------------------

def request_file(orientation=None, alpha=False):
    y, x = np.mgrid[0:64, 0:96]
    px = np.stack([(x * 2 + y) % 256, (y * 4) % 256, (x * y) % 256, np.full_like(x, 255) if not alpha else (x + y) % 256], axis=2).astype(np.uint8)
    ext = None if orientation is None else dict(alpha=alpha, after=[(b"EXIF", vw.exif(orientation, prefix=bool(orientation & 1)))])
    data = vw.write(px, [(vw.GREEN,), (vw.PREDICTOR, 3, wc.mode_mix(96, 64, 3)), (vw.CROSS, 4, (5, -9, 17))], alpha_bit=int(alpha), extended=ext, cache_bits=5)
    return data, px if alpha else px[..., :3]


def same(p, q):
    """payloads of process_image: pixels, or the planes for a host WebP encoder"""
    return np.array_equal(p, q) if isinstance(p, np.ndarray) else all(np.array_equal(getattr(p, n), getattr(q, n)) for n in "yuva")


@pytest.mark.parametrize("lossless", [False, True])
def test_process_webp_equals_process_image_on_the_decoded_pixels(gpu_state, fl, lossless):
    data, pixels = request_file()
    assert np.array_equal(vm.decode_rgba(data)[..., :3], pixels)
    content = fl.Format(fl.ENCODE_WEBP_LOSSLESS if lossless else 0)
    query = "w=30&h=20&quality=100" if lossless else "w=30&h=20"
    mime, kind, body = gpu_state.process_webp(data, query, content)
    mime2, kind2, body2 = gpu_state.process_image(pixels, query, content, input_format=fl.IN_WEBP)
    assert (mime, kind) == (mime2, kind2)
    plain = gpu_state.process_pixels(pixels, fl.make_params(30, 20))
    if lossless:
        # a WebP source leaves as a finished lossless WebP file: libwebp decodes the body to the FE_NONE pixels
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM)
        assert isinstance(body, bytes) and body == body2
        assert np.array_equal(vm.decode_rgba(body), vm.into_rgba8(plain))
    else:
        assert mime == "image/webp" and same(body, body2)
    # an accepted container goes the same way
    webp = fl.Format(fl.ACCEPT_WEBP)
    a, b = gpu_state.process_webp(data, "w=30&h=20&webp=true", webp), gpu_state.process_image(pixels, "w=30&h=20&webp=true", webp, input_format=fl.IN_WEBP)
    assert a[:2] == b[:2] == ("image/webp", fl.RESULT_WEBP_PLANES)
    assert same(a[2], b[2])


@pytest.mark.parametrize("orientation", range(2, 9))
def test_process_webp_honours_the_exif_orientation(gpu_state, fl, orientation):
    data, pixels = request_file(orientation, alpha=bool(orientation & 2))
    assert fl.webp_info(data)["exif_orientation"] == orientation
    a = gpu_state.process_webp(data, "w=30&h=20")
    b = gpu_state.process_image(pixels, "w=30&h=20", None, input_format=fl.IN_WEBP, orientation=orientation)
    c = gpu_state.process_image(pixels, "w=30&h=20", None, input_format=fl.IN_WEBP, orientation=1)
    assert a[:2] == b[:2]
    assert same(a[2], b[2])
    assert not same(a[2], c[2])   # (the orientation changes this picture)
    assert np.array_equal(gpu_state.decode_webp(data), pixels)   # flgpu_decode_webp applies none


def test_process_webp_as_is_and_size_gate(gpu_state, fl):
    data, _ = request_file()
    assert gpu_state.process_webp(data, "") == ("image/webp", fl.RESULT_AS_IS, data)          # input format WebP: an empty query is as_is
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_webp(data, "w=2001&h=1001")
    assert e.value.status == fl.ERR_PARSE
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_webp(data[:40], "w=30&h=20")
    assert e.value.status == fl.ERR_PARSE


# ---- rejected inputs: they end in the host half, nothing is launched -----------------------------------------------------------

def test_unsupported_and_broken_files_leave_the_context_usable(gpu_state, fl):
    from PIL import Image
    good, pixels = request_file()
    img = wc.rng(310).integers(0, 256, (6, 8, 4)).astype(np.uint8)
    lossy, lossy_alpha, anim = io.BytesIO(), io.BytesIO(), io.BytesIO()
    Image.fromarray(img[..., :3]).save(lossy, "WEBP", quality=80)
    Image.fromarray(img).save(lossy_alpha, "WEBP", quality=80)
    Image.fromarray(img[..., :3]).save(anim, "WEBP", save_all=True, append_images=[Image.fromarray(255 - img[..., :3])], lossless=True)
    plain, ppx = wc.get("mode11_37x21")
    cut = plain[:len(plain) - 40]
    cut = cut[:4] + (len(cut) - 8).to_bytes(4, "little") + cut[8:16] + (len(cut) - 20).to_bytes(4, "little") + cut[20:]   # sizes repaired: the stream ends early
    cases = [
        (lossy.getvalue(), (6, 8, 3), fl.ERR_UNSUPPORTED),
        (lossy_alpha.getvalue(), (6, 8, 4), fl.ERR_UNSUPPORTED),
        (anim.getvalue(), (6, 8, 3), fl.ERR_UNSUPPORTED),
        (cut, (21, 37, 4), fl.ERR_PARSE),
        (good[:len(good) // 2], (64, 96, 3), fl.ERR_PARSE),
        (b"RIFF\x04\0\0\0WEBPnot a webp at all", (1, 1, 3), fl.ERR_PARSE),
        (good, (64, 96, 4), fl.ERR_INVALID_ARG),        # announced channels do not match the file
        (good, (96, 64, 3), fl.ERR_INVALID_ARG),
    ]
    before = gpu_state.webp_counters()["webp_sources"]
    for data, shape, status in cases:
        with pytest.raises(fl.FanlinError) as e:
            gpu_state.process_webp_pixels(data, fl.make_params(), shape=shape)
        assert e.value.status == status, (shape, status, str(e.value))
        if status != fl.ERR_INVALID_ARG:               # the batch entry point says the same
            with pytest.raises(fl.FanlinError) as e:
                gpu_state.process_batch([data], [fl.make_params()])
            assert e.value.status == status, (shape, status, str(e.value))
        assert np.array_equal(gpu_state.decode_webp(good), pixels)   # the next request is served
    assert "do not match the file" in str(e.value)
    assert gpu_state.webp_counters()["webp_sources"] - before == len(cases)   # only the good ones were decoded
