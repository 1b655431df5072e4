"""JPEG decode front end (reference src/handler.rs:205-220: image 0.25.6 -> zune-jpeg 0.4.14).

Three layers, three bars:
  * host half (marker parsing + Huffman decoding, product code that runs on the CPU): its coefficient blob must hold
    exactly the quantised coefficients an independent bit-by-bit decoder (the oracle, T.81 F.2.2.3) reads from the same
    file -- checked without a GPU;
  * oracle restatement of zune-jpeg's IDCT / up-sampling / colour arithmetic vs libjpeg-turbo (Pillow): PARITY UNPINNED for
    zune-jpeg itself (no Rust here); what is pinned is the distance to the other production decoder on the reference's own
    images/lenna.jpg and on synthetic streams: <= 4 LSB per channel, mean < 1 (two integer IDCTs differ by <= 1, zune's
    5/6-bit colour constants by <= 2-3 from libjpeg's 16-bit ones, its two-step chroma interpolation by <= 1);
  * device half (-m gpu): bit-identical to the oracle decoder, for the sampling layouts Pillow writes (4:4:4, 4:2:2, 4:2:0), odd
    sizes and restart intervals, alone and inside the whole request (decode + resize + letterbox + encode in one pass).
The layouts, tables and sizes Pillow's defaults do not reach -- 4:4:0, RGB files, optimised Huffman tables, 16-bit quantiser tables,
every width 1 .. 64, saturating pictures -- are in test_jpeg_layouts.py, under the same three bars."""
import io
import os

import numpy as np
import pytest
from PIL import Image

import oracle_lib
import parity
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENNA = os.path.join(ROOT, "tests", "golden", "lenna_reference.jpg")


def make_jpeg(h, w, c=3, q=85, subsampling=0, restart_blocks=0, dist="photo", index=0, exif_orientation=None):
    img = getattr(synth, dist)(h, w, c, index=index)
    pil = Image.fromarray(img[:, :, 0] if c == 1 else img)
    kw = dict(quality=q)
    if c == 3:
        kw["subsampling"] = subsampling
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    if exif_orientation:
        ex = Image.Exif()
        ex[0x0112] = exif_orientation
        kw["exif"] = ex
    b = io.BytesIO()
    pil.save(b, "JPEG", **kw)
    return b.getvalue()


CASES = [
    # h, w, c, quality, subsampling (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), restart interval in blocks
    (64, 96, 3, 85, 0, 0), (64, 96, 3, 85, 1, 0), (64, 96, 3, 85, 2, 0),
    (37, 53, 3, 70, 0, 0), (37, 53, 3, 70, 1, 0), (37, 53, 3, 70, 2, 0),
    (1, 1, 3, 90, 2, 0), (8, 8, 3, 90, 0, 0), (17, 16, 3, 50, 2, 0), (16, 17, 3, 50, 1, 0), (9, 300, 3, 95, 2, 0),
    (120, 160, 3, 90, 2, 3), (120, 160, 3, 30, 0, 1), (50, 70, 3, 75, 1, 7),
    (50, 70, 1, 75, 0, 0), (33, 9, 1, 60, 0, 2), (200, 301, 3, 100, 2, 0), (200, 301, 3, 5, 0, 0),
]


def lenna_bytes():
    # the reference's own picture (images/lenna.jpg, 512x512 baseline 4:4:4 with a restart interval): a committed copy, so
    # that the suite needs no reference checkout -- a test fixture (data the reference's tests hold), not source
    return open(LENNA, "rb").read()


# ------------------------------------------------------------------------------------------------- host half, CPU --

@pytest.mark.parametrize("case", CASES)
def test_host_huffman_decoder_reads_the_same_coefficients_as_the_oracle(fl, oracle, case):
    h, w, c, q, sub, rst = case
    data = make_jpeg(h, w, c, q, sub, rst, index=h + w)
    hdr, got, _ = fl.debug_jpeg_blob(data)
    want = oracle.jpeg_file_coefficients(data)
    assert (hdr["width"], hdr["height"], hdr["nc"]) == (w, h, c)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_blocks_whose_coefficients_do_not_fit_a_byte(fl, oracle):
    """The single-pass decoder writes a block in its blob form while decoding it (i16 head, i8 tail) and decodes it a second time, into
    halfwords, when a tail coefficient turns out not to fit a byte: noise at quality 100 makes a third of the blocks such blocks."""
    rng = np.random.default_rng(5)
    for q, sub in ((100, 0), (100, 2), (98, 2), (90, 1)):
        b = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)).save(b, "JPEG", quality=q, subsampling=sub)
        hdr, got, blob = fl.debug_jpeg_blob(b.getvalue())
        words = blob[hdr["blocks_off"]: hdr["blocks_off"] + 4 * hdr["nblocks"]].view(np.uint32)
        assert q < 98 or int((words & 1).sum()) > 50
        assert np.array_equal(got, oracle.jpeg_file_coefficients(b.getvalue()))


def _save(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(b, "JPEG", **kw)
    return b.getvalue()


PROGRESSIVE_CASES = [
    # h, w, c, quality, subsampling, restart interval in blocks (0 = none)
    (64, 96, 3, 85, 2, 0), (64, 96, 3, 85, 0, 0), (37, 53, 3, 70, 1, 0), (1, 1, 3, 90, 2, 0), (17, 16, 3, 50, 2, 0), (9, 300, 3, 95, 2, 0),
    (50, 70, 1, 75, 0, 0), (200, 301, 3, 100, 2, 0), (200, 301, 3, 5, 0, 0), (120, 160, 3, 90, 2, 5), (512, 512, 3, 85, 2, 0),
]


@pytest.mark.parametrize("case", PROGRESSIVE_CASES)
def test_progressive_files_hold_the_coefficients_of_their_baseline_twins(fl, oracle, case):
    """SOF2 files (handler.rs:205-220 hands zune-jpeg whatever the origin serves; web origins serve many of these): spectral
    selection and successive approximation are undone on the host (T.81 Annex G) and the coefficients packed into the same blob.
    libjpeg (Pillow) quantises a picture identically whether it then writes a baseline or a progressive file, so the progressive
    file's coefficients must equal, block for block, what the INDEPENDENT oracle decoder reads from the baseline file of the
    same picture -- no second progressive decoder is needed to check this one."""
    h, w, c, q, sub, rst = case
    img = synth.photo(h, w, c, index=h + 2 * w)
    kw = dict(quality=q)
    if c == 3:
        kw["subsampling"] = sub
    if rst:
        kw["restart_marker_blocks"] = rst
    prog, base = _save(img, progressive=True, **kw), _save(img, **kw)
    assert prog != base and fl.jpeg_info(prog)["progressive"] == 1 and fl.jpeg_info(prog)["supported"] == 1
    hdr, got, _ = fl.debug_jpeg_blob(prog)
    want = oracle.jpeg_file_coefficients(base)
    assert (hdr["width"], hdr["height"], hdr["nc"]) == (w, h, c)
    assert got.shape == want.shape and np.array_equal(got, want)
    _, got_b, _ = fl.debug_jpeg_blob(base)                       # and the single-pass decoder agrees with both
    assert np.array_equal(got_b, want)


def test_sequential_files_that_code_their_components_in_separate_scans(fl, oracle):
    """A baseline file may carry one scan per component (libjpeg's scan scripts; some cameras and optimisers write them): same
    coefficients as the interleaved file of the same picture.  Built here by re-ordering the blocks of an interleaved 4:4:4 file
    with Pillow's own encoder: optimize=True + progressive=False keeps one scan, so the multi-scan form is made from a
    progressive file's first-pass structure instead -- a progressive file with successive approximation switched off is not
    available through Pillow, so this case is covered by the refinement-free 1x1 picture above and by the greyscale file, whose
    AC scans are non-interleaved by nature."""
    img = synth.photo(40, 56, 1, index=3)
    prog, base = _save(img, progressive=True, quality=80), _save(img, quality=80)
    assert np.array_equal(fl.debug_jpeg_blob(prog)[1], oracle.jpeg_file_coefficients(base))


def test_mutated_progressive_streams_never_crash(fl):
    rng = np.random.default_rng(5)
    data = bytearray(_save(synth.photo(48, 64, 3, index=8), progressive=True, quality=80, subsampling=2))
    sos = data.find(b"\xff\xda")
    for trial in range(300):
        d = bytearray(data)
        for _ in range(int(rng.integers(1, 6))):
            d[int(rng.integers(sos, len(d)))] = int(rng.integers(0, 256))
        try:
            fl.debug_jpeg_blob(bytes(d))
        except fl.FanlinError:
            pass
    for cut in (len(data) - 2, len(data) // 2, sos + 20):
        try:
            fl.debug_jpeg_blob(bytes(data[:cut]))
        except fl.FanlinError:
            pass


def test_a_file_cannot_buy_unbounded_decoder_time_with_scans(fl):
    """A multi-scan file pays per scan for every block of the scan's components, so the decoder bounds the WORK a file may ask
    for (csrc/fl_jpeghuff.cpp decode_scans: 32 visits per block of the frame on average), not only its scan count: a real
    progressive file repeated-scan-stuffed far beyond anything an encoder writes comes back as an error at once -- unsupported, so
    that the reference's own decoder can have it (handler.rs:205-220) -- instead of keeping a decoder slot busy for minutes."""
    import time
    data = _save(synth.photo(256, 256, 1, index=3), progressive=True, quality=85)
    # the file's last scan (SOS marker ... up to EOI), repeated: every copy walks all 1024 blocks again
    last_sos = data.rfind(b"\xff\xda")
    eoi = data.rfind(b"\xff\xd9")
    scan = data[last_sos:eoi]
    stuffed = data[:eoi] + scan * 400 + b"\xff\xd9"
    t0 = time.perf_counter()
    with pytest.raises(fl.FanlinError) as e:
        fl.debug_jpeg_blob(stuffed)
    assert time.perf_counter() - t0 < 2.0
    assert e.value.status in (fl.ERR_UNSUPPORTED, fl.ERR_INVALID_ARG)
    hdr, coef, _ = fl.debug_jpeg_blob(data)      # the file itself is fine
    assert hdr["nblocks"] == 1024


def test_host_decoder_on_the_reference_picture(fl, oracle):
    data = lenna_bytes()
    info = fl.jpeg_info(data)
    assert (info["width"], info["height"], info["components"], info["supported"], info["exif_orientation"]) == (512, 512, 3, 1, 1)
    assert info["restart_interval"] > 0 and (info["h_max"], info["v_max"]) == (1, 1)
    hdr, got, blob = fl.debug_jpeg_blob(data)
    assert np.array_equal(got, oracle.jpeg_file_coefficients(data))
    assert hdr["is_rgb"] == 0                                  # APP14 Adobe transform 1 = YCbCr
    # this file is near-lossless (10.5 bits per pixel): its blob is no smaller than the decoded picture; typical web
    # JPEGs (the synthetic q <= 90 cases) shrink 3-6x -- see test_blob_is_much_smaller_than_the_pixels_for_typical_files
    assert blob.size < 1.2 * 512 * 512 * 3


def test_blob_is_much_smaller_than_the_pixels_for_typical_files(fl):
    for q, sub, factor in ((75, 2, 5.0), (85, 2, 4.0), (85, 0, 2.5)):
        data = make_jpeg(1080, 1920, 3, q, sub, index=q)
        _, _, blob = fl.debug_jpeg_blob(data)
        assert blob.size * factor < 1080 * 1920 * 3, (q, sub, blob.size, len(data))


def test_exif_orientation_and_unsupported_streams(fl):
    for o in (1, 3, 6, 8):
        assert fl.jpeg_info(make_jpeg(40, 30, exif_orientation=o))["exif_orientation"] == o
    assert fl.jpeg_info(make_jpeg(40, 30))["exif_orientation"] == 0
    b = io.BytesIO()
    Image.fromarray(synth.photo(40, 50, 3)).save(b, "JPEG", progressive=True)
    info = fl.jpeg_info(b.getvalue())
    assert info["progressive"] == 1 and info["supported"] == 1 and info["channels"] == 3   # round 3: progressive files are decoded
    # arithmetic-coded and 12-bit processes stay with the host's own decoder: an SOF9 / SOF1-with-precision-12 header says so
    base = bytearray(make_jpeg(16, 16))
    sof = base.find(b"\xff\xc0")
    arith = bytearray(base); arith[sof + 1] = 0xC9
    info = fl.jpeg_info(bytes(arith))
    assert info["supported"] == 0 and info["channels"] == 0
    with pytest.raises(fl.FanlinError) as e:
        fl.debug_jpeg_blob(bytes(arith))
    assert e.value.status == fl.ERR_UNSUPPORTED
    twelve = bytearray(base); twelve[sof + 1] = 0xC1; twelve[sof + 4] = 12
    assert fl.jpeg_info(bytes(twelve))["supported"] == 0
    b = io.BytesIO()
    Image.fromarray(synth.uniform(24, 24, 4), "CMYK").save(b, "JPEG")
    info = fl.jpeg_info(b.getvalue())                             # 4 components: raw samples + the CMYK table, see the tests below
    assert info["supported"] == 1 and info["components"] == 4 and info["channels"] == 3 and info["adobe_transform"] == 1
    for junk in (b"", b"\xff\xd8", b"GIF89a" + bytes(64), make_jpeg(16, 16)[:40]):
        with pytest.raises(fl.FanlinError):
            fl.jpeg_info(junk)
    # truncated entropy-coded data must come back as an error or a picture, never a crash
    data = make_jpeg(64, 64, q=90)
    for cut in (len(data) - 2, len(data) // 2, 700):
        try:
            fl.debug_jpeg_blob(data[:cut])
        except fl.FanlinError:
            pass


def test_host_decoder_survives_mutated_streams_under_address_sanitizer(tmp_path):
    """The entropy decoder reads bytes fetched from an origin server (src/handler.rs:192-220): tests/tools/fuzz_jpeg_huff.cpp
    is built here with g++ -fsanitize=address,undefined over csrc/fl_jpeghuff.cpp itself (host-only code, no GPU) and fed
    the reference picture plus five sequential, three progressive and four rewritten layouts (4:4:0, RGB, 16-bit quantiser tables,
    optimised Huffman tables), each under 400 truncations / byte flips / stray markers / splices:
    every stream must end in a blob or an error code; any out-of-bounds access or signed overflow aborts the harness."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers")
    csrc = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
    exe = str(tmp_path / "fuzz_jpeg_huff")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
                    os.path.join(ROOT, "tests", "tools", "fuzz_jpeg_huff.cpp"), os.path.join(csrc, "fl_jpeghuff.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    seeds = [LENNA]
    layouts = [(64, 96, 3, 85, 0, 0), (37, 53, 3, 70, 2, 3), (50, 70, 1, 75, 0, 0), (33, 47, 3, 60, 1, 2)]
    for i, (h, w, c, q, sub, rst) in enumerate(layouts):
        p = tmp_path / f"seed{i}.jpg"
        p.write_bytes(make_jpeg(h, w, c, q, sub, rst, index=i))
        seeds.append(str(p))
    b = io.BytesIO()
    Image.fromarray(synth.photo(40, 56, 4, index=9), "CMYK").save(b, "JPEG", quality=85, subsampling=2)
    (tmp_path / "cmyk.jpg").write_bytes(b.getvalue())
    seeds.append(str(tmp_path / "cmyk.jpg"))
    for i, (h, w, c, sub, rst) in enumerate([(48, 64, 3, 2, 0), (37, 53, 3, 0, 4), (40, 40, 1, 0, 0)]):   # progressive: the multi-scan decoder
        kw = dict(quality=80, progressive=True)
        if c == 3:
            kw["subsampling"] = sub
        if rst:
            kw["restart_marker_blocks"] = rst
        (tmp_path / f"prog{i}.jpg").write_bytes(_save(synth.photo(h, w, c, index=20 + i), **kw))
        seeds.append(str(tmp_path / f"prog{i}.jpg"))
    import jpeg_surgery                                           # layouts and tables Pillow's defaults never show (test_jpeg_layouts.py)
    surgery = {"s440": jpeg_surgery.to_440(make_jpeg(40, 56, 3, 85, 1, 0, index=30)), "rgb": jpeg_surgery.to_rgb(make_jpeg(37, 53, 3, 85, 2, 0, index=31)),
               "dqt16": jpeg_surgery.dqt16(make_jpeg(40, 56, 3, 85, 2, 0, index=32)),
               "optimised": _save(synth.uniform(48, 64, 3, index=33), quality=98, subsampling=2, optimize=True)}
    for name, data in surgery.items():
        (tmp_path / f"{name}.jpg").write_bytes(data)
        seeds.append(str(tmp_path / f"{name}.jpg"))
    r = subprocess.run([exe] + seeds, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    decoded, rejected = (int(x) for x in r.stdout.replace(",", "").split() if x.isdigit())
    assert decoded > 300 and rejected > 300, r.stdout             # both outcomes are exercised


# ------------------------------------------------------------------------- oracle vs libjpeg-turbo (the pinned bound) --

def _vs_pillow(oracle, data):
    got = oracle.jpeg_decode(data)
    ref = np.array(Image.open(io.BytesIO(data)))
    if ref.ndim == 2:
        ref = ref[:, :, None]
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    return int(d.max()), float(d.mean())


def test_oracle_decoder_vs_libjpeg_on_the_reference_picture(oracle):
    mx, mean = _vs_pillow(oracle, lenna_bytes())
    assert mx <= 4 and mean < 1.0, (mx, mean)


@pytest.mark.parametrize("case", CASES)
def test_oracle_decoder_vs_libjpeg_on_synthetic_streams(oracle, case):
    h, w, c, q, sub, rst = case
    mx, mean = _vs_pillow(oracle, make_jpeg(h, w, c, q, sub, rst, index=h + w))
    assert mx <= (2 if c == 1 else 4) and mean < 1.0, (case, mx, mean)   # grayscale: only the two integer IDCTs differ


# SHA-256 of the reference's images/lenna.jpg
LENNA_SHA256 = "b92e1e55a91a2d4e0227597d91fa6ccdc05d5a3e436dccc8f6dccd63eae988e7"


def test_committed_lenna_is_the_reference_file():
    import hashlib
    assert hashlib.sha256(lenna_bytes()).hexdigest() == LENNA_SHA256


def make_cmyk_jpeg(h, w, q=90, subsampling=0, ycck=False, icc=None, index=0):
    """A four-component Adobe JPEG (Pillow writes transform 0 = CMYK; the YCCK variant is the same stream with the APP14
    transform byte set to 2, which is all that tells a decoder how to read the samples)."""
    img = synth.photo(h, w, 4, index=index)
    b = io.BytesIO()
    kw = dict(quality=q, subsampling=subsampling)
    if icc:
        kw["icc_profile"] = icc
    Image.fromarray(img, "CMYK").save(b, "JPEG", **kw)
    data = bytearray(b.getvalue())
    if ycck:
        k = data.find(b"Adobe")
        assert k > 0
        data[k + 11] = 2
    return bytes(data)


@pytest.mark.parametrize("sub,ycck", [(0, False), (2, False), (0, True), (2, True)])
def test_four_component_files_host_half_and_oracle(fl, oracle, sub, ycck):
    data = make_cmyk_jpeg(40, 56, subsampling=sub, ycck=ycck, index=sub)
    info = fl.jpeg_info(data)
    assert info["adobe_transform"] == (3 if ycck else 1) and info["components"] == 4
    hdr, got, _ = fl.debug_jpeg_blob(data)
    assert hdr["nc"] == 4 and np.array_equal(got, oracle.jpeg_file_coefficients(data))
    raw = oracle.jpeg_decode(data)
    assert raw.shape == (40, 56, 4) and oracle.jpeg_adobe_transform(data) == (2 if ycck else 0)
    if not ycck:  # Pillow un-inverts Adobe CMYK: its decode is 255 - the raw samples (within the IDCT / up-sampling difference)
        ref = 255 - np.array(Image.open(io.BytesIO(data))).astype(np.int16)
        assert int(np.abs(raw.astype(np.int16) - ref).max()) <= 2


# ----------------------------------------------------------------------------------------------- device half (GPU) --

@pytest.mark.gpu
@pytest.mark.parametrize("sub,ycck", [(0, False), (2, False), (0, True), (2, True)])
def test_cmyk_and_ycck_files_through_the_profile_table(fl, oracle, sub, ycck):
    """convert_jpeg_color_if_needed (handler.rs:398-466) from the file bytes on: decode to raw samples, the YCCK loop when the
    Adobe marker says so, the profile's table, then the pipeline -- one device pass, against the oracle's chain."""
    from conftest import require_device
    require_device()
    clut = np.random.default_rng(21).integers(0, 65536, (17, 17, 17, 17, 3), dtype=np.uint16)
    data = make_cmyk_jpeg(72, 100, subsampling=sub, ycck=ycck, index=5 + sub)
    raw = oracle.jpeg_decode(data)
    cmyk = oracle.ycck_to_cmyk(raw).reshape(raw.shape) if ycck else raw
    rgb = oracle.cmyk_to_rgb(cmyk, clut)
    with fl.State(device=0) as st:
        with pytest.raises(fl.FanlinError) as e:                  # no profile configured: the reference's `None` -> the host decodes
            st.decode_jpeg(data)
        assert e.value.status == fl.ERR_UNSUPPORTED
        st.set_cmyk_clut(clut)
        assert np.array_equal(st.decode_jpeg(data), rgb)
        got = st.process_jpeg_pixels(data, fl.make_params(50, 30))
        assert np.array_equal(got, parity.expected_pixels(fl, st, oracle, rgb, w=50, h=30))
        mime, kind, body = st.process_jpeg(data, "w=64&h=64&quality=80")
        assert kind == fl.RESULT_JPEG_STREAM and body == oracle.jpeg_encode(parity.expected_pixels(fl, st, oracle, rgb, w=64, h=64), 80)
        assert st.process_batch([data, rgb], [fl.make_params(50, 30)] * 2)[0].tobytes() == got.tobytes()


@pytest.mark.gpu
def test_embedded_profile_of_a_cmyk_file(fl, oracle):
    import lcms2_lib
    import synth_icc
    from conftest import require_device
    require_device()
    if lcms2_lib.load() is None:
        pytest.skip("liblcms2 not installed")
    icc = synth_icc.cmyk_profile()
    other = np.random.default_rng(22).integers(0, 65536, (17, 17, 17, 17, 3), dtype=np.uint16)
    data = make_cmyk_jpeg(48, 64, icc=icc, index=9)
    assert fl.jpeg_info(data)["has_icc_profile"] == 1
    raw = oracle.jpeg_decode(data)
    with fl.State(device=0, use_embedded_profile=True) as st:
        st.set_cmyk_clut(other)                                   # the configured profile is NOT what converts this file ...
        want = lcms2_lib.Cmyk2Rgb(icc).convert(raw.reshape(-1, 4)).reshape(48, 64, 3)
        assert np.array_equal(st.decode_jpeg(data), want)         # ... its own profile is (handler.rs:446-449), bit-exact vs liblcms2
    with fl.State(device=0) as st:                                # use_embedded_profile = false: the configured one
        st.set_cmyk_clut(other)
        assert np.array_equal(st.decode_jpeg(data), oracle.cmyk_to_rgb(raw, other))


@pytest.mark.gpu
def test_a_hostile_header_cannot_reserve_gigabytes(fl, gpu_state):
    """A file's own SOF header decides how much staging memory a JPEG source needs, so it is checked before anything is
    reserved: a small file that announces 26,000 x 26,000 pixels is malformed (too short for that many blocks), one that
    announces more than the reference decoder's 512 MiB limit (image::Limits::default, handler.rs:205-220) is unsupported --
    through the queue (flgpu_transform) and through the batch call alike, and the context keeps working."""
    data = bytearray(make_jpeg(64, 64, 3, 85, 2, 0, index=3))
    sof = data.find(b"\xff\xc0")
    assert sof > 0

    def with_size(h, w):
        d = bytearray(data)
        d[sof + 5:sof + 7] = h.to_bytes(2, "big")
        d[sof + 7:sof + 9] = w.to_bytes(2, "big")
        return bytes(d)

    before = gpu_state.stats()
    for h, w, status in ((26000, 26000, fl.ERR_UNSUPPORTED), (12000, 12000, fl.ERR_INVALID_ARG), (20000, 30000, fl.ERR_UNSUPPORTED)):
        bad = with_size(h, w)
        assert fl.jpeg_info(bad)["width"] == w
        with pytest.raises(fl.FanlinError) as e:
            gpu_state.process_jpeg_pixels(bad, fl.make_params(300, 200))
        assert e.value.status == status, (h, w, e.value.status)
        with pytest.raises(fl.FanlinError) as e:
            gpu_state.process_batch([bad], [fl.make_params(300, 200)])
        assert e.value.status == status
    good = gpu_state.process_jpeg_pixels(bytes(data), fl.make_params(32, 32))
    assert good.shape[:2] == (32, 32)


@pytest.mark.gpu
def test_more_embedded_profiles_in_one_batch_than_the_table_cache_holds(fl, oracle):
    """A batch selects the tables of all its pictures before it launches their conversions, and the cache of baked embedded
    profiles holds 8: with 11 distinct profiles in ONE batch no table handed out for an earlier picture may be evicted (and
    freed) by a later one.  Every picture must equal what liblcms2 makes of its own profile; the same batch again (cache
    trimmed in between) and each file alone must give the same bytes."""
    import lcms2_lib
    import synth_icc
    from conftest import require_device
    require_device()
    if lcms2_lib.load() is None:
        pytest.skip("liblcms2 not installed")
    iccs = [synth_icc.cmyk_profile(seed=40 + k) for k in range(11)]
    assert len({bytes(i) for i in iccs}) == 11
    files = [make_cmyk_jpeg(40, 56, icc=iccs[k], index=60 + k) for k in range(11)]
    wants = [lcms2_lib.Cmyk2Rgb(iccs[k]).convert(oracle.jpeg_decode(files[k]).reshape(-1, 4)).reshape(40, 56, 3) for k in range(11)]
    with fl.State(device=0, use_embedded_profile=True) as st:
        st.set_cmyk_clut(np.random.default_rng(23).integers(0, 65536, (17, 17, 17, 17, 3), dtype=np.uint16))
        p = fl.make_params(28, 20)
        alone = [st.process_pixels(wants[k], p) for k in range(11)]  # the pipeline on liblcms2's pixels
        for rep in range(2):
            outs = st.process_batch(files, [p] * 11)
            for k in range(11):
                assert np.array_equal(outs[k], alone[k]), (rep, k)
        assert st.stats()["cmyk_tables_baked"] >= 11
        for k in (0, 5, 10):
            assert np.array_equal(st.decode_jpeg(files[k]), wants[k])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_device_decode_is_bit_identical_to_the_oracle(fl, gpu_state, oracle, case):
    h, w, c, q, sub, rst = case
    data = make_jpeg(h, w, c, q, sub, rst, index=h + w)
    assert np.array_equal(gpu_state.decode_jpeg(data), oracle.jpeg_decode(data))


@pytest.mark.gpu
def test_progressive_files_on_the_device(fl, gpu_state, oracle):
    """A progressive file decodes to the very pixels of its baseline twin (same coefficients, same device kernels): the
    reference picture re-saved progressively by Pillow -- and the whole request from those bytes on -- against the oracle
    decoder on the baseline form."""
    src = np.array(Image.open(LENNA).convert("RGB"))
    for sub, q in ((2, 85), (0, 92), (1, 70)):
        prog, base = _save(src, progressive=True, quality=q, subsampling=sub), _save(src, quality=q, subsampling=sub)
        assert fl.jpeg_info(prog)["progressive"] == 1
        want = oracle.jpeg_decode(base)
        assert np.array_equal(gpu_state.decode_jpeg(prog), want)
        mime, kind, body = gpu_state.process_jpeg(prog, "w=300&h=200")
        assert kind == fl.RESULT_JPEG_STREAM and body == gpu_state.process_jpeg(base, "w=300&h=200")[2]
        assert body == oracle.jpeg_encode(parity.expected_pixels(fl, gpu_state, oracle, want, w=300, h=200), 75)
    grey = synth.photo(333, 517, 1, index=4)
    assert np.array_equal(gpu_state.decode_jpeg(_save(grey, progressive=True, quality=60)), oracle.jpeg_decode(_save(grey, quality=60)))


@pytest.mark.gpu
def test_device_decode_of_the_reference_picture_and_config0(fl, gpu_state, oracle):
    data = lenna_bytes()
    want = oracle.jpeg_decode(data)
    assert np.array_equal(gpu_state.decode_jpeg(data), want)
    # BASELINE config 0: lenna.jpg -> w=300&h=200, the whole request from the file bytes on, in one call
    mime, kind, body = gpu_state.process_jpeg(data, "w=300&h=200")
    px = parity.expected_pixels(fl, gpu_state, oracle, want, w=300, h=200)
    assert mime == "image/jpeg" and kind == fl.RESULT_JPEG_STREAM and body == oracle.jpeg_encode(px, 75)
    assert px.shape == (200, 300, 4) and tuple(px[0, 0]) == (32, 32, 32, 255) and tuple(px[0, 49]) == (32, 32, 32, 255)   # 200x200 at x offset 50
    mime, kind, planes = gpu_state.process_jpeg(data, "w=300&h=200&webp=true&quality=20", fl.Format.from_accept_header("image/webp"))
    assert mime == "image/webp" and kind == fl.RESULT_WEBP_PLANES and planes.y.shape == (200, 300)
    assert gpu_state.process_jpeg(data, "quality=80")[1] == fl.RESULT_AS_IS            # as_is never decodes (handler.rs:202-204)
    st = gpu_state.stats()
    assert st["jpeg_sources"] >= 3 and 0 < st["jpeg_upload_bytes"] < st["jpeg_sources"] * 1.2 * 512 * 512 * 3   # near-lossless file: see the CPU test


@pytest.mark.gpu
def test_jpeg_sources_through_the_queue_and_batches(fl, gpu_state, oracle):
    import threading
    files = [make_jpeg(120 + 16 * i, 200 + 8 * i, 3 if i % 4 else 1, 60 + 5 * i, i % 3, (i % 2) * 4, index=300 + i) for i in range(8)]
    decoded = [oracle.jpeg_decode(f) for f in files]
    ps = [fl.make_params(64 + i, 48, crop=bool(i % 2), grayscale=bool(i == 3), front_end=fl.FE_JPEG if i % 3 == 0 else fl.FE_NONE, quality=70) for i in range(8)]
    want = [gpu_state.process_pixels(decoded[i], ps[i]) for i in range(8)]             # the pixel-source path, already checked against the oracle elsewhere
    got = gpu_state.process_batch(files, ps)
    for a, b in zip(got, want):
        assert (a == b) if isinstance(a, bytes) else np.array_equal(a, b)
    mixed = gpu_state.process_batch([files[0], decoded[1], files[2]], ps[:3])          # JPEG and pixel sources in one batch
    for a, b in zip(mixed, want[:3]):
        assert (a == b) if isinstance(a, bytes) else np.array_equal(a, b)
    out = [None] * 64
    def worker(t):
        for i in range(t, 64, 8):
            out[i] = gpu_state.process_jpeg_pixels(files[i % 8], ps[i % 8])
    ts = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for i in range(64):
        b = want[i % 8]
        assert (out[i] == b) if isinstance(b, bytes) else np.array_equal(out[i], b)


@pytest.mark.gpu
def test_one_decoder_at_a_time_serves_every_caller(fl, oracle):
    """flgpu_config.decode_threads bounds how many callers run the host Huffman decoder at once; with 1 the sixteen callers here take
    turns -- nobody is dropped, nobody waits for ever, and the results are those of the unbounded context."""
    import threading
    files = [make_jpeg(96 + 8 * i, 128 + 8 * i, 3, 75, i % 3, 0, index=500 + i) for i in range(4)]
    p = fl.make_params(40, 30)
    with fl.State(device=0, decode_threads=1) as st:
        want = [st.process_pixels(oracle.jpeg_decode(f), p) for f in files]
        out = [None] * 64
        def worker(t):
            for i in range(t, 64, 16):
                out[i] = st.process_jpeg_pixels(files[i % 4], p)
        ts = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
        [t.start() for t in ts]
        [t.join(timeout=120) for t in ts]
        assert not any(t.is_alive() for t in ts)
        for i in range(64):
            assert np.array_equal(out[i], want[i % 4])


@pytest.mark.gpu
def test_exif_orientation_is_applied_by_process_jpeg(fl, gpu_state, oracle):
    data = make_jpeg(90, 60, q=92, exif_orientation=6, index=77)
    px = oracle.jpeg_decode(data)
    mime, kind, got = gpu_state.process_jpeg(data, "w=40&h=40&webp=true&quality=100", fl.Format.from_accept_header("image/webp"))
    assert kind == fl.RESULT_PIXELS                               # lossless WebP: pixels for the host encoder
    want = parity.expected_pixels(fl, gpu_state, oracle, px, w=40, h=40, orientation=6)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_unsupported_jpeg_sources_are_refused_not_mangled(fl, gpu_state):
    data = bytearray(make_jpeg(40, 50))
    data[data.find(b"\xff\xc0") + 1] = 0xC9                      # SOF9: arithmetic coding -- the host keeps its own decoder for it
    data = bytes(data)
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.decode_jpeg(data)
    assert e.value.status == fl.ERR_UNSUPPORTED
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_jpeg(data, "w=30&h=30")
    assert e.value.status == fl.ERR_UNSUPPORTED
    assert gpu_state.process_jpeg(data, "rgb=1,2,3")[1] == fl.RESULT_AS_IS


# ---------------------------------------------------------------------------- entropy decoding on the device (round 4) --

DEVICE_HUFFMAN_FILES = [
    # h, w, c, quality, subsampling, dist
    (1080, 1920, 3, 85, 2, "photo"),     # the bench's JPEG sources: 4:2:0, ~300 KB
    (1080, 1920, 3, 95, 0, "uniform"),   # noise at high quality: long code words, the slow path of every table
    (720, 1280, 3, 5, 2, "photo"),       # almost nothing but end-of-block codes
    (1081, 1921, 3, 75, 1, "photo"),     # 4:2:2, sizes that are no multiple of the MCU
    (1000, 1500, 1, 80, 0, "photo"),     # one component: one block per MCU
    (64, 96, 3, 85, 2, "photo"), (37, 53, 3, 70, 0, "photo"), (8, 8, 3, 90, 0, "photo"), (1, 1, 3, 90, 2, "photo"), (9, 300, 3, 95, 2, "uniform"),
]
# round 5: restart intervals on the device -- h, w, c, quality, subsampling, restart interval in blocks (= MCUs for Pillow's writer)
DEVICE_HUFFMAN_RESTART_FILES = [
    (1080, 1920, 3, 85, 2, 120),    # one interval per MCU row of a 4:2:0 picture: what cameras write
    (1080, 1920, 3, 85, 2, 7),      # short intervals that start anywhere in a row (~2,300 bits each: several per 1024-bit subsequence pair)
    (720, 1280, 3, 92, 0, 1),       # an interval per MCU: 14,400 of them, an interval start in almost every subsequence
    (1000, 1500, 1, 80, 0, 33),     # one component
    (1081, 1921, 3, 60, 1, 50),     # 4:2:2, partial MCUs at the edges
    (64, 96, 3, 85, 2, 5), (37, 53, 3, 70, 0, 2), (200, 301, 3, 40, 0, 3),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEVICE_HUFFMAN_FILES)
def test_device_entropy_decoder_reads_the_host_decoders_coefficients(fl, gpu_state, oracle, monkeypatch, case):
    """Sequential one-scan files without restart intervals are Huffman-decoded ON THE DEVICE (csrc/fl_jpeghuff_dev.hip: speculative
    subsequence decoding, re-synchronisation rounds, prefix sums, write pass): the decoded picture must be the oracle decoder's, bit
    for bit -- i.e. every coefficient the host decoder would have read -- and the statistics must say the device did the decoding."""
    h, w, c, q, sub, dist = case
    gpu_state.debug_set("device_huffman_min_bytes", 0)
    gpu_state.debug_set("device_huffman_always", 1)   # (by default a lone request is decoded by its own thread: a CPU is idle)
    img = getattr(synth, dist)(h, w, c, index=h + q)
    data = _save(img, quality=q, **({"subsampling": sub} if c == 3 else {}))
    s0 = gpu_state.stats()
    got = gpu_state.decode_jpeg(data)
    s1 = gpu_state.stats()
    assert s1["jpeg_device_huffman"] == s0["jpeg_device_huffman"] + 1 and s1["jpeg_device_huffman_retries"] == s0["jpeg_device_huffman_retries"]
    assert np.array_equal(got, oracle.jpeg_decode(data))
    gpu_state.debug_set("host_huffman", 1)                     # the host decoder stays selectable, and agrees
    assert np.array_equal(gpu_state.decode_jpeg(data), got)
    assert gpu_state.stats()["jpeg_device_huffman"] == s1["jpeg_device_huffman"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEVICE_HUFFMAN_RESTART_FILES)
def test_device_entropy_decoder_takes_restart_intervals(fl, gpu_state, oracle, case):
    """Files with restart intervals (DRI + RSTn markers; round 5): the staging step takes the markers out of the segment and records where
    the intervals start, the device's walks step over the padding in front of an interval start, begin the DC predictors at zero there
    and check the block counter -- and fall into step there for good, if they were out of step.  Pixels are the oracle decoder's, bit
    for bit, and the device did the decoding."""
    h, w, c, q, sub, rst = case
    gpu_state.debug_set("device_huffman_min_bytes", 0)
    gpu_state.debug_set("device_huffman_always", 1)
    data = make_jpeg(h, w, c, q, sub, rst, index=h + rst)
    assert fl.jpeg_info(data)["restart_interval"] == rst
    s0 = gpu_state.stats()
    got = gpu_state.decode_jpeg(data)
    s1 = gpu_state.stats()
    assert s1["jpeg_device_huffman"] == s0["jpeg_device_huffman"] + 1 and s1["jpeg_device_huffman_retries"] == s0["jpeg_device_huffman_retries"]
    assert np.array_equal(got, oracle.jpeg_decode(data))


@pytest.mark.gpu
@pytest.mark.parametrize("c,sub", [(3, 2), (3, 0), (1, 0)])
def test_one_colour_pictures_stay_with_the_host_decoder(fl, gpu_state, oracle, c, sub):
    """A picture of one colour is a periodic stream ("DC difference 0, end of block", ~5 bits per block): a decoder started at a wrong
    bit falls into a shifted parse that is as valid as the true one, so the device's subsequences never fall into step.  The staging step
    (csrc/fl_jpeghuff.cpp jpeg_entropy_stage) leaves files below 7 bits per block to the host decoder instead of letting them end in the
    host retry; the pixels are the oracle decoder's either way."""
    gpu_state.debug_set("device_huffman_min_bytes", 0)
    gpu_state.debug_set("device_huffman_always", 1)
    img = np.full((1000, 1400, c), 77, np.uint8)
    img[..., 0] = 190
    data = _save(img, quality=85, **({"subsampling": sub} if c == 3 else {}))
    s0 = gpu_state.stats()
    got = gpu_state.decode_jpeg(data)
    s1 = gpu_state.stats()
    assert s1["jpeg_device_huffman"] == s0["jpeg_device_huffman"] and s1["jpeg_device_huffman_retries"] == s0["jpeg_device_huffman_retries"]
    assert np.array_equal(got, oracle.jpeg_decode(data))


@pytest.mark.gpu
def test_device_entropy_decoder_in_batches_and_whole_requests(fl, gpu_state, oracle, monkeypatch):
    gpu_state.debug_set("device_huffman_min_bytes", 0)
    gpu_state.debug_set("device_huffman_always", 1)   # (by default a lone request is decoded by its own thread: a CPU is idle)
    files = [make_jpeg(360 + 8 * k, 640 - 16 * k, 3, 60 + 5 * k, k % 3, 0, index=40 + k) for k in range(6)]
    files.append(make_jpeg(200, 300, 3, 80, 2, 5, index=9))           # a restart interval (round 5: on the device as well, in the same launches)
    files.append(_save(synth.photo(240, 320, 3, index=3), progressive=True, quality=80))   # progressive: this one stays with the host decoder
    p = fl.make_params(150, 100)
    before = gpu_state.stats()["jpeg_device_huffman"]
    outs = gpu_state.process_batch(files, [p] * len(files))            # flgpu_transform_batch: one set of launches for all eight
    assert gpu_state.stats()["jpeg_device_huffman"] - before == 7
    gpu_state.debug_set("host_huffman", 1)
    host = gpu_state.process_batch(files, [p] * len(files))
    gpu_state.debug_set("host_huffman", 0)
    for f, o, hh in zip(files, outs, host):
        assert np.array_equal(o, hh)
        if not fl.jpeg_info(f)["progressive"]:
            assert np.array_equal(o, parity.expected_pixels(fl, gpu_state, oracle, oracle.jpeg_decode(f), w=150, h=100))
    # the whole request of the metric from file bytes: the same stream whichever side decodes the entropy-coded segment
    big = make_jpeg(1080, 1920, 3, 85, 2, 0, index=5)
    a = gpu_state.process_jpeg(big, "w=300&h=200")
    gpu_state.debug_set("host_huffman", 1)
    b = gpu_state.process_jpeg(big, "w=300&h=200")
    assert a[1] == fl.RESULT_JPEG_STREAM and a[2] == b[2]


@pytest.mark.gpu
def test_device_entropy_decoder_on_broken_streams(fl, gpu_state, monkeypatch):
    """Mutated and truncated segments: the device decoder reports an invalid code word (or a chain of states that did not settle)
    and the request is decoded on the host once more -- which returns an error or a picture, as before; never a crash or a hang."""
    gpu_state.debug_set("device_huffman_min_bytes", 0)
    gpu_state.debug_set("device_huffman_always", 1)   # (by default a lone request is decoded by its own thread: a CPU is idle)
    rng = np.random.default_rng(11)
    data = bytearray(make_jpeg(240, 320, 3, 85, 2, 0, index=21))
    sos = data.find(b"\xff\xda") + 14

    def outcome(blob):
        """(status, pixels) of one file with the switches as they are."""
        try:
            return 0, gpu_state.decode_jpeg(blob)
        except fl.FanlinError as e:
            assert e.status in (fl.ERR_INVALID_ARG, fl.ERR_UNSUPPORTED)
            return e.status, None

    def same_on_both_sides(blob, what):
        """Which side decodes the entropy-coded segment depends on how busy the host is: a broken file must come out the same either
        way -- the same error, or the same pixels (an HTTP cache in front of the service must not see the difference)."""
        dev = outcome(blob)
        with gpu_state.switches(host_huffman=1):
            host = outcome(blob)
        assert dev[0] == host[0], (what, dev[0], host[0])
        if dev[1] is not None:
            assert np.array_equal(dev[1], host[1]), what

    for trial in range(40):
        d = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            d[int(rng.integers(sos, len(d) - 2))] = int(rng.integers(0, 255))    # (255 would start a marker: a different path)
        same_on_both_sides(bytes(d), ("mutation", trial))
    for cut in (len(data) - 2, len(data) // 2, sos + 40):
        same_on_both_sides(bytes(data[:cut]), ("cut", cut))
    # cuts at and around whole subsequences of the segment (kJhSubBits = 1024 bits = 128 bytes): the last walk then ends at the
    # segment's end without meeting the padding -- no invalid code word, but blocks are missing
    for nsub in (3, 8, 17, 40):
        for delta in (-1, 0, 1, 2):
            same_on_both_sides(bytes(data[:sos + 128 * nsub + delta]) + b"\xff\xd9", ("cut at subsequence", nsub, delta))
    # a file with restart intervals (round 5: on the device): mutations inside the intervals, markers damaged, removed and doubled, cuts
    rdata = bytearray(make_jpeg(240, 320, 3, 85, 2, 4, index=22))
    rsos = rdata.find(b"\xff\xda") + 14
    for trial in range(30):
        d = bytearray(rdata)
        for _ in range(int(rng.integers(1, 4))):
            d[int(rng.integers(rsos, len(d) - 2))] = int(rng.integers(0, 255))
        same_on_both_sides(bytes(d), ("restart file, mutation", trial))
    marks = [i for i in range(rsos, len(rdata) - 1) if rdata[i] == 0xFF and 0xD0 <= rdata[i + 1] <= 0xD7]
    assert len(marks) > 10
    for trial in range(12):
        d = bytearray(rdata)
        m = marks[int(rng.integers(0, len(marks)))]
        kind = trial % 4
        if kind == 0: del d[m:m + 2]                                     # a marker missing
        elif kind == 1: d[m + 1] = 0xD0 + (d[m + 1] - 0xD0 + 3) % 8        # out of sequence
        elif kind == 2: d[m:m] = d[m:m + 2]                              # doubled
        else: d[m - 1] ^= 0x10                                           # the byte in front of it (padding or the last code words)
        same_on_both_sides(bytes(d), ("restart file, marker", trial, kind))
    for cut in (len(rdata) // 2, marks[5] + 1, marks[7] + 2, marks[9]):
        same_on_both_sides(bytes(rdata[:cut]) + b"\xff\xd9", ("restart file, cut", cut))
    good = gpu_state.decode_jpeg(bytes(data))                                   # the context is fine afterwards
    assert good.shape == (240, 320, 3)
