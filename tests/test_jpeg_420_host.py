"""FLGPU_FEO_JPEG_420 / FLGPU_ENCODE_JPEG_420, the host half: the constants and the unchanged structs, the plan, the mapping of the accept
bit, and the rule restated in numpy (tests/jpeg_420_model.py) judged on the corpus (tests/jpeg_420_cases.py) by Pillow's decoder, by the
oracle's entropy decoder and against libjpeg's own 4:2:0 files.  No GPU."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_420_cases as cases
import jpeg_420_model as m
import jpeg_opt_model as jm
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Against libjpeg through Pillow on the same pixels, measured with the model on LIBJPEG_CASES on the CPU; every pair is in DESIGN.md
# section 4.  Size: len(model 4:2:0) / len(oracle.jpeg_encode) minus Pillow's subsampling=2 / subsampling=0.  Quality: the RGB PSNR of
# Pillow's decode of libjpeg's 4:2:0 file against the source minus that of the model's file.  The two coders hold different coefficients
# (the crate's colour rounding, integer DCT and quantiser rounding against libjpeg's, and libjpeg's alternating bias in the average), so
# the figures are near, not equal.  The margins are the largest excess rounded up to the next 0.005 and the largest deficit rounded up
# to the next 0.05 dB.  Pictures of one MCU stay out: at 1 x 1 the two coders' colour rounding is all there is.
LIBJPEG_CASES = [(h, w, q) for (h, w) in ((200, 300), (61, 83)) for q in (1, 30, 75, 95, 100)]
LIBJPEG_LARGEST_EXCESS = 0.0194    # 83 x 61 at quality 75: 0.7650 (1,595 of 2,085 bytes) against 0.7456 (1,574 of 2,111)
LIBJPEG_SIZE_MARGIN = 0.020
LIBJPEG_LARGEST_DEFICIT = 0.389    # 83 x 61 at quality 100: 35.84 dB against 36.23 dB
LIBJPEG_PSNR_MARGIN = 0.40


# ----------------------------------------------------------------------------------------------------------- the ABI --

def test_the_constants_the_headers_and_the_shim(fl, tmp_path):
    assert fl.ENCODE_JPEG_420 == 0x200000 and fl.FEO_JPEG_420 == 8 and fl.load_library().flgpu_abi_version() == 6
    assert C.sizeof(fl.flgpu_params) == 28 and fl.flgpu_params.reserved.offset == 26 and C.sizeof(fl.flgpu_plan) == 96
    others = (fl.ACCEPT_WEBP, fl.ACCEPT_AVIF, fl.ENCODE_PNG, fl.DECODE_PNG_ADAM7, fl.DECODE_PNG_INFLATE, fl.ENCODE_WEBP_LOSSLESS, fl.ENCODE_GIF, fl.ENCODE_GIF_QUANTIZE,
              fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER, fl.ENCODE_WEBP_LOSSY_ALPHA,
              fl.ENCODE_WEBP_LOSSY_SEGMENTS, fl.ENCODE_JPEG_OPTIMIZE)
    assert not any(fl.ENCODE_JPEG_420 & b for b in others)
    assert tuple(fl.make_params().reserved) == (0, 0) and tuple(fl.make_params(jpeg_420=True).reserved) == (8, 0)
    assert tuple(fl.make_params(jpeg_420=True, jpeg_optimize=True, segments=True, alpha_vp8l=True).reserved) == (15, 0)
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert "#define FLGPU_ENCODE_JPEG_420 0x200000u" in header and "#define FLGPU_FEO_JPEG_420 8u" in header and "#define FLGPU_ABI_VERSION 6" in header
    assert "void encode_jpeg_420() { flags_ |= FLGPU_ENCODE_JPEG_420; }" in open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    shim = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    assert "ENCODE_JPEG_420: u32 = 0x200000" in shim and "FEO_JPEG_420: u8 = 8" in shim
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fanlin_gpu.h"\nint main(void) { printf("%zu %zu %zu %u %u %d\\n", sizeof(flgpu_params), '
                   'sizeof(flgpu_plan), offsetof(flgpu_params, options), FLGPU_FEO_JPEG_420, FLGPU_ENCODE_JPEG_420, FLGPU_ABI_VERSION); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["28", "96", "26", "8", str(0x200000), "6"]


def test_the_cpp_mirror_sets_the_flag(fl, tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include <cstdio>\n#include "fanlin_gpu.hpp"\nint main() { fanlin::content::Format f; f.encode_jpeg_optimize(); const unsigned before = f.flags(); '
                   'f.encode_jpeg_420(); std::printf("%u %u\\n", before, f.flags()); return 0; }\n')
    exe, libdir = str(tmp_path / "mirror"), os.path.dirname(fl.LIB_PATH)
    subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", str(src), "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lfanlin_gpu",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    before, after = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert before == fl.ENCODE_JPEG_OPTIMIZE and after == before | fl.ENCODE_JPEG_420


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (16, 16), (17, 17), (300, 200)])
def test_the_plan_with_the_option(fl, w, h):
    for c in (1, 3, 4):
        for optimize in (False, True):
            plan = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_JPEG, jpeg_420=True, jpeg_optimize=optimize), w, h, c)
            pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
            assert (plan.out_w, plan.out_h, plan.out_c) == (w, h, c)
            assert (plan.plane_w, plan.plane_h, plan.chroma_w, plan.chroma_h) == (pw, ph, pw // 2, ph // 2)
            assert plan.out_bytes == 1024 + 3 * pw * ph // 2
            assert plan.max_out_bytes == 1024 + 2 * 208 * 6 * (pw // 16) * (ph // 16)
    one = fl.plan_output(fl.make_params(front_end=fl.FE_JPEG), 8, 8, 3).max_out_bytes
    assert fl.plan_output(fl.make_params(front_end=fl.FE_JPEG, jpeg_420=True), 8, 8, 3).max_out_bytes == 1024 + 2 * 208 * 6 > one == 1024 + 2 * 208 * 3


def test_every_other_front_end_ignores_the_option(fl):
    for fe in (fl.FE_JFIF444, fl.FE_PNG, fl.FE_WEBP420, fl.FE_NONE, fl.FE_WEBP_LOSSLESS, fl.FE_WEBP_LOSSY, fl.FE_WEBP_LOSSY_I4):
        for (w, h, c) in ((300, 200, 4), (17, 9, 3)):
            a, b = fl.plan_output(fl.make_params(quality=75, front_end=fe), w, h, c), fl.plan_output(fl.make_params(quality=75, front_end=fe, jpeg_420=True), w, h, c)
            assert bytes(a) == bytes(b), fe
    a, b = fl.plan_output(fl.make_params(front_end=fl.FE_JPEG), 300, 200, 4), fl.plan_output(fl.make_params(front_end=fl.FE_JPEG, jpeg_optimize=True), 300, 200, 4)
    assert bytes(a) == bytes(b) and (a.plane_w, a.plane_h, a.max_out_bytes) == (304, 200, 1024 + 2 * 208 * 3 * 38 * 25), "without the bit the plan is what it was"


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=3):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


def test_the_mapping_of_the_accept_bit(fl):
    """The option is set exactly where flgpu_params_from_query chooses FLGPU_FE_JPEG, alone and beside FLGPU_ENCODE_JPEG_OPTIMIZE."""
    new = fl.ENCODE_JPEG_420

    def fields(p):
        return [getattr(p, n) for n, _ in fl.flgpu_params._fields_ if n != "reserved"]
    every = (fl.ENCODE_PNG | fl.ENCODE_WEBP_LOSSLESS | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS | fl.ENCODE_WEBP_LOSSY_FILTER
             | fl.ENCODE_WEBP_LOSSY_ALPHA | fl.ENCODE_WEBP_LOSSY_SEGMENTS | fl.ENCODE_GIF | fl.ENCODE_GIF_QUANTIZE)
    for query in ("w=300&h=200", "w=300&h=200&quality=30", "w=300&h=200&webp=true&quality=75", "w=300&h=200&avif=true", "blur=12", "w=300&h=200&webp=true&quality=100"):
        q = fl.Query.parse(query)
        for accept in (0, fl.ACCEPT_WEBP, fl.ACCEPT_AVIF, fl.ACCEPT_WEBP | fl.ACCEPT_AVIF):
            for extra in (0, every, fl.ENCODE_JPEG_OPTIMIZE):
                for is_jpeg in (0, 1, 2):
                    flags = accept | extra
                    without, fmt0 = q.to_params(fl.Format(flags), is_jpeg)
                    with_bit, fmt1 = q.to_params(fl.Format(flags | new), is_jpeg)
                    assert fields(without) == fields(with_bit) and fmt0 == fmt1 and without.reserved[1] == with_bit.reserved[1] == 0
                    assert without.reserved[0] & fl.FEO_JPEG_420 == 0 and with_bit.reserved[0] & ~fl.FEO_JPEG_420 == without.reserved[0]
                    want = with_bit.front_end == fl.FE_JPEG
                    assert want == (is_jpeg == 2 and fmt1 == fl.OUT_KEEP), (query, hex(flags), is_jpeg)
                    assert bool(with_bit.reserved[0] & fl.FEO_JPEG_420) == want, (query, hex(flags), is_jpeg)
                    assert bool(with_bit.reserved[0] & fl.FEO_JPEG_OPTIMIZE) == (want and extra == fl.ENCODE_JPEG_OPTIMIZE)
                for fmt in (fl.IN_PNG, fl.IN_WEBP, fl.IN_OTHER, fl.IN_GIF_FRAME):
                    a, b = _plan(fl, query, accept | extra, fmt), _plan(fl, query, accept | extra | new, fmt)
                    assert a[:2] == b[:2] and bytes(a[2]) == bytes(b[2]), (query, fmt)
    # webp=true with WebP accepted, a PNG input, as_is: not set (the plan is the one without the bit)
    for query, flags, fmt in (("w=300&h=200&webp=true", fl.ACCEPT_WEBP, fl.IN_JPEG), ("w=300&h=200", fl.ENCODE_PNG, fl.IN_PNG), ("", 0, fl.IN_JPEG)):
        a, b = _plan(fl, query, flags, fmt), _plan(fl, query, flags | new, fmt)
        assert a[:2] == b[:2] and bytes(a[2]) == bytes(b[2]), query
    rc, kind, _ = _plan(fl, "", new, fl.IN_JPEG)
    assert rc == fl.OK and kind == fl.RESULT_AS_IS
    # a JPEG that stays JPEG: the stream, planned 4:2:0
    rc, kind, plan = _plan(fl, "w=300&h=200", new, fl.IN_JPEG)
    assert rc == fl.OK and kind == fl.RESULT_JPEG_STREAM and (plan.plane_w, plan.plane_h, plan.chroma_w, plan.chroma_h) == (304, 208, 152, 104)
    assert plan.max_out_bytes == 1024 + 2 * 208 * 6 * 19 * 13


# ----------------------------------------------------------------------------------------------------------- the model --

def _open(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def test_the_corpus_reaches_what_it_is_there_for(oracle):
    cases.check_conditions(oracle)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_corpus_file_is_a_valid_420_file_of_the_models_coefficients(fl, oracle, name):
    from PIL import JpegImagePlugin
    img, q = cases.get(name)
    h, w, c = img.shape
    plain, info0 = cases.model(oracle, name)
    for optimize in (False, True):
        data, info = cases.model(oracle, name, optimize)
        im = _open(data)
        assert im.size == (w, h) and JpegImagePlugin.get_sampling(im) == 2
        plan = fl.plan_output(fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_420=True, jpeg_optimize=optimize), w, h, c)
        assert len(data) <= plan.max_out_bytes
        segs = jm.segments(data)
        assert [mk for mk, _ in segs] == [0xE0, 0xC0, 0xDB, 0xDB, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA] and data[-2:] == b"\xff\xd9"
        assert segs[1][1] == bytes([8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
        # an independent reading of the stream: the oracle's entropy decoder lists the blocks per component, in raster order of the padded plane
        got = oracle.jpeg_file_coefficients(data)
        want = m.file_order(info["coef"], w, h)
        assert got.shape == want.shape and np.array_equal(got, want)
        if optimize:
            print(name, len(plain), "->", len(data), "optimized" if info["optimized"] else "standard")
            assert (len(data) < len(plain)) if info["optimized"] else (data == plain)
            assert np.array_equal(np.asarray(im), np.asarray(_open(plain)))
            assert cases.model(oracle, name, True, True)[0] == plain, "the fallback is the 4:2:0 Annex K file"
    # everything but the one sampling byte of the header is FE_JPEG's
    hd = oracle.jpeg_header(w, h, q)
    assert plain[:31] == hd[:31] and plain[31] == 0x22 and hd[31] == 0x11 and plain[32:jm.STD_HEADER_BYTES] == hd[32:]


def test_the_sizes_the_issue_states(oracle):
    img = synth.photo(200, 300, 3, index=7)
    got = [(len(oracle.jpeg_encode(img, q)), len(m.encode(oracle, img, q)[0])) for q in (1, 30, 75, 95, 100)]
    assert got == [(2450, 1751), (5955, 4357), (11158, 8362), (44139, 24869), (105613, 49668)]


def _psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_size_and_quality_against_libjpegs_420(oracle):
    from PIL import Image
    excess = deficit = -1.0
    for h, w, q in LIBJPEG_CASES:
        img = synth.photo(h, w, 3, index=7)
        ours = m.encode(oracle, img, q)[0]
        ratio = len(ours) / len(oracle.jpeg_encode(img, q))
        files = []
        for subsampling in (2, 0):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=subsampling)
            files.append(buf.getvalue())
        theirs = len(files[0]) / len(files[1])
        p_ours, p_theirs = _psnr(np.asarray(_open(ours).convert("RGB")), img), _psnr(np.asarray(_open(files[0]).convert("RGB")), img)
        print(f"{w}x{h} q{q}: ours {ratio:.4f} libjpeg {theirs:.4f} excess {ratio - theirs:+.4f}; PSNR ours {p_ours:.2f} libjpeg {p_theirs:.2f} deficit {p_theirs - p_ours:+.3f}")
        excess, deficit = max(excess, ratio - theirs), max(deficit, p_theirs - p_ours)
        assert ratio <= theirs + LIBJPEG_SIZE_MARGIN, (h, w, q)
        assert p_ours >= p_theirs - LIBJPEG_PSNR_MARGIN, (h, w, q)
    assert abs(excess - LIBJPEG_LARGEST_EXCESS) < 0.0005 and abs(deficit - LIBJPEG_LARGEST_DEFICIT) < 0.005, f"the recorded figures are stale: {excess:.4f} {deficit:.3f}"
