"""FLGPU_FEO_JPEG_PROGRESSIVE / FLGPU_ENCODE_JPEG_PROGRESSIVE, the host half: the constants and the unchanged struct, the mapping of the
accept bit, the restated coder (tests/jpeg_prog_model.py) judged on the corpus (tests/jpeg_prog_cases.py) by Pillow's decoder and by the
library's own progressive entropy decoder, the validity of every table, the re-derived max_out_bytes, and the coder as compiled
(flgpu_debug_jpeg_progressive_scans, and tests/jpeg_prog_host.cpp plain and under ASan + UBSan) against the model.  No GPU."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_opt_model as jm
import jpeg_prog_cases as cases
import jpeg_prog_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")


# ----------------------------------------------------------------------------------------------------------- the ABI --

def test_the_constants_the_headers_and_the_shim(fl, tmp_path):
    assert fl.ENCODE_JPEG_PROGRESSIVE == 0x400000 and fl.FEO_JPEG_PROGRESSIVE == 16 and fl.load_library().flgpu_abi_version() == 6
    assert C.sizeof(fl.flgpu_params) == 28 and fl.flgpu_params.reserved.offset == 26 and fl.flgpu_params.reserved.size == 2
    others = (fl.ACCEPT_WEBP, fl.ACCEPT_AVIF, fl.ENCODE_PNG, fl.DECODE_PNG_ADAM7, fl.ENCODE_WEBP_LOSSLESS, fl.ENCODE_GIF, fl.ENCODE_GIF_QUANTIZE, fl.ENCODE_WEBP_LOSSY,
              fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER, fl.ENCODE_WEBP_LOSSY_ALPHA, fl.ENCODE_WEBP_LOSSY_SEGMENTS,
              fl.ENCODE_JPEG_OPTIMIZE, fl.ENCODE_JPEG_420, 0x100000)
    assert not any(fl.ENCODE_JPEG_PROGRESSIVE & b for b in others)
    assert tuple(fl.make_params().reserved) == (0, 0) and tuple(fl.make_params(jpeg_progressive=True).reserved) == (16, 0)
    assert tuple(fl.make_params(jpeg_progressive=True, jpeg_420=True, jpeg_optimize=True, segments=True, alpha_vp8l=True).reserved) == (31, 0)
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert "#define FLGPU_ENCODE_JPEG_PROGRESSIVE 0x400000u" in header and "#define FLGPU_FEO_JPEG_PROGRESSIVE 16u" in header
    assert "#define FLGPU_ABI_VERSION 6" in header and "uint8_t options;" in header
    assert "void encode_jpeg_progressive() { flags_ |= FLGPU_ENCODE_JPEG_PROGRESSIVE; }" in open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    shim = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    assert "ENCODE_JPEG_PROGRESSIVE: u32 = 0x400000" in shim and "FEO_JPEG_PROGRESSIVE: u8 = 16" in shim
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fanlin_gpu.h"\nint main(void) { printf("%zu %zu %zu %u %u %d\\n", sizeof(flgpu_params), '
                   'offsetof(flgpu_params, options), offsetof(flgpu_params, reserved), FLGPU_FEO_JPEG_PROGRESSIVE, FLGPU_ENCODE_JPEG_PROGRESSIVE, FLGPU_ABI_VERSION); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["28", "26", "27", "16", str(0x400000), "6"]


def test_the_cpp_mirror_sets_the_flag(fl, tmp_path):
    """include/fanlin_gpu.hpp: content::Format::encode_jpeg_progressive() sets the accept bit and no other."""
    src = tmp_path / "mirror.cpp"
    src.write_text('#include <cstdio>\n#include "fanlin_gpu.hpp"\nint main() { fanlin::content::Format f; f.accept_webp(); const unsigned before = f.flags(); '
                   'f.encode_jpeg_progressive(); std::printf("%u %u\\n", before, f.flags()); return 0; }\n')
    exe, libdir = str(tmp_path / "mirror"), os.path.dirname(fl.LIB_PATH)
    subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", str(src), "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lfanlin_gpu",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    before, after = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert before == fl.ACCEPT_WEBP and after == before | fl.ENCODE_JPEG_PROGRESSIVE


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=3):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


def test_the_mapping_of_the_accept_bit(fl):
    """The option is set exactly where flgpu_params_from_query chooses FLGPU_FE_JPEG; nothing else of the parameters moves, and of a
    plan only max_out_bytes of the JPEG arm -- and not even that beside the 4:2:0 bit."""
    new = fl.ENCODE_JPEG_PROGRESSIVE

    def fields(p):
        return [getattr(p, n) for n, _ in fl.flgpu_params._fields_ if n != "reserved"]
    every = (fl.ENCODE_PNG | fl.ENCODE_WEBP_LOSSLESS | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS | fl.ENCODE_WEBP_LOSSY_FILTER
             | fl.ENCODE_WEBP_LOSSY_ALPHA | fl.ENCODE_WEBP_LOSSY_SEGMENTS | fl.ENCODE_GIF | fl.ENCODE_GIF_QUANTIZE | fl.ENCODE_JPEG_OPTIMIZE)
    for query in ("w=300&h=200", "w=300&h=200&quality=30", "w=300&h=200&webp=true&quality=75", "w=300&h=200&avif=true", "blur=12", "w=300&h=200&webp=true&quality=100"):
        q = fl.Query.parse(query)
        for accept in (0, fl.ACCEPT_WEBP, fl.ACCEPT_AVIF, fl.ACCEPT_WEBP | fl.ACCEPT_AVIF):
            for extra in (0, every, fl.ENCODE_JPEG_420):
                for is_jpeg in (0, 1, 2):
                    flags = accept | extra
                    without, fmt0 = q.to_params(fl.Format(flags), is_jpeg)
                    with_bit, fmt1 = q.to_params(fl.Format(flags | new), is_jpeg)
                    assert fields(without) == fields(with_bit) and fmt0 == fmt1 and without.reserved[1] == with_bit.reserved[1] == 0
                    assert without.reserved[0] & fl.FEO_JPEG_PROGRESSIVE == 0 and with_bit.reserved[0] & ~fl.FEO_JPEG_PROGRESSIVE == without.reserved[0]
                    want = with_bit.front_end == fl.FE_JPEG
                    assert want == (is_jpeg == 2 and fmt1 == fl.OUT_KEEP), (query, hex(flags), is_jpeg)
                    assert bool(with_bit.reserved[0] & fl.FEO_JPEG_PROGRESSIVE) == want, (query, hex(flags), is_jpeg)
                for fmt in (fl.IN_JPEG, fl.IN_PNG, fl.IN_WEBP, fl.IN_OTHER, fl.IN_GIF_FRAME):
                    (rc0, k0, a), (rc1, k1, b) = _plan(fl, query, accept | extra, fmt), _plan(fl, query, accept | extra | new, fmt)
                    assert (rc0, k0) == (rc1, k1), (query, fmt)
                    grows = rc0 == fl.OK and k0 == fl.RESULT_JPEG_STREAM and not extra & fl.ENCODE_JPEG_420
                    if grows:
                        units = 3 * (a.plane_w // 8) * (a.plane_h // 8)
                        assert (a.max_out_bytes, b.max_out_bytes) == (1024 + 2 * 208 * units, 1104 + 2 * 216 * units), (query, fmt)
                        b.max_out_bytes = a.max_out_bytes
                    assert bytes(a) == bytes(b), (query, fmt, "only max_out_bytes of the JPEG arm moves")
    # as_is never reaches a front end
    rc, kind, _ = _plan(fl, "", new, fl.IN_JPEG)
    assert rc == fl.OK and kind == fl.RESULT_AS_IS
    # only FE_JPEG knows the bit; beside the 4:2:0 bit it is ignored
    for fe in (fl.FE_JFIF444, fl.FE_PNG, fl.FE_WEBP420, fl.FE_NONE, fl.FE_WEBP_LOSSLESS, fl.FE_WEBP_LOSSY):
        a, b = fl.plan_output(fl.make_params(quality=75, front_end=fe), 300, 200, 4), fl.plan_output(fl.make_params(quality=75, front_end=fe, jpeg_progressive=True), 300, 200, 4)
        assert bytes(a) == bytes(b), fe
    for optimize in (False, True):
        a = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_JPEG, jpeg_420=True, jpeg_optimize=optimize), 300, 200, 4)
        b = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_JPEG, jpeg_420=True, jpeg_optimize=optimize, jpeg_progressive=True), 300, 200, 4)
        assert bytes(a) == bytes(b)
    a = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_JPEG, jpeg_progressive=True), 300, 200, 4)
    b = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_JPEG, jpeg_progressive=True, jpeg_optimize=True), 300, 200, 4)
    assert bytes(a) == bytes(b) and a.max_out_bytes == 1104 + 2 * 216 * 2850


# ----------------------------------------------------------------------------------------------------------- the model --

def _pillow(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    return np.asarray(im), bool(im.info.get("progressive"))


def _segments(data):
    """[(marker, body)] of every marker segment of a file with several scans (entropy-coded data skipped)"""
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker = data[at + 1]
        if marker == 0xD9:
            assert at + 2 == len(data)
            return out
        n = int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            while not (data[at] == 0xFF and data[at + 1] != 0):
                at += 1


def test_the_corpus_reaches_what_it_is_there_for(oracle):
    assert len(cases.NAMES) == len(set(cases.NAMES))
    cases.check_conditions(oracle)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_corpus_file_is_progressive_valid_and_shows_the_baseline_pixels(fl, oracle, name):
    img, q = cases.get(oracle, name)
    h, w, c = img.shape
    data, info = cases.model(oracle, name)
    std = oracle.jpeg_encode(img, q)
    pixels, progressive = _pillow(data)
    assert progressive and np.array_equal(pixels, _pillow(std)[0])
    assert np.array_equal(fl.debug_jpeg_blob(data)[1], oracle.jpeg_file_coefficients(std))
    print(name, len(std), "->", len(data))
    # the segments: the baseline prefix with SOF2, then DHT DHT SOS, and four times DHT SOS
    assert data[:pm.PREFIX_BYTES] == std[:pm.SOF_MARKER_AT] + b"\xc2" + std[pm.SOF_MARKER_AT + 1:pm.PREFIX_BYTES] and data[-2:] == b"\xff\xd9"
    segs = _segments(data)
    assert [m for m, _ in segs] == [0xE0, 0xC2, 0xDB, 0xDB, 0xC4, 0xC4, 0xDA] + [0xC4, 0xDA] * 4
    assert segs[6][1] == bytes([3, 1, 0x00, 2, 0x10, 3, 0x10, 0, 0, 0])
    for k, (comp, ss, se) in enumerate(pm.AC_SCANS):
        assert segs[8 + 2 * k][1] == bytes([1, comp + 1, 0x00, ss, se, 0])
    dhts = [body for m, body in segs if m == 0xC4]
    assert [b[0] for b in dhts] == [0x00, 0x01, 0x10, 0x10, 0x10, 0x10]
    for t, body in enumerate(dhts):
        cnt, lut = info["counts"][t], info["rules"][t]["lut"]
        used = sorted(s for s in range(256) if cnt[s])
        assert used and sorted(body[17:]) == used and len(body) == 17 + len(used) and sum(body[1:17]) == len(used)
        assert len(used) <= (12 if t < 2 else 176)
        kraft, codes = 0, []
        for s in used:
            length, code = int(lut[s]) >> 16, int(lut[s]) & 0xFFFF
            assert 1 <= length <= 16 and code < (1 << length) - 1, (t, s, "no code is all ones, none longer than 16 bits")
            kraft += 1 << (16 - length)
            codes.append(format(code, "0%db" % length))
        assert kraft <= (1 << 16) - 1
        codes.sort()
        assert not any(b.startswith(a) for a, b in zip(codes, codes[1:])), (t, "a prefix code")
    bound = int(fl.plan_output(fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_progressive=True), w, h, c).max_out_bytes)
    assert len(data) <= bound


def test_the_bound_holds_for_the_longest_codes(fl, oracle):
    """Noise at quality 100 is the corpus' densest coding: its bytes per unit against the 216 (stuffed: 432) the bound allows."""
    for name in ("noise_32x32_q100", "noise_256x256_q100"):
        img, q = cases.get(oracle, name)
        units = 3 * (img.shape[0] // 8) * (img.shape[1] // 8)
        assert len(cases.model(oracle, name)[0]) <= 1104 + 2 * 216 * units
    # a picture of one block: the header's worst case is what the fixed part is for
    one = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_JPEG, jpeg_progressive=True), 1, 1, 3)
    assert one.max_out_bytes == 1104 + 2 * 216 * 3 and 1104 >= 177 + 2 * (21 + 12) + 14 + 4 * (21 + 176 + 10) + 2 + 2 * 5


# ----------------------------------------------------------------------------------------------------------- the coder as compiled --

TWIN_NAMES = cases.NAMES


def test_the_library_twin_equals_the_model(fl, oracle):
    for name in TWIN_NAMES:
        img, q = cases.get(oracle, name)
        got = fl.debug_jpeg_progressive_scans(oracle.jpeg_coefficients(img, q), oracle.jpeg_header(img.shape[1], img.shape[0], q))
        want, info = cases.model(oracle, name)
        assert np.array_equal(got["counts"], info["counts"]), name
        assert got["file"] == want, name


@pytest.mark.parametrize("sanitised", (False, True), ids=("plain", "asan_ubsan"))
def test_the_stand_alone_twin_equals_the_model(oracle, tmp_path, sanitised):
    """The core header driven by a program of its own; the second build runs it under ASan + UBSan."""
    exe = str(tmp_path / "jpeg_prog_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitised else []
    subprocess.run(["g++", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-std=c++17", *extra, os.path.join(ROOT, "tests", "jpeg_prog_host.cpp"), "-I", CSRC, "-o", exe], check=True)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for name in TWIN_NAMES:
            img, q = cases.get(oracle, name)
            coef = oracle.jpeg_coefficients(img, q)
            f.write(struct.pack("<I", len(coef) // 3) + oracle.jpeg_header(img.shape[1], img.shape[0], q)[:pm.PREFIX_BYTES] + b"\0\0\0" + coef.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == f"jpeg_prog ok {len(TWIN_NAMES)} records\n" and not r.stderr, (r.returncode, r.stdout, r.stderr)
    raw, at = open(dst, "rb").read(), 0
    for name in TWIN_NAMES:
        want, info = cases.model(oracle, name)
        counts = np.frombuffer(raw[at:at + 6144], np.uint32).reshape(6, 256)
        n = struct.unpack("<I", raw[at + 6144:at + 6148])[0]
        assert np.array_equal(counts, info["counts"]) and raw[at + 6148:at + 6148 + n] == want, name
        at += 6148 + n
    assert at == len(raw)
