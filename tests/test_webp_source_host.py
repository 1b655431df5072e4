"""Host half of the lossless WebP decode front end (csrc/fl_webpsrc.cpp): the RIFF container, the VP8L headers, and the whole
entropy stage -- prefix codes, LZ77 with the short-distance map, colour cache, meta prefix codes, the transforms' sub-images.
No GPU: flgpu_webp_info_of and flgpu_debug_webp_residuals are pure host functions.  The blob they leave is undone by the numpy
inverse of tests/vp8l_write.py and held against the pixels the files were written from; the files themselves (tests/webp_cases.py)
are held against libwebp, through ctypes and through Pillow."""
import ctypes
import io
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import vp8l_model as vm
import vp8l_write as vw
import webp_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
P, X, G, I = vw.PREDICTOR, vw.CROSS, vw.GREEN, vw.PALETTE


def status_of(fl, fn, *args):
    try:
        fn(*args)
    except fl.FanlinError as e:
        return e.status
    return fl.OK


def pillow_pixels(data):
    """Pillow's decode: RGBA, or RGB where libwebp reports no alpha (it goes by the VP8L header's bit, in the extended form too)"""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


# ---- the writer's files are valid for libwebp, and the host half is exact on them --------------------------------------------

@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_writer_file_is_valid_for_libwebp_and_the_host_half_is_exact(fl, name):
    data, want = wc.get(name)
    ref = vm.decode_rgba(data)
    if want is None:
        want = ref   # modes 14 and 15
    c = want.shape[2]
    assert vm._libwebp(), "libwebp itself must be loadable: it is the arbiter"
    assert np.array_equal(ref[..., :c], want), "libwebp (ctypes) does not decode the file to the pixels it was written from"
    pil = pillow_pixels(data)
    assert np.array_equal(pil[..., :c], want[..., :pil.shape[2]]), "Pillow does not decode the file to the pixels it was written from"
    info = fl.webp_info(data)
    assert (info["width"], info["height"], info["channels"], info["supported"], info["lossless"]) == (want.shape[1], want.shape[0], c, 1, 1)
    blob = fl.debug_webp_residuals(data)
    H = vw.blob_header(blob)
    assert (H["width"], H["height"], H["channels"], H["total_bytes"]) == (want.shape[1], want.shape[0], c, len(blob))
    assert sum(1 << t for t in H["ttype"][:H["ntransforms"]]) == info["transforms"]
    if name in wc.BIG:
        return   # (too many pixels for the pixel-by-pixel inverse; the device test decodes it)
    got = vw.inverse(blob)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_pillow_corpus_host_half_is_exact_and_covers_the_format(fl):
    union, cache, groups = 0, 0, 0
    for name, data, px in wc.pillow_corpus():
        info = fl.webp_info(data)
        assert (info["width"], info["height"], info["channels"], info["supported"]) == (px.shape[1], px.shape[0], px.shape[2], 1), name
        assert info["has_alpha"] == int(px.shape[2] == 4) and info["lossless"] == 1 and info["animated"] == 0, name
        union |= info["transforms"]
        cache += info["color_cache_bits"] > 0
        groups += info["prefix_groups"] > 1
        got = vw.inverse(fl.debug_webp_residuals(data))
        assert got.shape == px.shape and np.array_equal(got, px), name
        assert np.array_equal(vm.decode_rgba(data)[..., :px.shape[2]], px), name
    # a condition on the corpus, not a measurement: libwebp's encoder used every transform, a colour cache and several code groups
    assert union == 15 and cache >= 1 and groups >= 1, (union, cache, groups)


def test_short_distance_map_is_the_formats(fl):
    # the writer's table as (dx, dy) against the packed table the decoder uses, read from its source
    text = open(os.path.join(CSRC, "fl_webpsrc.cpp")).read()
    body = re.search(r"kCodeToPlane\[120\] = \{(.*?)\};", text, re.S).group(1)
    packed = [int(v, 16) for v in re.findall(r"0x([0-9a-f]{2})", body)]
    assert len(packed) == 120
    assert [(8 - (e & 15), e >> 4) for e in packed] == vw.PLANE_CODES
    assert vw.plane_distance(5, 4) == 4 and vw.plane_distance(1, 4) == 1 and vw.plane_distance(3, 121) == 1   # (-1, 1) at xsize 1: clamped to 1


# ---- flgpu_webp_info_of -----------------------------------------------------------------------------------------------------

def test_info_fields_on_writer_files(fl):
    base = dict(extended=0, animated=0, lossless=1, exif_orientation=0, supported=1)
    for name, want in {
        "order_none": dict(transforms=0, color_cache_bits=0, prefix_groups=1),
        "order_PXGI": dict(transforms=15, color_cache_bits=0, prefix_groups=1),
        "order_G": dict(transforms=4), "order_X": dict(transforms=2), "order_I": dict(transforms=8), "order_P": dict(transforms=1),
        "stream_cache1": dict(color_cache_bits=1), "stream_cache11": dict(color_cache_bits=11, transforms=0),
        "stream_cache4_transforms": dict(color_cache_bits=4, transforms=7),
        "stream_groups": dict(prefix_groups=5, transforms=1), "stream_groups_cache_refs": dict(prefix_groups=6, color_cache_bits=3),
        "channels_alpha1_simple": dict(has_alpha=1, channels=4), "channels_alpha0_simple": dict(has_alpha=0, channels=3),
    }.items():
        info = fl.webp_info(wc.get(name)[0])
        for k, v in {**base, **want}.items():
            assert info[k] == v, (name, k, info)


def test_info_of_the_extended_form(fl):
    # the VP8X alpha flag decides, not the VP8L header's bit (written the other way round in these files)
    for bit in (0, 1):
        info = fl.webp_info(wc.get(f"channels_alpha{bit}_extended")[0])
        assert (info["extended"], info["has_alpha"], info["channels"], info["exif_orientation"]) == (1, bit, 4 if bit else 3, 0)
    info = fl.webp_info(wc.get("extended_iccp_xmp_unknown")[0])
    assert (info["extended"], info["supported"], info["exif_orientation"], info["transforms"]) == (1, 1, 6, 4)
    for o in range(1, 9):
        for form in ("tiff", "prefixed"):
            info = fl.webp_info(wc.get(f"extended_exif{o}_{form}")[0])
            assert (info["exif_orientation"], info["supported"], info["extended"]) == (o, 1, 1), (o, form)
    # an orientation outside 1..8, and an EXIF chunk that is no TIFF structure: no orientation
    px = wc.noise(4, 4, 1)
    for payload in (vw.exif(9), b"garbage!", b""):
        data = vw.write(px, extended=dict(alpha=True, after=[(b"EXIF", payload)]))
        assert fl.webp_info(data)["exif_orientation"] == 0
    # an EXIF chunk in front of the picture counts too
    data = vw.write(px, extended=dict(alpha=True, before=[(b"EXIF", vw.exif(3))]))
    assert fl.webp_info(data)["exif_orientation"] == 3


def test_info_of_lossy_and_animated_files_are_unsupported(fl):
    from PIL import Image
    img = wc.noise(6, 8, 2)
    for kw, pixels in ((dict(quality=80), img[..., :3]), (dict(quality=80), img), (dict(save_all=True, append_images=[Image.fromarray(255 - img[..., :3])], lossless=True), img[..., :3])):
        b = io.BytesIO()
        Image.fromarray(pixels).save(b, "WEBP", **kw)
        info = fl.webp_info(b.getvalue())
        assert (info["supported"], info["channels"]) == (0, 0), kw
        assert (info["width"], info["height"]) == (8, 6), kw
        assert info["animated"] == int("save_all" in kw) and (info["lossless"] == 0 or info["animated"])
        assert status_of(fl, fl.debug_webp_residuals, b.getvalue()) == fl.ERR_UNSUPPORTED


def test_info_rejects_damaged_containers(fl):
    px = wc.noise(5, 7, 3)
    pay = vw.payload(px, [(G,)])
    good = vw.container(pay)
    assert fl.webp_info(good)["supported"] == 1
    odd = pay if len(pay) & 1 else pay + b"\0"   # an odd payload (a trailing zero byte is more zero bits for the reader)
    assert fl.webp_info(vw.container(odd))["supported"] == 1
    no_pad = vw.container(odd)[:-1]
    no_pad = no_pad[:4] + struct.pack("<I", len(no_pad) - 8) + no_pad[8:]
    bad = {
        "odd chunk without its padding byte": no_pad,
        "chunk length beyond the file": good[:16] + struct.pack("<I", len(pay) + 10) + good[20:],
        "RIFF size too large": vw.container(pay, size=4 + 8 + len(pay) + (len(pay) & 1) + 2),
        "RIFF size too small": vw.container(pay, size=4 + 8 + len(pay) + (len(pay) & 1) - 2),
        "trailing bytes": good + b"\0\0",
        "signature": vw.container(vw.payload(px, [(G,)], signature=0x2E)),
        "version": vw.container(vw.payload(px, [(G,)], version=1)),
        "not RIFF": b"RIFX" + good[4:],
        "not WEBP": good[:8] + b"WEBQ" + good[12:],
        "unknown first chunk": good[:12] + b"ABCD" + good[16:],
        "too short": good[:19],
        "empty VP8L": vw.container(b""),
        "canvas disagrees with the picture": vw.container(pay, extended=dict(width=8, height=5, alpha=True)),
        "extended without a picture": vw.container(pay, extended=dict(width=7, height=5))[:30][:4] + struct.pack("<I", 22) + b"WEBP" + vw.chunk(b"VP8X", bytes(10)),
    }
    for name, data in bad.items():
        assert status_of(fl, fl.webp_info, data) == fl.ERR_PARSE, name
        assert status_of(fl, fl.debug_webp_residuals, data) == fl.ERR_PARSE, name
    assert fl.webp_info(good)["supported"] == 1


# ---- broken streams -------------------------------------------------------------------------------------------------------------

def raw_stream(w, h, body, alpha=1):
    """a simple-form file whose bits after the VP8L header are written by body(BitWriter)"""
    bw = vm.BitWriter()
    bw.put(0x2F, 8); bw.put(w - 1, 14); bw.put(h - 1, 14); bw.put(alpha, 1); bw.put(0, 3)
    body(bw)
    return vw.container(vm.pack(bw.vals, bw.lens)[0])


def onehot(n, *syms):
    h = np.zeros(n, np.int64)
    h[list(syms)] = 1
    return h


def lz_image(first):
    """main image of 2 x 2 pixels, no transforms: green code = {literal 7, length symbol}, distance code = one symbol"""
    def body(bw):
        bw.put(0, 1); bw.put(0, 1); bw.put(0, 1)              # no transform, no colour cache, no meta prefix codes
        ls, ds = (0, 0) if first == "ref" else (3, 1)         # length 1 at plane code 1 = (0, 1): one row up; length 4 at plane code 2 = (1, 0)
        lg, cg = vw.write_code(bw, onehot(280, 7, 256 + ls), 280, style="normal")
        for _ in range(3):
            vw.write_code(bw, onehot(256, 0), 256)
        vw.write_code(bw, onehot(40, ds), 40)
        if first == "ref":
            bw.put(cg[256], lg[256])                          # a backward reference as the first token: before pixel 0
        else:
            bw.put(cg[7], lg[7]); bw.put(cg[259], lg[259])    # one literal, then a copy of 4 into the 3 pixels that are left
            if first == "ok":                                 # ... or three more literals
                bw.vals.pop(); bw.lens.pop()
                for _ in range(3):
                    bw.put(cg[7], lg[7])
    return body


def code_header(cl_lengths, tokens=(), max_symbol=None):
    """a normal code whose code-length code has the given lengths (in kCodeLengthCodeOrder: 17, 18, 0, 1, 2, ...)"""
    def body(bw):
        bw.put(0, 1); bw.put(0, 1); bw.put(0, 1)
        bw.put(0, 1); bw.put(len(cl_lengths) - 4, 4)
        for v in cl_lengths:
            bw.put(v, 3)
        if max_symbol is None:
            bw.put(0, 1)
        else:
            bw.put(1, 1); bw.put(max_symbol[0], 3); bw.put(max_symbol[1], 2 + 2 * max_symbol[0])
        for v, n in tokens:
            bw.put(v, n)
        bw.put(0, 64)
    return body


def test_broken_streams_are_parse_errors_and_the_thread_goes_on(fl):
    good, gpx = wc.get("stream_groups_cache_refs")
    px = wc.noise(5, 7, 4)

    def truncated(data, cut):
        d = data[:len(data) - cut]
        d += b"\0" * (len(d) & 1)
        return d[:4] + struct.pack("<I", len(d) - 8) + d[8:16] + struct.pack("<I", len(d) - 20) + d[20:]

    def transforms_twice(t):
        def body(bw):
            for _ in range(2):
                bw.put(1, 1); bw.put(t, 2)
            bw.put(0, 64)
        return body

    def cache_bits(n):
        def body(bw):
            bw.put(0, 1); bw.put(1, 1); bw.put(n, 4); bw.put(0, 64)
        return body

    assert np.array_equal(vm.decode_rgba(raw_stream(2, 2, lz_image("ok")))[..., 1], np.full((2, 2), 7))   # the hand-written stream itself is sound
    assert np.array_equal(vw.inverse(fl.debug_webp_residuals(raw_stream(2, 2, lz_image("ok"))))[..., 1], np.full((2, 2), 7))
    bad = {
        "stream ends early (pixels)": truncated(good, 8),
        "stream ends early (codes)": truncated(good, len(good) - 40),
        "stream ends early (headers)": truncated(good, len(good) - 26),
        "subtract-green twice": raw_stream(4, 4, transforms_twice(G)),
        "reference before pixel 0": raw_stream(2, 2, lz_image("ref")),
        "copy past the last pixel": raw_stream(2, 2, lz_image("copy")),
        "colour cache of 0 bits": raw_stream(4, 4, cache_bits(0)),
        "colour cache of 12 bits": raw_stream(4, 4, cache_bits(12)),
        # code-length code: four symbols of length 1 / two symbols of length 2 / no symbol at all
        "over-subscribed code-length code": raw_stream(4, 4, code_header([1, 1, 1, 1])),
        "incomplete code-length code": raw_stream(4, 4, code_header([2, 2, 0, 0])),
        "empty code-length code": raw_stream(4, 4, code_header([0, 0, 0, 0])),
        # code-length code {0: 1 bit '0', 2: 1 bit '1'}: symbols 0 and 1 get length 2, the rest none -- an incomplete code
        "incomplete code": raw_stream(4, 4, code_header([0, 0, 1, 0, 1], [(1, 1), (1, 1)], max_symbol=(0, 0))),
        # code-length code {1: '0', 2: '1'}: lengths 1, 1, 1 -- over-subscribed
        "over-subscribed code": raw_stream(4, 4, code_header([0, 0, 0, 1, 1], [(0, 1), (0, 1), (0, 1)], max_symbol=(0, 1))),
        # max_symbol beyond the alphabet (2 + 0xffff > 280): the way a symbol the alphabet does not have -- a cache index without a cache -- would have to be written
        "max_symbol beyond the alphabet": raw_stream(4, 4, code_header([0, 0, 1, 1], max_symbol=(7, 0xFFFF))),
        # code-length code {17: '0', 0: '1'}: 17 with 3 extra bits repeats zero 10 times, 28 times over: fine; once more runs past symbol 280
        "repeat past the alphabet": raw_stream(4, 4, code_header([1, 0, 1, 0], [(0b1110, 4)] * 29)),
    }
    for name, data in bad.items():
        assert status_of(fl, fl.debug_webp_residuals, data) == fl.ERR_PARSE, name
        assert np.array_equal(vw.inverse(fl.debug_webp_residuals(good)), gpx), name   # the next call on this thread succeeds
    # a repeat of each of the four transform types (the ones with a sub-image need it in between)
    for t in ((P, 2, 1), (X, 2, (1, 2, 3)), (I, np.unique(vw.to_argb(px)))):
        pay = vw.payload(px, [t])
        assert fl.webp_info(vw.container(pay))["supported"] == 1
    for t in (P, X, I):
        def twice(bw, t=t):
            bw.put(1, 1); bw.put(t, 2)
            bw.put(0, 8 if t == I else 3)                           # one colour / block bits 2
            vw.encode_image(bw, np.full((1, 1) if t == I else (2, 2), 0xFF000000, np.uint32))
            bw.put(1, 1); bw.put(t, 2); bw.put(0, 64)
        assert status_of(fl, fl.debug_webp_residuals, raw_stream(5, 5, twice)) == fl.ERR_PARSE, t


# ---- sanitized stand-alone program ------------------------------------------------------------------------------------------------

def test_mutated_files_under_address_and_ub_sanitizers(fl, tmp_path):
    """tests/webp_host_fuzz.cpp + csrc/fl_webpsrc.cpp as one program with -fsanitize=address,undefined, run as a child process:
    2,000 seeded mutations (bit flips, byte overwrites, truncations, length-field edits) of each of four small files through the
    info and residual functions; any sanitizer report aborts it, a decode with the wrong pixel count fails it."""
    exe = str(tmp_path / "webp_host_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts in whatever environment it is given
                    os.path.join(ROOT, "tests", "webp_host_fuzz.cpp"), os.path.join(CSRC, "fl_webpsrc.cpp"), "-o", exe], check=True)
    files = []
    for k, name in enumerate(["order_PXGI", "stream_groups_cache_refs", "stream_cache4_transforms", "extended_iccp_xmp_unknown"]):
        path = tmp_path / f"f{k}.webp"
        path.write_bytes(wc.get(name)[0])
        files.append(str(path))
    r = subprocess.run([exe, "2000"] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("file ")]
    assert len(lines) == len(files)
    for l in lines:
        f = dict(kv.split("=") for kv in l.split()[2:])
        # every intact file decoded, and the mutants were really looked at: many are refused, some survive (a flipped literal cannot be told)
        assert f["intact"] == "ok" and int(f["mutants"]) == 2000 and int(f["wrong"]) == 0 and int(f["refused"]) > 500, l


def test_host_half_is_plain_cpp(fl):
    src = open(os.path.join(CSRC, "fl_webpsrc.cpp")).read() + open(os.path.join(CSRC, "fl_webpsrc.h")).read()
    assert "#include <hip" not in src and "webp/decode.h" not in src and "dlopen" not in src
    # nothing is allocated in the decode path: the one vector is the deep header walk's work area
    assert src.count("std::vector") == 1 and "malloc" not in src and "new " not in src.replace("new red", "")


# ---- mirrors ------------------------------------------------------------------------------------------------------------------------

def test_rust_shim_cpp_mirror_and_ctypes_know_the_webp_entry_points(fl, tmp_path):
    text = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    m = re.search(r"pub struct FlWebpInfo \{(.*?)\}", text, re.S)
    names = [f.split(":")[0].strip() for f in m.group(1).split(",") if ":" in f]
    assert names == [n for n, _ in fl.flgpu_webp_info._fields_]
    assert all(t == "u32" for t in re.findall(r":\s*(\w+)", m.group(1)))
    block = re.search(r'extern "C" \{(.*?)\n\}', text, re.S).group(1)
    assert {"flgpu_webp_info_of", "flgpu_process_webp", "flgpu_process_webp_plan"} <= set(re.findall(r"fn (flgpu_\w+)\(", block))
    assert "pub fn webp_info(" in text and "pub fn process_webp(" in text
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert int(re.search(r"const IMG_WEBP_SOURCE: u32 = (\d+);", text).group(1)) == int(re.search(r"#define FLGPU_IMG_WEBP_SOURCE\s+(\d+)u", header).group(1)) == fl.IMG_WEBP_SOURCE == 64
    fields = re.search(r"typedef struct flgpu_webp_info \{(.*?)\} flgpu_webp_info;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert [n.strip() for decl in re.findall(r"uint32_t ([^;]+);", fields) for n in decl.split(",")] == names
    assert ctypes.sizeof(fl.flgpu_webp_info) == 48 and len(names) == 12
    lib = fl.load_library()
    for sym in ("flgpu_webp_info_of", "flgpu_decode_webp", "flgpu_process_webp", "flgpu_process_webp_plan", "flgpu_debug_webp_residuals"):
        assert sym in fl.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    hpp = open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    assert "process_webp(" in hpp and "flgpu_webp_info_of" in hpp
    # the C++ mirror compiles the way the other clients do, and its webp_info (no device needed) reads a file
    exe = str(tmp_path / "webp_src_host")
    libdir = os.path.dirname(fl.LIB_PATH)
    subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", os.path.join(ROOT, "tests", "webp_src_host.cpp"), "-I", os.path.join(ROOT, "include"),
                    "-L", libdir, "-lfanlin_gpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    path = tmp_path / "f.webp"
    path.write_bytes(wc.get("extended_exif5_tiff")[0])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (kv.split("=") for kv in out.split())}
    assert got == fl.webp_info(wc.get("extended_exif5_tiff")[0])


def test_process_webp_plan_needs_no_device(fl):
    data, px = wc.get("extended_exif6_tiff")
    C = ctypes
    lib = fl.load_library()
    plan, kind = fl.flgpu_plan(), C.c_int()
    assert lib.flgpu_process_webp_plan(data, len(data), b"w=30&h=20", 0, C.byref(plan), C.byref(kind)) == fl.OK
    assert kind.value != fl.RESULT_AS_IS
    assert lib.flgpu_process_webp_plan(data, len(data), b"", 0, C.byref(plan), C.byref(kind)) == fl.OK and kind.value == fl.RESULT_AS_IS
    assert lib.flgpu_process_webp_plan(data[:30], 30, b"w=30&h=20", 0, C.byref(plan), C.byref(kind)) == fl.ERR_PARSE
