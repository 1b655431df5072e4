"""Adam7-interlaced PNG sources, host half (csrc/fl_pngsrc.cpp with the Adam7 bit, csrc/fl_png_adam7.h): what
flgpu_png_info_of_flags reports, and the inflated stream -- the seven passes' filtered scanlines back to back -- from
flgpu_debug_png_scanlines_flags.  No GPU.  Files come from tests/png_adam7_write.py, which this module also pins against
Pillow's reader."""
import io
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_adam7_write as aw
import png_write as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")

SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (4, 4), (5, 5), (8, 8), (9, 9), (13, 11)]      # (width, height)
KINDS = [(2, 8), (0, 1), (3, 2)]                                                          # RGB8, grey 1-bit, palette 2-bit


def rng(seed):
    return np.random.default_rng(seed)


def status_of(fl, fn, *args, **kw):
    try:
        fn(*args, **kw)
    except fl.FanlinError as e:
        return e.status
    return fl.OK


def sample(ct, depth, w, h, seed=0):
    r = rng(1000 * seed + 64 * ct + 8 * depth + 16 * w + h)
    s = r.integers(0, 1 << depth, (h, w, pw.SAMPLES[ct]))
    plte = r.integers(0, 256, (1 << depth, 3)) if ct == 3 else None
    return s, plte


def mixed(seed):
    """A filter type per pass row, seeded."""
    r = rng(seed)
    return lambda k, ph: r.integers(0, 5, ph).tolist()


def reassemble(data, stream, **kw):
    import struct
    w, h, d, ct = struct.unpack(">IIBB", data[16:26])
    plte = next((p for _, k, p in pw.chunks_of(data) if k == b"PLTE"), None)
    return pw.assemble(w, h, d, ct, stream, plte=None if plte is None else np.frombuffer(plte, np.uint8), interlace=1, **kw)


# ---- flgpu_png_info_of_flags ------------------------------------------------------------------------------------------

def test_info_with_and_without_the_flag(fl):
    from PIL import Image
    s, _ = sample(2, 8, 6, 4)
    inter = aw.write_png(s, 2)
    assert fl.png_info(inter) == {"width": 6, "height": 4, "color_type": 2, "bit_depth": 8, "channels": 0, "interlaced": 1, "has_trns": 0, "supported": 0}
    assert fl.png_info(inter, adam7=True) == {"width": 6, "height": 4, "color_type": 2, "bit_depth": 8, "channels": 3, "interlaced": 1, "has_trns": 0, "supported": 1}
    # sub-byte with tRNS: the channels of the expanded picture
    g, _ = sample(0, 2, 7, 5)
    assert fl.png_info(aw.write_png(g, 0, 2, trns=[1]), adam7=True)["channels"] == 2
    # 16-bit samples, interlaced: unsupported either way
    buf = io.BytesIO()
    Image.fromarray(rng(1).integers(0, 65536, (4, 6)).astype(np.uint16)).save(buf, "PNG")
    sixteen = buf.getvalue()
    sixteen = sixteen[:8] + pw.ihdr(6, 4, 16, 0, 1) + sixteen[8 + 25:]
    for adam7 in (False, True):
        info = fl.png_info(sixteen, adam7=adam7)
        assert (info["bit_depth"], info["interlaced"], info["supported"], info["channels"]) == (16, 1, 0, 0)
        assert status_of(fl, fl.debug_png_scanlines, sixteen, adam7=adam7) == fl.ERR_UNSUPPORTED
    # a non-interlaced file: the same either way
    plain = pw.write_png(s, 2, filters=4)
    assert fl.png_info(plain) == fl.png_info(plain, adam7=True)
    assert fl.png_info(plain)["supported"] == 1
    assert fl.debug_png_scanlines(plain) == fl.debug_png_scanlines(plain, adam7=True) == zlib.decompress(pw.idat_payload(plain))
    # without the flag the host half refuses the interlaced file as before
    assert status_of(fl, fl.debug_png_scanlines, inter) == fl.ERR_UNSUPPORTED


# ---- the inflated stream: seven passes back to back ----------------------------------------------------------------------

@pytest.mark.parametrize("ct,depth", KINDS)
def test_scanlines_are_the_passes_back_to_back(fl, ct, depth):
    for k, (w, h) in enumerate(SIZES):
        s, plte = sample(ct, depth, w, h)
        filters = mixed(k)
        data = aw.write_png(s, ct, depth, filters=filters, plte=plte)
        want = aw.scanlines(s, ct, depth, mixed(k))
        assert want == zlib.decompress(pw.idat_payload(data))
        assert len(want) == aw.scan_bytes(w, h, ct, depth), (w, h)
        assert fl.debug_png_scanlines(data, adam7=True) == want, (w, h)


def test_scanlines_from_seven_byte_idat_chunks(fl):
    s, _ = sample(2, 8, 13, 11, seed=1)
    data = aw.write_png(s, 2, filters=mixed(20), split=7)
    assert sum(1 for _, k, _ in pw.chunks_of(data) if k == b"IDAT") > 10
    assert fl.debug_png_scanlines(data, adam7=True) == aw.scanlines(s, 2, 8, mixed(20))


def test_absent_passes_contribute_nothing():
    # 1 x 1: pass 1 alone; 1 x 9: no pass with an x origin beyond 0; 4 x 4: passes 2 and 3 are absent (x0 = 4, y0 = 4)
    assert aw.scan_bytes(1, 1, 2, 8) == 1 + 3
    assert [p for p in aw.pass_shapes(4, 4)] == [(1, 1), (0, 1), (1, 0), (1, 1), (2, 1), (2, 2), (4, 2)]
    assert aw.scan_bytes(4, 4, 0, 1) == 2 + 2 + 2 + 2 * 2 + 2 * 2           # every pass row of up to 8 one-bit samples is one byte
    assert aw.scan_bytes(9, 9, 0, 1) == 2 * 2 + 2 * 2 + 1 * 2 + 3 * 2 + 2 * 2 + 5 * 2 + 4 * 3   # (pass 7: 9 bits, two bytes a row)


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_too_many_too_few_bad_filter_byte_bad_adler(fl):
    s, _ = sample(2, 8, 13, 11, seed=2)
    data = aw.write_png(s, 2, filters=1)
    raw = aw.scanlines(s, 2, 8, 1)
    assert fl.debug_png_scanlines(data, adam7=True) == raw
    for level in (0, 1, 9):
        assert status_of(fl, fl.debug_png_scanlines, reassemble(data, zlib.compress(raw + b"\0", level)), adam7=True) == fl.ERR_UNSUPPORTED
    assert status_of(fl, fl.debug_png_scanlines, reassemble(data, zlib.compress(raw[:-1])), adam7=True) == fl.ERR_PARSE
    # filter byte 5 in the first row of pass 4: behind passes 1..3
    shapes, rbs = aw.pass_shapes(13, 11), aw.pass_row_bytes(13, 11, 2, 8)
    at = sum(ph * (1 + rb) for (_, ph), rb in list(zip(shapes, rbs))[:3])
    assert at == 41 and raw[at] == 1   # 2 x (1 + 6) + 2 x (1 + 6) + 1 x (1 + 12)
    bad = bytearray(raw)
    bad[at] = 5
    assert status_of(fl, fl.debug_png_scanlines, reassemble(data, zlib.compress(bytes(bad))), adam7=True) == fl.ERR_PARSE
    # ... and one byte further it is a sample, not a filter byte
    ok = bytearray(raw)
    ok[at + 1] = 5
    assert fl.debug_png_scanlines(reassemble(data, zlib.compress(bytes(ok))), adam7=True) == bytes(ok)
    stream = zlib.compress(raw)
    assert status_of(fl, fl.debug_png_scanlines, reassemble(data, stream[:-1] + bytes([stream[-1] ^ 1])), adam7=True) == fl.ERR_PARSE
    # a header that announces far more picture than the file could hold: too few bytes, nothing is reserved
    assert status_of(fl, fl.png_info, pw.assemble(30000, 30000, 8, 0, stream, interlace=1), adam7=True) == fl.ERR_PARSE


# ---- the writer, against Pillow's reader ------------------------------------------------------------------------------------

@pytest.mark.parametrize("ct,depth", KINDS)
def test_writer_files_decode_to_their_samples_in_pillow(ct, depth):
    from PIL import Image
    for k, (w, h) in enumerate(SIZES):
        s, plte = sample(ct, depth, w, h)
        data = aw.write_png(s, ct, depth, filters=mixed(30 + k), plte=plte)
        img = Image.open(io.BytesIO(data))
        assert img.info.get("interlace") == 1
        want = pw.expand(s, ct, depth, plte)
        got = np.asarray(img.convert("RGB" if want.shape[2] == 3 else "L"))
        assert np.array_equal(got.reshape(want.shape), want), (ct, depth, w, h)


# ---- the public texts ---------------------------------------------------------------------------------------------------------

def test_header_shim_and_python_name_the_bits(fl):
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert int(re.search(r"#define FLGPU_IMG_PNG_ADAM7\s+(\d+)u", header).group(1)) == 256 == fl.IMG_PNG_ADAM7
    assert int(re.search(r"#define FLGPU_DECODE_PNG_ADAM7\s+(0x[0-9a-fA-F]+)u", header).group(1), 16) == 0x10000 == fl.DECODE_PNG_ADAM7
    assert int(re.search(r"#define FLGPU_ABI_VERSION\s+(\d+)", header).group(1)) == 6
    assert fl.load_library().flgpu_abi_version() == 6
    shim = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    assert int(re.search(r"const IMG_PNG_ADAM7: u32 = (\d+);", shim).group(1)) == 256
    assert int(re.search(r"pub const DECODE_PNG_ADAM7: u32 = (0x[0-9a-fA-F]+);", shim).group(1), 16) == 0x10000
    assert "fn flgpu_png_info_of_flags(" in shim
    # the blob header keeps its size: sixteen words and the palette
    text = open(os.path.join(CSRC, "fl_pngsrc.h")).read()
    body = re.search(r"struct alignas\(16\) PngBlobHeader \{(.*?)\n\};", text, re.S).group(1)
    assert "uint32_t interlaced;" in body and "uint32_t pad;" not in body
    # one statement of the pass table: the kernel file and the host half take it from fl_png_adam7.h
    for name in ("fl_pngsrc.cpp", "fl_pngdec.hip", "fl_source.cpp"):
        src = open(os.path.join(CSRC, name)).read()
        assert "adam7_pass(" in src and "0x0102040" not in src, name


# ---- sanitized stand-alone program ------------------------------------------------------------------------------------

def test_mutated_adam7_files_under_address_and_ub_sanitizers(tmp_path):
    """tests/png_adam7_fuzz.cpp + csrc/fl_pngsrc.cpp as one program with -fsanitize=address,undefined, run as a child process:
    2,000 seeded byte / bit mutations of each file through the info and scanline functions with the Adam7 bit; any sanitizer
    report aborts it."""
    exe = str(tmp_path / "png_adam7_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts in whatever environment it is given
                    os.path.join(ROOT, "tests", "png_adam7_fuzz.cpp"), os.path.join(CSRC, "fl_pngsrc.cpp"), "-o", exe], check=True)
    files = []
    specs = [(2, 8, 13, 11, dict()), (0, 1, 9, 9, dict(level=0)), (3, 2, 5, 5, dict(split=7)), (2, 8, 1, 9, dict(strategy=zlib.Z_FIXED)),
             (0, 1, 4, 4, dict(level=9)), (3, 2, 13, 11, dict(strategy=zlib.Z_HUFFMAN_ONLY))]
    for k, (ct, depth, w, h, kw) in enumerate(specs):
        s, plte = sample(ct, depth, w, h, seed=3)
        path = tmp_path / f"a{k}.png"
        path.write_bytes(aw.write_png(s, ct, depth, filters=mixed(40 + k), plte=plte, **kw))
        files.append(str(path))
    r = subprocess.run([exe, "2000"] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("file ")]
    assert len(lines) == len(files)
    for l in lines:
        f = dict(kv.split("=") for kv in l.split()[2:])
        # every intact file decoded, no pass table contradicted itself, and the mutants were really looked at
        assert f["intact"] == "ok" and int(f["mutants"]) == 2000 and int(f["broken"]) == 0 and int(f["refused"]) > 1000, l
