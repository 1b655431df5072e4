"""Host half of the PNG decode front end (csrc/fl_pngsrc.cpp): container parsing with chunk CRCs, our own inflate, Adler-32.
No GPU: flgpu_png_info_of and flgpu_debug_png_scanlines are pure host functions.  The inflated scanlines are held against
zlib.decompress of the same IDAT payload; files come from tests/png_write.py."""
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_write as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")


def rng(seed):
    return np.random.default_rng(seed)


def status_of(fl, fn, *args):
    try:
        fn(*args)
    except fl.FanlinError as e:
        return e.status
    return fl.OK


# ---- flgpu_png_info_of ------------------------------------------------------------------------------------------------

COMBOS = [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)]
CHANNELS = {(0, False): 1, (0, True): 2, (2, False): 3, (2, True): 4, (3, False): 3, (3, True): 4, (4, False): 2, (6, False): 4}


def sample_file(ct, depth, trns, w=11, h=5, seed=0, **kw):
    r = rng(seed + 16 * ct + depth)
    s = r.integers(0, 1 << depth, (h, w, pw.SAMPLES[ct]))
    plte = r.integers(0, 256, (min(1 << depth, 200), 3)) if ct == 3 else None
    t = None
    if trns:
        t = {0: [int(s[0, 0, 0])], 2: [int(v) for v in s[0, 0]], 3: bytes(r.integers(0, 256, 5).astype(np.uint8))}[ct]
    return pw.write_png(s, ct, depth, plte=plte, trns=t, **kw), s, plte, t


@pytest.mark.parametrize("ct,depth,trns", [(ct, d, t) for ct, d in COMBOS for t in (False, True) if not (t and ct in (4, 6))])
def test_info_of_every_colour_type_and_depth(fl, ct, depth, trns):
    data, *_ = sample_file(ct, depth, trns)
    info = fl.png_info(data)
    assert info == {"width": 11, "height": 5, "color_type": ct, "bit_depth": depth, "channels": CHANNELS[(ct, trns)],
                    "interlaced": 0, "has_trns": int(trns), "supported": 1}


def test_info_of_sixteen_bit_and_interlaced_files_are_unsupported(fl):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rng(1).integers(0, 65536, (4, 6)).astype(np.uint16)).save(buf, "PNG")
    info = fl.png_info(buf.getvalue())
    assert (info["bit_depth"], info["supported"], info["channels"]) == (16, 0, 0)
    assert status_of(fl, fl.debug_png_scanlines, buf.getvalue()) == fl.ERR_UNSUPPORTED
    data = pw.write_png(rng(2).integers(0, 256, (4, 6, 3)), 2, interlace=1)  # (the IDAT is not Adam7 data: the header alone decides)
    info = fl.png_info(data)
    assert (info["interlaced"], info["supported"], info["channels"]) == (1, 0, 0)
    assert status_of(fl, fl.debug_png_scanlines, data) == fl.ERR_UNSUPPORTED


def test_info_of_skips_ancillary_chunks(fl):
    extra = [(b"gAMA", struct.pack(">I", 45455)), (b"sRGB", b"\0"), (b"tEXt", b"Comment\0hello"), (b"eXIf", b"MM\0*\0\0\0\x08\0\0")]
    s = rng(3).integers(0, 256, (3, 4, 3))
    data = pw.write_png(s, 2, extra=extra)
    assert fl.png_info(data)["supported"] == 1
    assert fl.debug_png_scanlines(data) == zlib.decompress(pw.idat_payload(data))
    # an ancillary chunk is not interpreted, so a bad CRC on it does not matter; an unknown critical chunk does
    bad = pw.SIGNATURE + pw.ihdr(4, 3, 8, 2) + pw.chunk(b"tEXt", b"x", crc=0) + data[8 + 25:]
    assert fl.png_info(bad)["supported"] == 1
    crit = pw.SIGNATURE + pw.ihdr(4, 3, 8, 2) + pw.chunk(b"ABCD", b"x") + data[8 + 25:]
    assert status_of(fl, fl.png_info, crit) == fl.ERR_PARSE


def test_info_of_rejects_damaged_containers(fl):
    data, *_ = sample_file(3, 4, True, split=7)
    assert status_of(fl, fl.png_info, b"\x89PNX" + data[4:]) == fl.ERR_PARSE
    assert status_of(fl, fl.png_info, data[:7]) == fl.ERR_PARSE
    chunks = pw.chunks_of(data)
    for off, kind, payload in chunks:                     # truncation at every chunk boundary (and inside the chunk)
        assert status_of(fl, fl.png_info, data[:off]) == fl.ERR_PARSE, kind
        assert status_of(fl, fl.png_info, data[:off + 8 + len(payload) // 2]) == fl.ERR_PARSE, kind
    for off, kind, payload in chunks:                     # a flipped CRC on every chunk that is interpreted
        at = off + 8 + len(payload)
        bad = data[:at] + bytes([data[at] ^ 0x40]) + data[at + 1:]
        assert status_of(fl, fl.png_info, bad) == fl.ERR_PARSE, kind
    # missing PLTE for colour type 3, zero and oversized dimensions, depths a colour type does not have
    s = rng(4).integers(0, 4, (2, 2, 1))
    assert status_of(fl, fl.png_info, pw.write_png(s, 3, 2)) == fl.ERR_PARSE
    stream = pw.idat_payload(data)
    for w, h, d, ct in ((0, 5, 8, 0), (5, 0, 8, 0), (1 << 31, 1, 8, 0), (2, 2, 4, 2), (2, 2, 3, 0), (2, 2, 8, 5)):
        assert status_of(fl, fl.png_info, pw.assemble(w, h, d, ct, stream)) == fl.ERR_PARSE, (w, h, d, ct)
    # chunk orders the png crate refuses: IDAT chunks apart, tRNS in front of PLTE
    one = pw.chunks_of(sample_file(3, 4, True, split=7)[0])
    raw = {k: pw.chunk(k, p) for _, k, p in one if k != b"IDAT"}
    idats = [pw.chunk(k, p) for _, k, p in one if k == b"IDAT"]
    ok = pw.SIGNATURE + raw[b"IHDR"] + raw[b"PLTE"] + raw[b"tRNS"] + b"".join(idats) + raw[b"IEND"]
    assert fl.png_info(ok)["supported"] == 1
    apart = pw.SIGNATURE + raw[b"IHDR"] + raw[b"PLTE"] + raw[b"tRNS"] + idats[0] + pw.chunk(b"tEXt", b"a\0b") + b"".join(idats[1:]) + raw[b"IEND"]
    assert status_of(fl, fl.png_info, apart) == fl.ERR_PARSE
    early = pw.SIGNATURE + raw[b"IHDR"] + raw[b"tRNS"] + raw[b"PLTE"] + b"".join(idats) + raw[b"IEND"]
    assert status_of(fl, fl.png_info, early) == fl.ERR_PARSE
    # a header that announces far more picture than the file could hold: too few bytes, nothing is reserved
    assert status_of(fl, fl.png_info, pw.assemble(30000, 30000, 8, 0, stream)) == fl.ERR_PARSE


def test_rust_shim_and_cpp_mirror_know_the_png_entry_points(fl):
    import re
    text = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    m = re.search(r"pub struct FlPngInfo \{(.*?)\}", text, re.S)
    names = [f.split(":")[0].strip() for f in m.group(1).split(",") if ":" in f]
    assert names == [n for n, _ in fl.flgpu_png_info._fields_]
    assert all(t == "u32" for t in re.findall(r":\s*(\w+)", m.group(1)))
    block = re.search(r'extern "C" \{(.*?)\n\}', text, re.S).group(1)
    assert {"flgpu_png_info_of", "flgpu_process_png", "flgpu_process_png_plan"} <= set(re.findall(r"fn (flgpu_\w+)\(", block))
    assert "pub fn png_info(" in text and "pub fn process_png(" in text
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert int(re.search(r"const IMG_PNG_SOURCE: u32 = (\d+);", text).group(1)) == int(re.search(r"#define FLGPU_IMG_PNG_SOURCE\s+(\d+)u", header).group(1)) == fl.IMG_PNG_SOURCE
    hpp = open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    assert "process_png(" in hpp and "flgpu_png_info_of" in hpp
    # the C struct is eight u32
    import ctypes
    assert ctypes.sizeof(fl.flgpu_png_info) == 32


# ---- inflate ------------------------------------------------------------------------------------------------------------

def noise(h, w, seed=5):
    return rng(seed).integers(0, 256, (h, w, 3))


def rows_repeating_32768_back():
    # 3 x 10922 + 1 filter byte = 32767 bytes per scanline + ... : a grey row of 32767 samples makes scanlines of exactly 32768 bytes,
    # so every row repeats the one before it at the maximum distance
    row = rng(6).integers(0, 256, (1, 32767, 1))
    return np.repeat(row, 4, axis=0)


STREAMS = {
    "stored": lambda: dict(samples=noise(20, 30), level=0),
    "stored_spans_blocks": lambda: dict(samples=noise(150, 200), level=0),            # 90,150 bytes: more than one stored block
    "fixed": lambda: dict(samples=noise(9, 65), strategy=zlib.Z_FIXED, filters=[4, 3, 2, 1, 0, 4, 4, 3, 1]),
    "huffman_only": lambda: dict(samples=noise(40, 50), strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": lambda: dict(samples=np.repeat(noise(40, 10), 5, axis=1), strategy=zlib.Z_RLE, filters=1),
    "level9_noise": lambda: dict(samples=noise(64, 64), level=9, filters=4),
    "level9_flat": lambda: dict(samples=np.full((200, 300, 3), 77), level=9),         # length-258 matches
    "level9_max_distance": lambda: dict(samples=rows_repeating_32768_back(), level=9, color_type=0),
    "level6_gradient": lambda: dict(samples=(np.add.outer(np.arange(120), np.arange(160))[:, :, None] // np.array([1, 2, 3])) % 256, filters=2),
}


@pytest.mark.parametrize("name", sorted(STREAMS))
@pytest.mark.parametrize("split", [None, 1, 7, "empty"])
def test_scanlines_equal_zlib(fl, name, split):
    kw = STREAMS[name]()
    data = pw.write_png(kw.pop("samples"), kw.pop("color_type", 2), split=split, **kw)
    want = zlib.decompress(pw.idat_payload(data))
    assert fl.debug_png_scanlines(data) == want
    if name == "level9_max_distance":
        assert len(want) == 4 * 32768


def test_match_at_distance_32768(fl):
    # zlib itself never looks further back than 32,506 bytes, so the longest distance is written by hand: a stored block of 32,768 bytes,
    # then a fixed block with one match of length 258 (code 285) at distance 32,768 (code 29 + 13 extra bits, all ones) and end-of-block
    w, h = 16512, 2
    first = bytearray(rng(9).integers(0, 256, 32768).astype(np.uint8).tobytes())
    first[0] = 0
    first[1 + w] = 2
    want = bytes(first) + bytes(first[:258])
    assert len(want) == h * (1 + w)
    fixed = [1, 1, 0] + [1, 1, 0, 0, 0, 1, 0, 1] + [1, 1, 1, 0, 1] + [1] * 13 + [0] * 7
    stream = b"\x78\x01" + b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + bytes(first) + bits_to_bytes(fixed) + struct.pack(">I", zlib.adler32(want))
    assert zlib.decompress(stream) == want
    assert fl.debug_png_scanlines(pw.assemble(w, h, 8, 0, stream, split=4096)) == want
    # one byte less of history: the same match now starts before the stream
    short = b"\x78\x01" + b"\x00" + struct.pack("<HH", 32767, 32767 ^ 0xFFFF) + bytes(first[:32767]) + bits_to_bytes(fixed) + b"\0\0\0\0"
    assert status_of(fl, fl.debug_png_scanlines, pw.assemble(w, h, 8, 0, short)) == fl.ERR_PARSE


def test_writer_files_are_valid_for_pillow(fl):
    from PIL import Image
    s = noise(9, 65, seed=7)
    data = pw.write_png(s, 2, filters=[4, 3, 2, 1, 0, 4, 4, 3, 1], strategy=zlib.Z_FIXED, split=1)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), s.astype(np.uint8))


def reassemble(data, stream):
    w, h, d, ct = struct.unpack(">IIBB", data[16:26])
    return pw.assemble(w, h, d, ct, stream)


def bits_to_bytes(bits):
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        out[i >> 3] |= b << (i & 7)
    return bytes(out)


def test_broken_streams_are_parse_errors(fl):
    s = noise(6, 8, seed=8)
    data = pw.write_png(s, 2, filters=1)
    stream = pw.idat_payload(data)
    assert fl.debug_png_scanlines(data) == zlib.decompress(stream)
    bad = {
        "adler": stream[:-1] + bytes([stream[-1] ^ 1]),
        "last_byte_missing": stream[:-1],
        "half": stream[:len(stream) // 2],
        "zlib_header": b"\x79" + stream[1:],
        "reserved_block_type": stream[:2] + b"\x07" + stream[3:],
        # fixed block: the literal 'a' (code 0x30 + 97, 8 bits), then a match of length 3 (code 257: 0000001) at distance 2 (code 1: 00001):
        # one byte of history, so the distance points before the start of the stream
        "distance_before_start": b"\x78\x01" + bits_to_bytes([1, 1, 0] + [int(c) for c in format(0x30 + 97, "08b")] + [0, 0, 0, 0, 0, 0, 1] + [0, 0, 0, 0, 1] + [0] * 7) + b"\0\0\0\0",
        # dynamic block whose code-length code gives four symbols the length 1: over-subscribed
        "oversubscribed": b"\x78\x01" + bits_to_bytes([1, 0, 1] + [0] * 5 + [0] * 5 + [0, 0, 0, 0] + [1, 0, 0] * 4 + [0] * 16) + b"\0\0\0\0",
        # stored block whose length and its complement disagree
        "stored_nlen": b"\x78\x01\x01\x05\x00\x00\x00hello",
    }
    for name, st in bad.items():
        assert status_of(fl, fl.debug_png_scanlines, reassemble(data, st)) == fl.ERR_PARSE, name
    # filter byte 5 on a row
    raw = bytearray(pw.scanlines(s, 2, 8, 0))
    raw[3 * (1 + 24)] = 5
    assert status_of(fl, fl.debug_png_scanlines, reassemble(data, zlib.compress(bytes(raw)))) == fl.ERR_PARSE
    # one scanline too few is a parse error, one extra scanline of data is for the caller's decoder to judge
    raw = pw.scanlines(s, 2, 8, 0)
    assert status_of(fl, fl.debug_png_scanlines, reassemble(data, zlib.compress(raw[:-25]))) == fl.ERR_PARSE
    for level in (0, 1, 9):
        assert status_of(fl, fl.debug_png_scanlines, reassemble(data, zlib.compress(raw + raw[:25], level))) == fl.ERR_UNSUPPORTED


def test_host_half_links_no_zlib(fl):
    # (the HIP runtime the library links brings its own libz into the process: what counts is what the library itself asks for)
    syms = subprocess.run(["nm", "-D", "--undefined-only", fl.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("inflate", "inflateInit_", "inflateInit2_", "uncompress", "crc32", "adler32", "dlopen_zlib"):
        assert not any(l.split()[-1].split("@")[0] == name for l in syms.splitlines() if l.strip()), name
    src = open(os.path.join(CSRC, "fl_pngsrc.cpp")).read() + open(os.path.join(CSRC, "fl_pngsrc.h")).read()
    assert "zlib.h" not in src and "dlopen" not in src and "#include <hip" not in src


# ---- sanitized stand-alone program ------------------------------------------------------------------------------------

def test_mutated_files_under_address_and_ub_sanitizers(fl, tmp_path):
    """tests/png_host_fuzz.cpp + csrc/fl_pngsrc.cpp as one program with -fsanitize=address,undefined, run as a child process:
    2,000 seeded byte / bit mutations of each file through the info and scanline functions; any sanitizer report aborts it."""
    exe = str(tmp_path / "png_host_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts in whatever environment it is given
                    os.path.join(ROOT, "tests", "png_host_fuzz.cpp"), os.path.join(CSRC, "fl_pngsrc.cpp"), "-o", exe], check=True)
    files = []
    specs = [(2, 8, False, dict(filters=4)), (3, 2, True, dict(split=7)), (0, 1, True, dict(level=0)), (6, 8, False, dict(strategy=zlib.Z_FIXED)),
             (0, 4, False, dict(strategy=zlib.Z_HUFFMAN_ONLY)), (4, 8, False, dict(level=9, split="empty"))]
    for k, (ct, depth, trns, kw) in enumerate(specs):
        data, *_ = sample_file(ct, depth, trns, w=37, h=19, seed=100 + k, **kw)
        path = tmp_path / f"f{k}.png"
        path.write_bytes(data)
        files.append(str(path))
    r = subprocess.run([exe, "2000"] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    # every intact file decoded, and the mutants were really looked at: most are refused, some survive (a flipped pixel bit cannot be told)
    lines = [l for l in r.stdout.splitlines() if l.startswith("file ")]
    assert len(lines) == len(files)
    for l in lines:
        f = dict(kv.split("=") for kv in l.split()[2:])
        assert f["intact"] == "ok" and int(f["mutants"]) == 2000 and int(f["refused"]) > 1000, l
