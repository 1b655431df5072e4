"""The corpus of the device-inflate tests (test_png_inflate_host.py holds the host twin against it, test_png_inflate_device.py the
kernel): deflate streams made by zlib in every mode, and hand-written ones (deflate_write.py) for what zlib never writes.  A stream is
wrapped as a one-row greyscale PNG, whose scanline data is one filter byte 0 and then anything: valid() = [(name, file, scanlines)],
broken() = [(name, file)].  Built once per process."""
import functools
import os
import re
import zlib

import numpy as np

import deflate_write as dw
import png_write as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    text = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_inflate.h")).read()
    return {k: int(v) for k, v in re.findall(r"(kInf(?:SubBits|Subs)) = (\d+)", text)}


K = kernel_constants()
SUB_BITS, SUBS = K["kInfSubBits"], K["kInfSubs"]
STRIP_BITS = SUB_BITS * SUBS
HEADER_BYTES = 16 * 4 + 256 * 4   # csrc/fl_pngsrc.h PngBlobHeader
PAD = 16                          # kPngzPad


def one_row(stream: bytes, raw_len: int) -> bytes:
    """a greyscale PNG of one row whose scanline data has raw_len bytes (the filter byte and raw_len - 1 pixels)"""
    return pw.assemble(raw_len - 1, 1, 8, 0, stream)


def rows(n, seed):
    """n bytes that start with 0: smooth-ish data, so that zlib finds literals and matches"""
    r = np.random.default_rng(seed)
    x = np.cumsum(r.integers(-2, 3, n)) % 256
    x[r.integers(0, n, n // 50)] = r.integers(0, 256, n // 50)
    x[0] = 0
    return x.astype(np.uint8).tobytes()


def z(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, sync_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out = b""
    if flush_every:
        for i in range(0, len(raw), flush_every):
            out += co.compress(raw[i:i + flush_every]) + co.flush(zlib.Z_SYNC_FLUSH)
    elif sync_at is not None:
        out = co.compress(raw[:sync_at]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(raw[sync_at:])
    else:
        out = co.compress(raw)
    return out + co.flush()


def fixed_literals(n8, n9=0):
    """n8 literals of 8 bits (the first is the filter byte 0) and n9 of 9 bits in the fixed code"""
    return [0] + [1 + k % 143 for k in range(n8 - 1)] + [200] * n9


@functools.lru_cache(maxsize=None)
def valid():
    out = []

    def add(name, stream, raw):
        assert zlib.decompress(stream) == raw, name
        out.append((name, one_row(stream, len(raw)), raw))

    noise = bytes([0]) + np.random.default_rng(1).integers(0, 256, 16383, dtype=np.uint8).tobytes()
    period = bytes([0]) + np.random.default_rng(2).integers(0, 256, 32767, dtype=np.uint8).tobytes()
    add("stored-level0-spanning", z(rows(70000, 3), 0), rows(70000, 3))
    add("stored-65535", z(rows(65535, 4), 0), rows(65535, 4))
    add("empty-stored-from-sync-flush", z(rows(3000, 5), sync_at=1500), rows(3000, 5))
    add("z-fixed", z(rows(16384, 6), strategy=zlib.Z_FIXED), rows(16384, 6))
    add("z-huffman-only", z(rows(16384, 7), strategy=zlib.Z_HUFFMAN_ONLY), rows(16384, 7))
    add("z-rle", z(rows(16384, 8), strategy=zlib.Z_RLE), rows(16384, 8))
    add("level9-noise", z(noise, 9), noise)
    add("flat", z(bytes(16384), 6), bytes(16384))
    add("rows-32768-back", z(period * 3, 9), period * 3)
    add("sync-flush-every-100", z(rows(6000, 9), flush_every=100), rows(6000, 9))
    add("level6-long", z(rows(60000, 10), 6), rows(60000, 10))

    def hand(name, blocks):
        """blocks: [(kind, tokens, kwargs)]"""
        w, raw = dw.Writer(), b""
        for i, (kind, tokens, kw) in enumerate(blocks):
            final = i == len(blocks) - 1
            if kind == "fixed":
                dw.fixed_block(w, tokens, final)
            else:
                dw.dynamic_block(w, tokens, final, **kw)
            raw += dw.expand(tokens, raw)
        add(name, dw.zlib_stream(w, raw), raw)

    lits = [0] + [int(v) for v in np.random.default_rng(11).integers(0, 256, 32767)]
    hand("match-at-distance-32768", [("dynamic", lits + [(258, 32768), 5, (3, 32768)], {})])
    hand("length-258-at-distance-1", [("fixed", [0, 7] + [(258, 1)] * 40 + [9, (258, 1)], {})])
    hand("chain-of-3-3-matches", [("fixed", [0, 1, 2, 3] + [(3, 3)] * 3000, {})])
    deep = [0] * 286
    for s in range(14):
        deep[s] = s + 1
    deep[14] = deep[256] = 15
    hand("15-bit-codes", [("dynamic", [0] + [int(v) for v in np.random.default_rng(12).integers(0, 15, 4000)] + [14, 13, 14], dict(lit_lengths=deep))])
    hand("single-distance-code", [("dynamic", [0, 1, 2, 3, 4, (4, 4), 9, (5, 4), (3, 4)], {})])
    hand("literal-only-dynamic", [("dynamic", [0] + [int(v) for v in np.random.default_rng(13).integers(0, 40, 5000)], {})])
    hand("fewer-bits-than-a-subsequence", [("fixed", [0, 1], {})])
    # the fixed block's tokens start at bit 16 + 3; literals below 144 have 8 bits, the end-of-block symbol 7
    per_strip = STRIP_BITS // 8
    hand("eob-in-the-last-subsequence", [("fixed", fixed_literals(per_strip - 6), {})])
    hand("eob-in-the-first-of-the-next-strip", [("fixed", fixed_literals(per_strip), {})])
    # 8 a + 9 b + 7 = one strip's bits, with one 9-bit literal
    a = (STRIP_BITS - 7 - 9) // 8
    assert 8 * a + 9 + 7 == STRIP_BITS
    hand("exactly-one-strip", [("fixed", fixed_literals(a, 1), {})])
    hand("one-strip-minus-a-token", [("fixed", fixed_literals(a - 1, 1), {})])
    hand("one-strip-plus-a-token", [("fixed", fixed_literals(a + 1, 1), {})])
    hand("blocks-of-every-kind", [("fixed", [0, 1, 2, (5, 2)], {}), ("dynamic", [4, 5, (6, 3), (4, 9)], {}), ("fixed", [(10, 8), 1], {})])
    return out


@functools.lru_cache(maxsize=None)
def broken():
    out = []
    raw = rows(5000, 20)
    good = z(raw, 6)
    # an over-subscribed code: three codes of one bit
    w = dw.Writer()
    lens = [0] * 286
    lens[0] = lens[1] = lens[256] = 1
    dw.dynamic_block(w, [0, 1, 0], True, lit_lengths=lens)
    out.append(("over-subscribed-code", one_row(dw.zlib_stream(w, bytes([0, 1, 0])), 3)))
    # a distance that reaches before the start of the stream
    w = dw.Writer()
    dw.fixed_block(w, [0, 1, (3, 5), 2], True)
    out.append(("distance-before-the-start", one_row(dw.zlib_stream(w, bytes(6)), 6)))
    out.append(("truncated", one_row(good[:len(good) * 2 // 3], len(raw))))
    out.append(("bad-adler", one_row(good[:-1] + bytes([good[-1] ^ 1]), len(raw))))
    out.append(("filter-byte-5", one_row(z(bytes([5]) + raw[1:], 6), len(raw))))
    out.append(("one-byte-too-many", one_row(good, len(raw) - 1)))
    out.append(("one-byte-too-few", one_row(good, len(raw) + 1)))
    return out


def picture(ct, depth, w, h, seed, trns=False, interlace=0, **kw):
    """(file, expected pixels) of a small picture with a mix of filters, as test_png_source.py makes them"""
    r = np.random.default_rng(seed)
    s = r.integers(0, 1 << depth, (h, w, pw.SAMPLES[ct]))
    plte = r.integers(0, 256, (max(2, (1 << depth) - 3), 3)) if ct == 3 else None
    t = None
    if trns:
        t = {0: [int(s[h // 2, w // 2, 0])], 2: [int(v) for v in s[h // 2, w // 2]], 3: bytes(r.integers(0, 256, max(1, (1 << depth) // 2)).astype(np.uint8))}[ct]
    if interlace:
        import png_adam7_write as aw
        data = aw.write_png(s, ct, depth, filters=lambda k, ph: r.integers(0, 5, ph).tolist(), plte=plte, trns=t, **kw)
    else:
        data = pw.write_png(s, ct, depth, filters=r.integers(0, 5, h).tolist(), plte=plte, trns=t, **kw)
    return data, pw.expand(s, ct, depth, plte, t)
