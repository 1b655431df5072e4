"""The PNG encoder's model, shared by test_png_encode.py and test_png_encode_edges.py: the png crate's adaptive row filter
restated in numpy, the stream checker that takes a device file apart, and the segment layout that csrc/fl_png.hip's header
comment promises (one IDAT chunk per 32 KB segment of the filtered stream, each whole bytes, then one IDAT for the Adler-32)."""
import io
import struct
import zlib

import numpy as np

SEG = 32768


def filtered_bytes(w, h, c):
    return h * (1 + w * c)


def max_out_bytes(w, h, c):
    """The format's worst case as the header states it: every 32 KB segment as stored blocks + flush + chunk framing."""
    f = filtered_bytes(w, h, c)
    nseg = (f + SEG - 1) // SEG
    lens = [SEG] * (nseg - 1) + [f - (nseg - 1) * SEG]
    return 8 + 25 + 2 + 4 + 12 + 12 + sum(n + 5 * ((n + 65534) // 65535) + 5 + 12 for n in lens)


def _candidates(px):
    """The four filtered candidates of every row (Sub, Up, Average, Paeth) and their scores sum |(i8)byte|."""
    h, w, c = px.shape
    cur = px.reshape(h, w * c).astype(np.int32)
    up = np.vstack([np.zeros((1, w * c), np.int32), cur[:-1]])
    a = np.hstack([np.zeros((h, c), np.int32), cur[:, :-c]]) if w > 1 else np.zeros_like(cur)
    ul = np.hstack([np.zeros((h, c), np.int32), up[:, :-c]]) if w > 1 else np.zeros_like(cur)
    p = a + up - ul
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, ul))
    cands = [(cur - pred) & 255 for pred in (a, up, (a + up) >> 1, paeth)]  # Sub, Up, Average, Paeth
    scores = [np.abs(x.astype(np.uint8).view(np.int8).astype(np.int64)).sum(axis=1) for x in cands]
    return cands, scores


def filter_scores(px):
    """(h, 4) int64: the scores of Sub, Up, Average and Paeth for every row, as filter_rows() compares them."""
    return np.stack(_candidates(px)[1], axis=1)


def filter_rows(px):
    """png 0.17 filter() with AdaptiveFilterType::Adaptive, restated: (filter bytes, filtered stream)."""
    h, w, c = px.shape
    cands, scores = _candidates(px)
    choice = np.ones(h, np.int64)
    best = scores[0].copy()
    for f in range(1, 4):
        take = scores[f] <= best
        best = np.where(take, scores[f], best)
        choice = np.where(take, f + 1, choice)
    out = np.empty((h, 1 + w * c), np.uint8)
    out[:, 0] = choice
    rows = np.stack(cands)[choice - 1, np.arange(h)]
    out[:, 1:] = rows.astype(np.uint8)
    return choice, out.tobytes()


def unfilter(stream, w, h, c):
    rb = w * c
    rows = np.frombuffer(stream, np.uint8).reshape(h, 1 + rb)
    out = np.zeros((h, rb), np.int32)
    prev = np.zeros(rb, np.int32)
    for y in range(h):
        f, d = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        r = np.zeros(rb, np.int32)
        for x in range(rb):
            a = r[x - c] if x >= c else 0
            b = prev[x]
            cc = prev[x - c] if x >= c else 0
            if f == 0:
                pr = 0
            elif f == 1:
                pr = a
            elif f == 2:
                pr = b
            elif f == 3:
                pr = (a + b) >> 1
            else:
                p = a + b - cc
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                pr = a if pa <= pb and pa <= pc else (b if pb <= pc else cc)
            r[x] = (d[x] + pr) & 255
        out[y] = r
        prev = r
    return out.astype(np.uint8).reshape(h, w, c)


def chunks_of(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "PNG signature"
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + body), f"CRC of chunk {len(out)} ({typ})"
        out.append((typ, body))
        pos += 12 + n
    assert pos == len(data), "trailing bytes"
    return out


def check_stream(data, pixels, quality):
    """Every structural and content rule of the contract; returns the zlib stream."""
    h, w, c = pixels.shape
    ch = chunks_of(data)
    types = [t for t, _ in ch]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and ch[-1][1] == b""
    assert len(types) >= 3 and all(t == b"IDAT" for t in types[1:-1]), types
    assert struct.unpack(">IIBBBBB", ch[0][1]) == (w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], 0, 0, 0)
    z = b"".join(b for t, b in ch[1:-1])
    assert z[0] == 0x78 and (z[0] * 256 + z[1]) % 31 == 0 and not (z[1] & 0x20)
    assert z[1] >> 6 == (3 if quality < 50 else 2 if quality < 85 else 0), "FLEVEL follows the level"
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", "zlib stream incomplete (or Adler-32 wrong)"
    assert len(raw) == h * (1 + w * c)
    choice, want = filter_rows(pixels)
    got_filters = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * c)[:, 0]
    assert np.array_equal(got_filters, choice), "filter bytes differ from the adaptive rule"
    assert raw == want, "filtered rows differ"
    if h * w * c <= 64 * 64 * 4:
        assert np.array_equal(unfilter(raw, w, h, c), pixels)
    try:
        from PIL import Image
        im = np.asarray(Image.open(io.BytesIO(data)))
        assert np.array_equal(im.reshape(h, w, c), pixels), "PIL decodes other pixels"
    except ImportError:
        pass
    return z, raw


def segment_chunks(data):
    """The chunk layout of csrc/fl_png.hip's header comment, checked on one device file.  Returns (filtered stream, the
    segments' raw deflate bodies): bodies[s] is IDAT chunk s without the first chunk's 2-byte zlib header.

    - IHDR, then exactly nseg IDAT chunks (nseg from IHDR's own dimensions), then one 4-byte IDAT = the Adler-32, then IEND;
    - only the first chunk starts with the zlib header;
    - every segment's chunk is at most 2 (first only) + 5 + L bytes: the stored form is the ceiling;
    - every non-final chunk is whole bytes on its own: one stored block of L bytes with BFINAL = 0, or a stream that ends with the
      empty stored block's 00 00 FF FF;
    - chunk s, inflated as raw deflate with the filtered bytes before it as the dictionary, is filtered bytes
      [32768 s, 32768 s + L) and nothing else; only the last one ends the deflate stream."""
    ch = chunks_of(data)
    assert ch[0][0] == b"IHDR" and ch[-1] == (b"IEND", b"")
    w, h, depth, ctype = struct.unpack(">IIBB", ch[0][1][:10])
    c = {0: 1, 4: 2, 2: 3, 6: 4}[ctype]
    f = filtered_bytes(w, h, c)
    nseg = (f + SEG - 1) // SEG
    idat = [b for t, b in ch[1:-1]]
    assert all(t == b"IDAT" for t, _ in ch[1:-1])
    assert len(idat) == nseg + 1, f"{len(idat)} IDAT chunks for {nseg} segments"
    assert len(idat[-1]) == 4, "the last IDAT holds the Adler-32 alone"
    assert idat[0][0] == 0x78 and (idat[0][0] * 256 + idat[0][1]) % 31 == 0
    bodies = [idat[0][2:]] + idat[1:-1]
    raw = b""
    for s, body in enumerate(bodies):
        L = min(SEG, f - s * SEG)
        final = s == nseg - 1
        assert 12 + (2 if s == 0 else 0) + len(body) <= 12 + 2 + 5 + L, f"segment {s}: chunk longer than its stored form"
        stored = (body[0] & 6) == 0
        if stored:
            assert len(body) == 5 + L and body[1:5] == struct.pack("<HH", L, L ^ 0xFFFF), f"segment {s}: not one stored block"
            assert (body[0] & 1) == (1 if final else 0), f"segment {s}: BFINAL of the stored block"
        elif not final:
            assert body[-4:] == b"\x00\x00\xff\xff", f"segment {s}: no empty stored block at its end"
        d = zlib.decompressobj(-15, zdict=raw[-SEG:]) if raw else zlib.decompressobj(-15)
        got = d.decompress(body)
        assert d.unused_data == b"" and d.unconsumed_tail == b"", f"segment {s}: bytes after its blocks"
        assert d.eof == final, f"segment {s}: BFINAL {'missing' if final else 'set before the last segment'}"
        assert len(got) == L, f"segment {s} inflates to {len(got)} bytes, not {L}"
        raw += got
    assert len(raw) == f
    assert struct.unpack(">I", idat[-1])[0] == zlib.adler32(raw), "Adler-32 chunk"
    return raw, bodies
