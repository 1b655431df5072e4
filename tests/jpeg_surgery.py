"""Marker surgery on baseline JPEG files (T.81 Annex B), in plain Python: the layouts Pillow's writer cannot be asked for are made
from the files it does write, by rewriting marker segments and leaving the entropy-coded segment as it is.

One walker (`segments`) and one rewriter (`rewrite`) carry everything else.  Only single-scan files are handled: every marker
segment in front of the first SOS, then the scan up to EOI."""

SOF0, DHT, SOS, DQT, APP0, APP14 = 0xC0, 0xC4, 0xDA, 0xDB, 0xE0, 0xEE


def segments(data):
    """([(marker, payload)] of every marker segment up to and including the SOS header, offset of the scan's first byte)."""
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, out = 2, []
    while True:
        assert data[pos] == 0xFF, pos
        if data[pos + 1] == 0xFF:                                  # a fill byte in front of a marker (B.1.1.2)
            pos += 1
            continue
        m, ln = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        assert ln >= 2 and pos + 2 + ln <= len(data), (pos, m, ln)
        out.append((m, bytes(data[pos + 4:pos + 2 + ln])))
        pos += 2 + ln
        if m == SOS:
            return out, pos


def rewrite(data, fn):
    """The file with every marker segment passed through fn(marker, payload) -> a list of (marker, payload) to stand in its place
    (an empty list drops it); the scan is copied as it is."""
    segs, scan = segments(data)
    out = bytearray(b"\xff\xd8")
    for m, p in segs:
        for m2, p2 in fn(m, p):
            out += bytes([0xFF, m2]) + (len(p2) + 2).to_bytes(2, "big") + p2
    return bytes(out) + bytes(data[scan:])


def frame(data):
    """(height, width, [(id, h, v, tq)]) of the SOF0 header."""
    for m, p in segments(data)[0]:
        if m == SOF0:
            return (int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big"),
                    [(p[6 + 3 * i], p[7 + 3 * i] >> 4, p[7 + 3 * i] & 15, p[8 + 3 * i]) for i in range(p[5])])
    raise AssertionError("no SOF0")


def _sof(data, edit):
    def fn(m, p):
        if m != SOF0:
            return [(m, p)]
        q = bytearray(p)
        edit(q)
        return [(m, bytes(q))]
    return rewrite(data, fn)


def to_440(data):
    """A 4:2:2 file of an h x w picture -> a 4:4:0 file of a w x h (height x width) one.  Both layouts code an MCU as Y Y Cb Cr, and
    with the two dimensions swapped the MCU counts agree (ceil(w / 16) * ceil(h / 8) either way), so the entropy-coded segment stays
    valid.  The picture is a scramble of the original's blocks -- the same scramble for every decoder."""
    def edit(q):
        assert q[5] == 3 and q[7] == 0x21 and q[10] == 0x11 and q[13] == 0x11, "not a 4:2:2 file"
        q[1:3], q[3:5] = q[3:5], q[1:3]
        q[7] = 0x12
    return _sof(data, edit)


def to_rgb(data):
    """A three-component file whose samples are to be read as R, G, B: the JFIF APP0 segment (which says YCbCr) goes, an APP14 Adobe
    segment with transform 0 takes its place.  The planes may be sub-sampled; nothing else changes."""
    adobe = b"Adobe" + (100).to_bytes(2, "big") + bytes(4) + b"\x00"       # version, flags0, flags1, transform
    assert len(frame(data)[2]) == 3
    seen = []

    def fn(m, p):
        if m == APP0 and p[:5] == b"JFIF\0":
            seen.append(m)
            return [(APP14, adobe)]
        assert not (m == APP14 and p[:5] == b"Adobe"), "already carries an Adobe segment"
        return [(m, p)]
    out = rewrite(data, fn)
    assert seen == [APP0], "no JFIF segment to replace"
    return out


def dqt16(data):
    """Every quantiser table rewritten at 16-bit precision (Pq = 1), same step values."""
    def fn(m, p):
        if m != DQT:
            return [(m, p)]
        out, o = bytearray(), 0
        while o < len(p):
            pq, tq = p[o] >> 4, p[o] & 15
            steps = [int.from_bytes(p[o + 1 + 2 * k:o + 3 + 2 * k], "big") if pq else p[o + 1 + k] for k in range(64)]
            out += bytes([0x10 | tq]) + b"".join(s.to_bytes(2, "big") for s in steps)
            o += 1 + 64 * (pq + 1)
        assert o == len(p)
        return [(m, bytes(out))]
    return rewrite(data, fn)


def gray_2x2(data):
    """A one-component file whose sampling byte says 2 x 2, as some encoders write it: a single component is never interleaved
    (A.2.2), so the factors mean nothing and a decoder must ignore them."""
    def edit(q):
        assert q[5] == 1 and q[7] == 0x11
        q[7] = 0x22
    return _sof(data, edit)


def huffman_tables(data):
    """[(class, id, longest code length, length of the end-of-block code (AC tables; None for DC tables))] of every DHT table."""
    out = []
    for m, p in segments(data)[0]:
        o = 0
        while m == DHT and o < len(p):
            tc, th, counts = p[o] >> 4, p[o] & 15, list(p[o + 1:o + 17])
            vals = p[o + 17:o + 17 + sum(counts)]
            lengths = [l + 1 for l in range(16) for _ in range(counts[l])]      # code k (canonical order) has lengths[k] bits
            eob = lengths[vals.index(0)] if tc == 1 and 0 in vals else None
            out.append((tc, th, max(lengths), eob))
            o += 17 + len(vals)
    return out


def entropy_bits(data):
    """Bits of the entropy-coded segment with byte stuffing (0xFF00 -> 0xFF), fill bytes and restart markers taken out: the segment
    ends at the first other marker."""
    pos, n, nbytes = segments(data)[1], len(data), 0
    while pos < n:
        ff = data.find(b"\xff", pos)
        if ff < 0 or ff + 1 >= n:
            nbytes += (n if ff < 0 else ff) - pos
            break
        nbytes += ff - pos
        nxt = data[ff + 1]
        if nxt == 0x00:
            nbytes, pos = nbytes + 1, ff + 2
        elif nxt == 0xFF:
            pos = ff + 1
        elif 0xD0 <= nxt <= 0xD7:
            pos = ff + 2
        else:
            break
    return 8 * nbytes
