"""FLGPU_FEO_JPEG_OPTIMIZE restated in numpy: from the oracle's quantised coefficients (oracle.jpeg_coefficients) and its header
(oracle.jpeg_header) to the scan's symbols, their counts, the table rule of csrc/fl_jpeg_opt_core.h, the coder
and the file, the never-larger decision included.  Tables are in DHT order: 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma; a code
table is a uint32[256] of length << 16 | code (0 = no code)."""
import numpy as np

LIMIT = 16
PREFIX_BYTES = 177      # SOI, APP0, SOF0, DQT, DQT
SOS_BYTES = 14
STD_HEADER_BYTES = 623


# ----------------------------------------------------------------------------------------------------------- the scan's symbols --

def _size(v):
    return int(abs(int(v))).bit_length()


def _value(v, size):
    v = int(v)
    return (v if v >= 0 else v - 1) & ((1 << size) - 1)


def symbols(coef):
    """[(table, symbol, value, value bits)] of the whole scan in coding order; coef = oracle.jpeg_coefficients(img, q): [unit][64],
    unit = 3 * block + component, zig-zag order."""
    out = []
    prev = [0, 0, 0]
    for u, c in enumerate(np.asarray(coef, np.int64)):
        comp = u % 3
        diff = int(c[0]) - prev[comp]
        prev[comp] = int(c[0])
        s = _size(diff)
        out.append((2 if comp else 0, s, _value(diff, s), s))
        t = 3 if comp else 1
        last = 0
        for pos in np.nonzero(c[1:])[0] + 1:
            run = int(pos) - last - 1
            last = int(pos)
            while run > 15:
                out.append((t, 0xF0, 0, 0))
                run -= 16
            s = _size(c[pos])
            out.append((t, (run << 4) | s, _value(c[pos], s), s))
        if last != 63:
            out.append((t, 0x00, 0, 0))
    return out


def counts(syms):
    cnt = np.zeros((4, 256), np.uint32)
    for t, s, _, _ in syms:
        cnt[t, s] += 1
    return cnt


# ----------------------------------------------------------------------------------------------------------- the table rule --

def unlimited_depths(leaf_counts):
    """Minimum-redundancy depths (Moffat & Katajainen, in place) of counts in ascending order, two or more of them."""
    a = [int(x) for x in leaf_counts]
    n = len(a)
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            a[nxt] = a[root]; a[root] = nxt; root += 1
        else:
            a[nxt] = a[leaf]; leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]; a[root] = nxt; root += 1
        else:
            a[nxt] += a[leaf]; leaf += 1
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avbl, used, dpth, nxt, root = 1, 0, 0, n - 1, n - 2
    while avbl > 0:
        while root >= 0 and a[root] == dpth:
            used += 1; root -= 1
        while avbl > used:
            a[nxt] = dpth; nxt -= 1; avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    return a


def rule(cnt):
    """One table: counts[256] -> dict(lut uint32[256], num[17] codes per length, vals = the DHT's symbol list, folded = whether the
    16-bit limit bound)."""
    cnt = [int(x) for x in cnt]
    order = sorted((s for s in range(256) if cnt[s]), key=lambda s: (cnt[s], s))     # step 1; the reserved leaf goes in front
    lut, num = np.zeros(256, np.uint32), [0] * 34
    if not order:
        return dict(lut=lut, num=num[:17], vals=[], folded=False, lengths={})
    depths = unlimited_depths([1] + [cnt[s] for s in order])                         # step 2
    for d in depths:
        num[min(d, 33)] += 1
    folded = any(num[LIMIT + 1:])
    for i in range(LIMIT + 1, 34):                                                   # step 3
        num[LIMIT] += num[i]; num[i] = 0
    total = sum(num[i] << (LIMIT - i) for i in range(1, LIMIT + 1))
    while total > 1 << LIMIT:
        num[LIMIT] -= 1
        for i in range(LIMIT - 1, 0, -1):
            if num[i]:
                num[i] -= 1; num[i + 1] += 2
                break
        total -= 1
    num[max(i for i in range(1, LIMIT + 1) if num[i])] -= 1                          # step 4: the reserved leaf
    lengths, r = {}, 0
    for length in range(LIMIT, 0, -1):
        for _ in range(num[length]):
            lengths[order[r]] = length; r += 1
    assert r == len(order)
    code, vals = 0, []                                                               # step 5
    for length in range(1, LIMIT + 1):
        for s in sorted(s for s in lengths if lengths[s] == length):
            lut[s] = (length << 16) | code
            vals.append(s)
            code += 1
        code <<= 1
    return dict(lut=lut, num=num[:17], vals=vals, folded=folded, lengths=lengths)


def dht_segment(t, r):
    body = bytes([((t & 1) << 4) | (t >> 1)]) + bytes(r["num"][1:17]) + bytes(r["vals"])
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def standard_tables(header):
    """The four code tables of the DHT segments of a header (oracle.jpeg_header): the Annex K tables, as uint32[4][256]."""
    luts = np.zeros((4, 256), np.uint32)
    for marker, body in segments(header):
        if marker != 0xC4:
            continue
        t = ((body[0] >> 4) & 1) | ((body[0] & 15) << 1)
        code, k = 0, 17
        for length in range(1, 17):
            for _ in range(body[length]):
                luts[t, body[k]] = (length << 16) | code
                code += 1; k += 1
            code <<= 1
    return luts


def segments(data):
    """[(marker, body)] of the marker segments behind SOI up to and with SOS."""
    assert data[:2] == b"\xff\xd8"
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out


# ----------------------------------------------------------------------------------------------------------- the coder --

def code_scan(syms, luts):
    """BitWriter: codes and value bits most significant bit first, pad_byte (ones), 0xFF -> 0xFF00."""
    out = bytearray()
    acc = nbits = 0
    for t, s, value, vbits in syms:
        e = int(luts[t][s])
        assert e >> 16, (t, s)
        acc = (((acc << (e >> 16)) | (e & 0xFFFF)) << vbits) | value
        nbits += (e >> 16) + vbits
        while nbits >= 8:
            nbits -= 8
            b = (acc >> nbits) & 255
            out.append(b)
            if b == 255:
                out.append(0)
        acc &= (1 << nbits) - 1
    if nbits:
        b = ((acc << (8 - nbits)) | (0xFF >> nbits)) & 255
        out.append(b)
        if b == 255:
            out.append(0)
    return bytes(out)


def scan_bits(cnt, luts):
    """(code bits, value bits) of a scan with these counts under these tables"""
    code = sum(int(cnt[t, s]) * (int(luts[t][s]) >> 16) for t in range(4) for s in range(256) if cnt[t, s])
    value = sum(int(cnt[t, s]) * ((s & 15) if t & 1 else s) for t in range(4) for s in range(256))
    return code, value


def encode_with(header, coef, luts, dhts=None):
    """The file with the given tables; dhts = None keeps the header's own DHT segments."""
    head = header if dhts is None else header[:PREFIX_BYTES] + b"".join(dhts) + header[-SOS_BYTES:]
    return head + code_scan(symbols(coef), luts) + b"\xff\xd9"


def tables_of(cnt, std, fallback=False):
    """The rule and the decision for counts[4][256]; std = the Annex K tables (standard_tables).  -> dict(optimized, rules, luts = the
    picture's own tables, dht = its four DHT segments, own_bits / std_bits / value_bits, own_header)."""
    rules = [rule(cnt[t]) for t in range(4)]
    own = np.stack([r["lut"] for r in rules])
    own_bits, value = scan_bits(cnt, own)
    std_bits, _ = scan_bits(cnt, std)
    own_header = PREFIX_BYTES + sum(21 + len(r["vals"]) for r in rules) + SOS_BYTES
    on = (not fallback) and own_header <= STD_HEADER_BYTES and own_header + (own_bits + value + 7) // 8 < STD_HEADER_BYTES + (std_bits + value + 7) // 8
    return dict(optimized=on, rules=rules, luts=own, dht=b"".join(dht_segment(t, r) for t, r in enumerate(rules)), own_bits=own_bits, std_bits=std_bits,
                value_bits=value, own_header=own_header)


def encode(oracle, img, q, fallback=False):
    """(file, info) of FE_JPEG with FEO_JPEG_OPTIMIZE; info: tables_of's fields and the counts."""
    h, w = img.shape[:2]
    header = oracle.jpeg_header(w, h, q)
    assert len(header) == STD_HEADER_BYTES
    syms = symbols(oracle.jpeg_coefficients(img, q))
    cnt = counts(syms)
    std = standard_tables(header)
    info = tables_of(cnt, std, fallback)
    info["counts"] = cnt
    if not info["optimized"]:
        return header + code_scan(syms, std) + b"\xff\xd9", info
    return header[:PREFIX_BYTES] + info["dht"] + header[-SOS_BYTES:] + code_scan(syms, info["luts"]) + b"\xff\xd9", info
