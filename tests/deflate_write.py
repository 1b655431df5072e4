"""A token-level deflate writer (RFC 1951) for the streams zlib never writes: the caller chooses the tokens and, for a dynamic block,
the code lengths.  A token is an int (a literal byte) or a (length, distance) pair.  Blocks are appended to one Writer; zlib_stream
wraps the result (RFC 1950).  No compression is attempted: this is a test tool."""
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Writer:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        """n bits of value, lowest first (header fields and extra bits)"""
        self.bits.extend((value >> k) & 1 for k in range(n))

    def put_code(self, code, n):
        """a Huffman code, its top bit first"""
        self.bits.extend((code >> k) & 1 for k in range(n - 1, -1, -1))

    def align(self):
        self.bits.extend([0] * (-len(self.bits) % 8))

    def __len__(self):
        return len(self.bits)

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (0 = unused)"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


def balanced_lengths(used, nsym):
    """a complete code over the used symbols: lengths k - 1 and k (one used symbol: length 1, the incomplete code inflate accepts)"""
    used = sorted(set(used))
    out = [0] * nsym
    if len(used) == 1:
        out[used[0]] = 1
        return out
    k = max(1, (len(used) - 1).bit_length())
    short = (1 << k) - len(used)
    for i, s in enumerate(used):
        out[s] = k - 1 if i < short else k
    return out


def length_symbol(n):
    s = max(i for i in range(29) if LEN_BASE[i] <= n) if n < 258 else 28
    return s, n - LEN_BASE[s]


def dist_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, d - DIST_BASE[s]


def symbols_of(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, tuple):
            lit.add(257 + length_symbol(t[0])[0])
            dist.add(dist_symbol(t[1])[0])
        else:
            lit.add(t)
    return lit, dist


def put_tokens(w, tokens, lit_codes, dist_codes, end=True):
    for t in tokens:
        if isinstance(t, tuple):
            ls, le = length_symbol(t[0])
            w.put_code(*lit_codes[257 + ls])
            w.put(le, LEN_EXTRA[ls])
            ds, de = dist_symbol(t[1])
            w.put_code(*dist_codes[ds])
            w.put(de, DIST_EXTRA[ds])
        else:
            w.put_code(*lit_codes[t])
    if end:
        w.put_code(*lit_codes[256])


def stored_block(w, data, final=False):
    assert len(data) <= 65535
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xffff, 16)
    for b in data:
        w.put(b, 8)


def fixed_block(w, tokens, final=False):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def dynamic_block(w, tokens, final=False, lit_lengths=None, dist_lengths=None, end=True):
    """lit_lengths / dist_lengths: the code lengths to declare (lists; None = a balanced code over the symbols the tokens use).  The
    lengths are written one by one (code-length symbols 0..15, no run-length symbols)."""
    lit_used, dist_used = symbols_of(tokens)
    if lit_lengths is None:
        lit_lengths = balanced_lengths(lit_used, 286)
    if dist_lengths is None:
        dist_lengths = balanced_lengths(dist_used, 30) if dist_used else [0] * 30
    lit_lengths, dist_lengths = list(lit_lengths), list(dist_lengths)
    nlit = max(257, max(i for i, l in enumerate(lit_lengths) if l) + 1)
    ndist = max(1, max([i for i, l in enumerate(dist_lengths) if l], default=0) + 1)
    seq = lit_lengths[:nlit] + dist_lengths[:ndist]
    cl = balanced_lengths(seq, 19)
    ncl = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(nlit - 257, 5)
    w.put(ndist - 1, 5)
    w.put(ncl - 4, 4)
    for i in range(ncl):
        w.put(cl[CL_ORDER[i]], 3)
    cl_codes = canonical(cl)
    for l in seq:
        w.put_code(*cl_codes[l])
    put_tokens(w, tokens, canonical(lit_lengths), canonical(dist_lengths), end)


def expand(tokens, history=b""):
    """the bytes the tokens stand for, behind `history`"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(out)
            for _ in range(n):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out[len(history):])


def zlib_stream(w, raw, adler=None):
    """the Writer's blocks as a zlib stream; raw = what they inflate to (for the check value)"""
    check = zlib.adler32(raw) if adler is None else adler
    return b"\x78\x9c" + w.tobytes() + check.to_bytes(4, "big")
