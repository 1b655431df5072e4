"""A small pure-Python reader of raw deflate streams (RFC 1951) that keeps what zlib's inflate throws away: the blocks, their
types, a dynamic block's three code-length arrays and the symbols themselves -- literals and (length, distance) pairs -- so that a
test can assert that an encoder really produced a given match (distance 32768, length 258) and which block carried BFINAL.

    blocks, end_bit = walk(raw_deflate_bytes)
    replay(blocks, history=b"") -> the bytes the blocks stand for

Meant for streams of a few tens of kilobytes: it decodes bit by bit."""

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

STORED, FIXED, DYNAMIC = 0, 1, 2


class DeflateError(ValueError):
    pass


class Block:
    """type: STORED / FIXED / DYNAMIC; final: its BFINAL bit; symbols: ints 0..255 and (length, distance) tuples (a stored block's
    bytes are listed as literals); cl_lens / lit_lens / dist_lens: a dynamic block's code-length code (19 entries, by symbol),
    literal/length code (HLIT entries) and distance code (HDIST entries), None otherwise; start_bit / end_bit: its extent."""

    def __init__(self, type, final, start_bit):
        self.type, self.final, self.start_bit, self.end_bit = type, final, start_bit, start_bit
        self.symbols = []
        self.cl_lens = self.lit_lens = self.dist_lens = None

    def matches(self):
        return [s for s in self.symbols if isinstance(s, tuple)]


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.n = data, 0, 8 * len(data)

    def take(self, k):
        if self.pos + k > self.n:
            raise DeflateError("stream ends inside a block")
        v = 0
        for i in range(k):
            p = self.pos + i
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << i
        self.pos += k
        return v


def _decoder(lens):
    """Canonical code of RFC 1951 3.2.2 as {(length, code): symbol}; over-subscribed sets are refused."""
    maxl = max(lens) if lens else 0
    count = [0] * (maxl + 1)
    for n in lens:
        if n:
            count[n] += 1
    code, nxt, kraft = 0, [0] * (maxl + 1), 0
    for n in range(1, maxl + 1):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
        kraft += count[n] << (maxl - n)
    if maxl and kraft > (1 << maxl):
        raise DeflateError("over-subscribed code")
    table = {}
    for s, n in enumerate(lens):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table, maxl


def _symbol(bits, dec):
    table, maxl = dec
    code = 0
    for n in range(1, maxl + 1):
        code = (code << 1) | bits.take(1)   # Huffman codes are packed most significant bit first
        s = table.get((n, code))
        if s is not None:
            return s
    raise DeflateError("bits that are no code")


_FIXED_LIT = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _decoder([5] * 30)


def walk(data, max_blocks=None):
    """Reads blocks up to and including the one with BFINAL (or until the bytes run out exactly at a block boundary, which is how
    a flushed, unfinished stream ends).  Returns (blocks, the bit position after the last block)."""
    bits, blocks = _Bits(data), []
    while True:
        blk = Block(None, None, bits.pos)
        blk.final = bool(bits.take(1))
        blk.type = bits.take(2)
        if blk.type == STORED:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xFFFF:
                raise DeflateError("stored block: LEN and NLEN disagree")
            start = bits.pos >> 3
            if start + n > len(data):
                raise DeflateError("stored block runs past the end")
            blk.symbols = list(data[start:start + n])
            bits.pos += 8 * n
        elif blk.type in (FIXED, DYNAMIC):
            if blk.type == DYNAMIC:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.take(3)
                cdec = _decoder(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, cdec)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise DeflateError("repeat with nothing before it")
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                if len(lens) != hlit + hdist:
                    raise DeflateError("code lengths run past HLIT + HDIST")
                blk.cl_lens, blk.lit_lens, blk.dist_lens = cl, lens[:hlit], lens[hlit:]
                if blk.lit_lens[256] == 0:
                    raise DeflateError("no end-of-block code")
                ldec, ddec = _decoder(blk.lit_lens), _decoder(blk.dist_lens)
            else:
                ldec, ddec = _FIXED_LIT, _FIXED_DIST
            while True:
                s = _symbol(bits, ldec)
                if s < 256:
                    blk.symbols.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise DeflateError("length symbol 286 or 287")
                    length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                    d = _symbol(bits, ddec)
                    if d > 29:
                        raise DeflateError("distance symbol 30 or 31")
                    blk.symbols.append((length, DIST_BASE[d] + bits.take(DIST_EXTRA[d])))
        else:
            raise DeflateError("block type 3")
        blk.end_bit = bits.pos
        blocks.append(blk)
        if blk.final or bits.pos == bits.n or (max_blocks and len(blocks) >= max_blocks):
            break
    return blocks, bits.pos


def replay(blocks, history=b""):
    """The bytes the blocks' symbols stand for, given the bytes before them."""
    out = bytearray(history)
    for blk in blocks:
        for s in blk.symbols:
            if isinstance(s, tuple):
                length, dist = s
                if dist > len(out):
                    raise DeflateError(f"distance {dist} reaches before the start")
                for _ in range(length):
                    out.append(out[-dist])
            else:
                out.append(s)
    return bytes(out[len(history):])
