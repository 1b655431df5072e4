"""A numpy restatement of the lossless WebP stream FLGPU_FE_WEBP_LOSSLESS writes (fanlin-rs_amd/csrc/fl_webpll.hip), the
layout of `image-webp 0.2.1`'s encoder as DESIGN.md records it (reference src/handler.rs:286-292): subtract-green, a
predictor transform that is T everywhere (L on row 0), one prefix-code group, no colour cache, runs of the previous pixel
as the only backward references.  Test infrastructure only.

    encode(px)        the file for the FE_NONE pixels px (h, w, c), c in 1..4
    into_rgba8(px)    DynamicImage::into_rgba8 of those pixels
    decode_rgba(data) libwebp's decoder (WebPDecodeRGBA, or Pillow if it cannot be loaded), (h, w, 4)
    parse(data)       reads the headers back: transforms, the codes' kinds and lengths, where the pixel data starts"""
import ctypes as C
import ctypes.util
import io
import struct

import numpy as np

MAX_RUN = 4096
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
ALPHABETS = (280, 256, 256, 256)  # green + lengths, red, blue, alpha (the distance code is always symbol 1)


def into_rgba8(px):
    px = np.asarray(px, np.uint8)
    h, w, c = px.shape
    if c == 4:
        return px.copy()
    out = np.empty((h, w, 4), np.uint8)
    if c in (1, 2):
        out[..., 0] = out[..., 1] = out[..., 2] = px[..., 0]
        out[..., 3] = px[..., 1] if c == 2 else 255
    else:
        out[..., :3] = px
        out[..., 3] = 255
    return out


def residuals(px):
    """(h * w, 4) uint8 residuals (a, r, g, b) after subtract-green and the predictor transform, raster order."""
    rgba = into_rgba8(px).astype(np.int32)
    h, w, _ = rgba.shape
    g = rgba[..., 1]
    argb = np.stack([rgba[..., 3], (rgba[..., 0] - g) & 255, g, (rgba[..., 2] - g) & 255], axis=-1)
    pred = np.zeros_like(argb)
    pred[1:] = argb[:-1]                  # T for every later row, column 0 included
    pred[0, 1:] = argb[0, :-1]            # L on row 0
    pred[0, 0] = (255, 0, 0, 0)           # ARGB black for the first pixel
    return ((argb - pred) & 255).astype(np.uint8).reshape(h * w, 4)


def prefix_code(v):
    """VP8L prefix coding of v >= 1 (a length or distance): (symbol, extra bits, extra value)."""
    x = v - 1
    if x < 4:
        return x, 0, 0
    nb = x.bit_length() - 1
    return 2 * nb + ((x >> (nb - 1)) & 1), nb - 1, x & ((1 << (nb - 1)) - 1)


def tokens(res):
    """(kind, length) per pixel: kind 1 = literal, 2 = backward reference of distance 1 ending here, 0 = inside one."""
    n = len(res)
    key = res.view(np.uint32).reshape(n) if res.dtype == np.uint8 and res.ndim == 2 else res
    idx = np.arange(n, dtype=np.int64)
    flag = np.ones(n, bool)
    flag[1:] = key[1:] != key[:-1]
    start = np.maximum.accumulate(np.where(flag, idx, 0))
    m = (idx - start) % (MAX_RUN + 1)
    last = np.ones(n, bool)
    last[:-1] = flag[1:]
    lit = m == 0
    ref = (m != 0) & ((m == MAX_RUN) | last)
    return lit, ref, m


def huff_lengths(hist, limit):
    """fl_webpll.hip's huff_build (the Moffat-Katajainen builder of fl_png.hip folded to `limit` bits), restated."""
    used = sorted((int(f), s) for s, f in enumerate(hist) if f)
    n = len(used)
    lengths = [0] * len(hist)
    if n == 0:
        return lengths
    A = [f for f, _ in used]
    syms = [s for _, s in used]
    num = [0] * 34
    if n == 1:
        num[1] = 1
    else:
        A[0] += A[1]
        root, leaf = 0, 2
        for nxt in range(1, n - 1):
            if leaf >= n or A[root] < A[leaf]:
                A[nxt] = A[root]; A[root] = nxt; root += 1
            else:
                A[nxt] = A[leaf]; leaf += 1
            if leaf >= n or (root < nxt and A[root] < A[leaf]):
                A[nxt] += A[root]; A[root] = nxt; root += 1
            else:
                A[nxt] += A[leaf]; leaf += 1
        A[n - 2] = 0
        for nxt in range(n - 3, -1, -1):
            A[nxt] = A[A[nxt]] + 1
        avbl, usedc, dpth, nxt, root = 1, 0, 0, n - 1, n - 2
        while avbl > 0:
            while root >= 0 and A[root] == dpth:
                usedc += 1; root -= 1
            while avbl > usedc:
                A[nxt] = dpth; nxt -= 1; avbl -= 1
            avbl, dpth, usedc = 2 * usedc, dpth + 1, 0
        for i in range(n):
            num[min(A[i], 33)] += 1
        for i in range(limit + 1, 34):
            num[limit] += num[i]; num[i] = 0
        total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
        while total > (1 << limit):
            num[limit] -= 1
            for i in range(limit - 1, 0, -1):
                if num[i]:
                    num[i] -= 1; num[i + 1] += 2
                    break
            total -= 1
    j = n
    for ln in range(1, limit + 1):
        for _ in range(num[ln]):
            j -= 1
            lengths[syms[j]] = ln
    return lengths


def unlimited_depth(hist):
    """The longest code of the Moffat-Katajainen lengths before any fold (33 bits is past every depth a test histogram reaches)."""
    depth = max(huff_lengths(list(hist), 33))
    assert depth < 33
    return depth


def canonical(lengths):
    """Canonical codes (the deflate rule), bit-reversed for the LSB-first stream."""
    maxl = max(lengths) if lengths else 0
    bl = [0] * (maxl + 2)
    for ln in lengths:
        if ln:
            bl[ln] += 1
    code, nxt = 0, [0] * (maxl + 2)
    for ln in range(1, maxl + 1):
        code = (code + bl[ln - 1]) << 1
        nxt[ln] = code
    out = [0] * len(lengths)
    for s, ln in enumerate(lengths):
        if ln:
            v = nxt[ln]; nxt[ln] += 1
            out[s] = int("{:0{}b}".format(v, ln)[::-1], 2)
    return out


class BitWriter:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, v, n):
        self.vals.append(v); self.lens.append(n)

    def bits(self):
        return sum(self.lens)


def pack(vals, lens):
    """LSB-first packing of (value, bit count) items, vectorised."""
    vals = np.asarray(vals, np.uint64).ravel()
    lens = np.asarray(lens, np.int64).ravel()
    total = int(lens.sum())
    pos = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else np.zeros(0, np.int64)
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    for b in range(int(lens.max()) if len(lens) else 0):
        sel = lens > b
        bits[pos[sel] + b] = (vals[sel] >> np.uint64(b)) & np.uint64(1)
    return np.packbits(bits, bitorder="little").tobytes(), total


def write_simple(bw, sym):
    bw.put(1, 1); bw.put(0, 1)
    if sym < 2:
        bw.put(0, 1); bw.put(sym, 1)
    else:
        bw.put(1, 1); bw.put(sym, 8)


def write_code(bw, hist, alphabet):
    """One prefix code; returns (lengths, reversed codes) for the data that follows."""
    used = [s for s in range(alphabet) if hist[s]]
    if len(used) <= 1:
        write_simple(bw, used[0] if used else 0)
        return [0] * alphabet, [0] * alphabet
    lengths = huff_lengths(list(hist[:alphabet]), 15)
    codes = canonical(lengths)
    clh = [0] * 19
    for ln in lengths:
        clh[ln] += 1
    cl_len = huff_lengths(clh, 7)
    cl_code = canonical(cl_len)
    one = sum(1 for x in cl_len if x) == 1
    bw.put(0, 1)
    bw.put(15, 4)
    for s in CL_ORDER:
        bw.put(cl_len[s], 3)
    if alphabet == 256:
        bw.put(1, 1); bw.put(3, 3); bw.put(254, 8)
    else:
        bw.put(0, 1)
    if not one:
        for ln in lengths:
            bw.put(cl_code[ln], cl_len[ln])
    return lengths, codes


def header(w, h, hists):
    """The VP8L bit stream up to the pixel data, and the four codes."""
    bw = BitWriter()
    bw.put(0x2F, 8); bw.put(w - 1, 14); bw.put(h - 1, 14); bw.put(1, 1); bw.put(0, 3)
    bw.put(0b101, 3)                       # subtract green
    bw.put(0b111001, 6)                    # predictor, 2^9 blocks
    bw.put(0, 1)                           # sub-image: no colour cache
    write_simple(bw, 2)                    # mode T
    for _ in range(4):
        write_simple(bw, 0)
    bw.put(0, 1); bw.put(0, 1); bw.put(0, 1)  # no more transforms, no colour cache, no meta prefix codes
    codes = [write_code(bw, hists[k], ALPHABETS[k]) for k in range(4)]
    write_simple(bw, 1)                    # distance: plane code 2, the left pixel
    return bw, codes


def histograms(res, lit, ref, m):
    a, r, g, b = (res[lit, k].astype(np.int64) for k in range(4))
    hg = np.bincount(g, minlength=280)
    lsym = np.array([prefix_code(int(v))[0] for v in m[ref]], np.int64)
    if len(lsym):
        hg += np.bincount(256 + lsym, minlength=280)
    return [hg, np.bincount(r, minlength=256), np.bincount(b, minlength=256), np.bincount(a, minlength=256)]


def encode(px):
    px = np.asarray(px, np.uint8)
    if px.ndim == 2:
        px = px[..., None]
    h, w, _ = px.shape
    assert 1 <= w <= 16384 and 1 <= h <= 16384
    res = residuals(px)
    lit, ref, m = tokens(res)
    hists = histograms(res, lit, ref, m)
    bw, codes = header(w, h, hists)
    n = len(res)
    vals = np.zeros((n, 5), np.uint64)
    lens = np.zeros((n, 5), np.int64)
    # literal: green, red, blue, alpha
    for slot, k in ((0, 2), (1, 1), (2, 3), (3, 0)):
        cl = np.asarray(codes[(0, 1, 2, 3)[slot]][0], np.int64)
        cc = np.asarray(codes[(0, 1, 2, 3)[slot]][1], np.uint64)
        sym = res[lit, k].astype(np.int64)
        vals[lit, slot] = cc[sym]
        lens[lit, slot] = cl[sym]
    # reference: length symbol, extra bits (the distance code costs nothing)
    if ref.any():
        cl = np.asarray(codes[0][0], np.int64)
        cc = np.asarray(codes[0][1], np.uint64)
        pc = [prefix_code(int(v)) for v in m[ref]]
        sym = np.array([256 + p[0] for p in pc], np.int64)
        vals[ref, 0] = cc[sym]
        lens[ref, 0] = cl[sym]
        vals[ref, 1] = np.array([p[2] for p in pc], np.uint64)
        lens[ref, 1] = np.array([p[1] for p in pc], np.int64)
    data, nbits = pack(np.concatenate([np.asarray(bw.vals, np.uint64), vals.ravel()]),
                       np.concatenate([np.asarray(bw.lens, np.int64), lens.ravel()]))
    body = data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 12 + len(body)) + b"WEBP" + b"VP8L" + struct.pack("<I", len(data)) + body


def max_out_bytes(w, h):
    """fl_webpll.h webpll_max_out_bytes: 1024 + ceil(15 w h / 2)."""
    return 1024 + (15 * w * h + 1) // 2


# ----------------------------------------------------------------------------------------------------- decoding --

_webp = None


def _libwebp():
    global _webp
    if _webp is None:
        _webp = False
        for name in (ctypes.util.find_library("webp"), "libwebp.so.7", "libwebp.so"):
            if not name:
                continue
            try:
                lib = C.CDLL(name)
            except OSError:
                continue
            lib.WebPDecodeRGBA.restype = C.POINTER(C.c_uint8)
            lib.WebPDecodeRGBA.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            lib.WebPFree.argtypes = [C.c_void_p]
            _webp = lib
            break
    return _webp or None


def have_decoder():
    if _libwebp():
        return True
    try:
        from PIL import features
        return bool(features.check("webp"))
    except ImportError:
        return False


def decode_rgba(data):
    lib = _libwebp()
    if lib:
        w, h = C.c_int(), C.c_int()
        p = lib.WebPDecodeRGBA(data, len(data), C.byref(w), C.byref(h))
        if not p:
            raise ValueError("libwebp refused the stream")
        try:
            return np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
        finally:
            lib.WebPFree(p)
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))


# ------------------------------------------------------------------------------------------------------ parsing --

class BitReader:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def get(self, n):
        v = 0
        for i in range(n):
            byte = self.data[(self.pos + i) >> 3]
            v |= ((byte >> ((self.pos + i) & 7)) & 1) << i
        self.pos += n
        return v


def _read_code(br, alphabet):
    if br.get(1):
        n = br.get(1) + 1
        syms = [br.get(8 if br.get(1) else 1)]
        if n == 2:
            syms.append(br.get(8))
        return {"simple": syms}
    ncl = br.get(4) + 4
    cl = [0] * 19
    for k in range(ncl):
        cl[CL_ORDER[k]] = br.get(3)
    max_symbol = alphabet
    if br.get(1):
        nb = 2 + 2 * br.get(3)
        max_symbol = 2 + br.get(nb)
    used = [s for s in range(19) if cl[s]]
    lengths = []
    if len(used) == 1:
        lengths = [used[0]] * max_symbol
    else:
        codes = canonical(cl)
        table = {(cl[s], codes[s]): s for s in used}
        for _ in range(max_symbol):
            v, n = 0, 0
            while (n, v) not in table:
                v |= br.get(1) << n
                n += 1
                assert n <= 7, "bad code-length code"
            s = table[(n, v)]
            assert s < 16, "repeat codes are not used"
            lengths.append(s)
    return {"cl_lengths": cl, "num_cl": ncl, "max_symbol": max_symbol, "lengths": lengths}


def parse(data):
    """Container and headers of a stream this encoder wrote, read back field by field."""
    assert data[:4] == b"RIFF" and data[8:16] == b"WEBPVP8L"
    riff, = struct.unpack("<I", data[4:8])
    n, = struct.unpack("<I", data[16:20])
    assert riff == len(data) - 8 and len(data) == 20 + n + (n & 1)
    br = BitReader(data[20:20 + n])
    out = {"signature": br.get(8), "width": br.get(14) + 1, "height": br.get(14) + 1, "alpha": br.get(1), "version": br.get(3)}
    transforms = []
    while br.get(1):
        t = br.get(2)
        if t == 0:
            bits = br.get(3) + 2
            cache = br.get(1)
            sub = [_read_code(br, a) for a in (280, 256, 256, 256, 40)]
            transforms.append(("predictor", bits, cache, sub))
        else:
            transforms.append(({1: "cross-colour", 2: "subtract-green", 3: "colour-indexing"}[t],))
            assert t == 2, "only subtract-green and predictor are written"
    out["transforms"] = transforms
    out["colour_cache"] = br.get(1)
    out["meta_prefix"] = br.get(1)
    out["codes"] = [_read_code(br, a) for a in (280, 256, 256, 256, 40)]
    out["data_bit"] = br.pos
    return out
