"""A VP8L (lossless WebP) writer *from construction*, the counterpart of tests/png_write.py: given pixels it writes a file with
the transforms, block sizes, modes, elements, palette, colour cache, code groups, backward references, code-length coding and
container the test chose, so the expected pixels of a decode are the pixels the file was written from, not a decoder's.
`inverse(blob)` undoes the transforms of the blob csrc/fl_webpsrc.cpp leaves (header, sub-images, residuals) in numpy, so the
host half can be proven without a device.  Test infrastructure only; imports vp8l_model, does not change it.

    write(px, transforms=[...], ...)   the file for the (h, w, 4) RGBA pixels px
    container(payload, ...)            RIFF framing, simple or extended
    inverse(blob)                      (h, w, channels) pixels from a residual blob
    PLANE_CODES                        the 120-entry short-distance map as (dx, dy)"""
import struct

import numpy as np

import vp8l_model as vm

PREDICTOR, CROSS, GREEN, PALETTE = 0, 1, 2, 3
HEADER_DWORDS = 28   # csrc/fl_webpsrc.h WebpBlobHeader
MAGIC = 0x314C5057


def _plane_codes():
    """(dx, dy) per short-distance code 1..120, ordered by the format's rule: by Euclidean distance, ties ... -- the table is
    the specification's; distance = dy * xsize + dx."""
    t = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3),
         (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4),
         (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2),
         (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2),
         (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1),
         (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5),
         (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7),
         (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]
    assert len(t) == 120
    return t


PLANE_CODES = _plane_codes()


def plane_distance(xsize, code):
    if code > 120:
        return code - 120
    dx, dy = PLANE_CODES[code - 1]
    return max(dy * xsize + dx, 1)


def to_argb(px):
    px = np.asarray(px, np.uint32)
    return (px[..., 3] << 24) | (px[..., 0] << 16) | (px[..., 1] << 8) | px[..., 2]


def from_argb(argb, channels=4):
    argb = np.asarray(argb, np.uint32)
    out = np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255, argb >> 24], axis=-1).astype(np.uint8)
    return out[..., :channels]


def _ch(a):
    """(…,) uint32 -> (…, 4) int64 channels a, r, g, b"""
    a = np.asarray(a, np.int64)
    return np.stack([(a >> 24) & 255, (a >> 16) & 255, (a >> 8) & 255, a & 255], axis=-1)


def _unch(c):
    c = np.asarray(c, np.int64) & 255
    return ((c[..., 0] << 24) | (c[..., 1] << 16) | (c[..., 2] << 8) | c[..., 3]).astype(np.uint32)


def subsample(size, bits):
    return (size + (1 << bits) - 1) >> bits


def index_shift(n):
    return 3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0


# ---- the 14 predictors on channel arrays (…, 4): used forwards by the writer (all neighbours known), pixel by pixel by inverse() ----

def predict(mode, L, T, TR, TL):
    avg = lambda a, b: (a + b) >> 1
    clamp = lambda v: np.clip(v, 0, 255)
    if mode in (0, 14, 15):
        z = np.zeros_like(L)
        z[..., 0] = 255
        return z
    if mode == 1: return L
    if mode == 2: return T
    if mode == 3: return TR
    if mode == 4: return TL
    if mode == 5: return avg(avg(L, TR), T)
    if mode == 6: return avg(L, TL)
    if mode == 7: return avg(L, T)
    if mode == 8: return avg(TL, T)
    if mode == 9: return avg(T, TR)
    if mode == 10: return avg(avg(L, TL), avg(T, TR))
    if mode == 11:
        take_l = (np.abs(T - TL).sum(-1) < np.abs(L - TL).sum(-1))[..., None]
        return np.where(take_l, L, T)
    if mode == 12: return clamp(L + T - TL)
    if mode == 13:
        a = avg(L, T)
        d = a - TL
        return clamp(a + np.where(d < 0, -((-d) >> 1), d >> 1))   # C division: towards zero
    raise ValueError(mode)


def _mode_map(modes, bits, w, h):
    bw, bh = subsample(w, bits), subsample(h, bits)
    m = np.broadcast_to(np.asarray(modes, np.int64), (bh, bw)) if np.ndim(modes) else np.full((bh, bw), int(modes), np.int64)
    return m


def forward_predictor(argb, bits, modes):
    h, w = argb.shape
    m = _mode_map(modes, bits, w, h)
    per = np.repeat(np.repeat(m, 1 << bits, 0), 1 << bits, 1)[:h, :w].copy()
    per[0, :] = 1
    per[1:, 0] = 2
    per[0, 0] = 0
    flat = _ch(argb.reshape(-1))
    n = h * w
    idx = np.arange(n)
    nb = lambda off: flat[np.clip(idx + off, 0, n - 1)]
    L, T, TR, TL = nb(-1), nb(-w), nb(-w + 1), nb(-w - 1)
    pred = np.zeros_like(flat)
    pm = per.reshape(-1)
    for mode in np.unique(pm):
        sel = pm == mode
        pred[sel] = predict(int(mode), L[sel], T[sel], TR[sel], TL[sel])
    sub = np.zeros((m.shape[0], m.shape[1]), np.uint32) | 0xFF000000 | (m.astype(np.uint32) << 8)
    return _unch(flat - pred).reshape(h, w), sub


def _delta(t, c):
    t = np.asarray(t, np.int64); c = np.asarray(c, np.int64)
    s8 = lambda v: ((v & 255) ^ 128) - 128
    return (s8(t) * s8(c)) >> 5


def forward_cross(argb, bits, elements):
    h, w = argb.shape
    bw, bh = subsample(w, bits), subsample(h, bits)
    e = np.broadcast_to(np.asarray(elements, np.int64), (bh, bw, 3))   # (g2r, g2b, r2b), signed or unsigned bytes
    per = np.repeat(np.repeat(e, 1 << bits, 0), 1 << bits, 1)[:h, :w]
    c = _ch(argb)
    r = c[..., 1] - _delta(per[..., 0], c[..., 2])
    b = c[..., 3] - _delta(per[..., 1], c[..., 2]) - _delta(per[..., 2], c[..., 1])
    out = c.copy(); out[..., 1] = r; out[..., 3] = b
    sub = (0xFF000000 | ((e[..., 2] & 255) << 16) | ((e[..., 1] & 255) << 8) | (e[..., 0] & 255)).astype(np.uint32)
    return _unch(out), sub


def forward_green(argb):
    c = _ch(argb)
    c[..., 1] -= c[..., 2]; c[..., 3] -= c[..., 2]
    return _unch(c)


def forward_palette(argb, palette, indices=None):
    """palette: (n,) uint32 ARGB.  indices: explicit (h, w) indices (may lie beyond the palette), else looked up."""
    h, w = argb.shape
    palette = np.asarray(palette, np.uint32)
    if indices is None:
        lut = {int(v): i for i, v in reversed(list(enumerate(palette)))}
        indices = np.array([[lut[int(v)] for v in row] for row in argb], np.int64)
    indices = np.asarray(indices, np.int64)
    sh = index_shift(len(palette))
    per, bpp = 1 << sh, 8 >> sh
    pw_ = subsample(w, sh)
    packed = np.zeros((h, pw_), np.int64)
    for x in range(w):
        packed[:, x >> sh] |= (indices[:, x] & ((1 << bpp) - 1 if sh else 255)) << ((x & (per - 1)) * bpp)
    delta = palette.copy()
    c = _ch(palette)
    if len(palette) > 1:
        delta[1:] = _unch(c[1:] - c[:-1])
    return (0xFF000000 | (packed.astype(np.uint32) << 8)).astype(np.uint32), delta.reshape(1, -1)


# ---- prefix codes --------------------------------------------------------------------------------------------------------------

def _rle_tokens(lengths):
    """code lengths -> tokens (symbol, extra bits, extra value) with the repeat codes 16 / 17 / 18"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v = lengths[i]
        j = i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, 7, k - 11)); run -= k
            if run >= 3:
                out.append((17, 3, run - 3)); run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, 2, k - 3)); run -= k
            out += [(v, 0, 0)] * run
        i = j
    return out


def write_code(bw, hist, alphabet, style="auto", rle=True, max_symbol=False):
    """One prefix code for the symbols hist counts.  style: "auto" (simple where it fits), "normal" (always code-length coded,
    so a one-symbol code is a code of one length that consumes no bits), "simple".  Returns (lengths, reversed codes)."""
    used = [s for s in range(alphabet) if hist[s]]
    if not used:
        used = [0]
    simple_fits = len(used) <= 2 and used[-1] < 256 and (len(used) == 1 or True)
    if style == "simple":
        assert simple_fits
    if style != "normal" and simple_fits:
        lengths = [0] * alphabet
        bw.put(1, 1); bw.put(len(used) - 1, 1)
        if used[0] < 2:
            bw.put(0, 1); bw.put(used[0], 1)
        else:
            bw.put(1, 1); bw.put(used[0], 8)
        if len(used) == 2:
            bw.put(used[1], 8)
        if len(used) == 1:
            return lengths, [0] * alphabet
        for s in used:
            lengths[s] = 1
        return lengths, vm.canonical(lengths)
    if len(used) == 1:
        lengths = [0] * alphabet
        lengths[used[0]] = 1
    else:
        lengths = vm.huff_lengths([int(hist[s]) for s in range(alphabet)], 15)
    toks = _rle_tokens(lengths) if rle else [(v, 0, 0) for v in lengths]
    if max_symbol:
        while len(toks) > 2 and toks[-1][0] in (0, 17, 18):
            toks.pop()
    clh = [0] * 19
    for s, _, _ in toks:
        clh[s] += 1
    cl_len = vm.huff_lengths(clh, 7)
    cl_code = vm.canonical(cl_len)
    one = sum(1 for x in cl_len if x) == 1
    ncl = max(4, max(k + 1 for k, s in enumerate(vm.CL_ORDER) if cl_len[s]))
    bw.put(0, 1); bw.put(ncl - 4, 4)
    for s in vm.CL_ORDER[:ncl]:
        bw.put(cl_len[s], 3)
    if max_symbol:
        nb = 2
        while (len(toks) - 2) >> nb:
            nb += 2
        bw.put(1, 1); bw.put((nb - 2) // 2, 3); bw.put(len(toks) - 2, nb)
    else:
        bw.put(0, 1)
    for s, eb, ev in toks:
        if not one:
            bw.put(cl_code[s], cl_len[s])
        if eb:
            bw.put(ev, eb)
    if len(used) == 1:
        return [0] * alphabet, [0] * alphabet    # one symbol: no bits in the data
    return lengths, vm.canonical(lengths)


def _cache_key(argb, bits):
    return ((int(argb) * 0x1E35A7BD) & 0xFFFFFFFF) >> (32 - bits)


def encode_image(bw, argb, level0=False, cache_bits=0, entropy=None, refs=(), style="auto", rle=True, max_symbol=False, use_map=True):
    """One entropy-coded image.  entropy = (bits, group map (eh, ew)) for the main image; refs = [(position, length, distance)]
    in raster positions, checked against the pixels; a distance goes through the short-distance map where it has an entry
    (use_map) -- the first code whose clamped distance matches."""
    h, w = argb.shape
    flat = argb.reshape(-1)
    n = h * w
    bw.put(1 if cache_bits else 0, 1)
    if cache_bits:
        bw.put(cache_bits, 4)
    if level0:
        bw.put(1 if entropy else 0, 1)
    gidx = np.zeros(n, np.int64)
    ngroups = 1
    if entropy:
        ebits, gmap = entropy
        ew, eh = subsample(w, ebits), subsample(h, ebits)
        gmap = np.broadcast_to(np.asarray(gmap, np.int64), (eh, ew))
        bw.put(ebits - 2, 3)
        encode_image(bw, (0xFF000000 | (gmap.astype(np.uint32) << 8)).astype(np.uint32), style=style, rle=rle)
        gidx = np.repeat(np.repeat(gmap, 1 << ebits, 0), 1 << ebits, 1)[:h, :w].reshape(-1)
        ngroups = int(gmap.max()) + 1
    alpha0 = 280 + ((1 << cache_bits) if cache_bits else 0)
    sizes = (alpha0, 256, 256, 256, 40)
    fast = not refs and not cache_bits
    ch = _ch(flat)   # a, r, g, b
    hists = [[np.zeros(s, np.int64) for s in sizes] for _ in range(ngroups)]
    toks = []
    if fast:
        for g in range(ngroups):
            sel = gidx == g
            for k, c in ((0, 2), (1, 1), (2, 3), (3, 0)):
                hists[g][k][:256] += np.bincount(ch[sel, c], minlength=256)
    else:
        refs = {p: (ln, d) for p, ln, d in refs}
        cache = [0] * (1 << cache_bits) if cache_bits else None
        pos = 0
        while pos < n:
            g = int(gidx[pos])
            if pos in refs:
                ln, d = refs[pos]
                assert 1 <= d <= pos and pos + ln <= n and 1 <= ln <= 4096
                for k in range(ln):
                    assert flat[pos + k] == flat[pos + k - d], "the reference does not reproduce the pixels"
                code = d + 120
                if use_map:
                    for c in range(1, 121):
                        if plane_distance(w, c) == d:
                            code = c
                            break
                ls, lb, lv = vm.prefix_code(ln)
                ds, db, dv = vm.prefix_code(code)
                hists[g][0][256 + ls] += 1
                hists[g][4][ds] += 1
                toks.append((g, 1, (ls, lb, lv, ds, db, dv)))
                if cache_bits:
                    for k in range(ln):
                        cache[_cache_key(flat[pos + k], cache_bits)] = int(flat[pos + k])
                pos += ln
                continue
            v = int(flat[pos])
            if cache_bits and cache[_cache_key(v, cache_bits)] == v:
                key = _cache_key(v, cache_bits)
                hists[g][0][280 + key] += 1
                toks.append((g, 2, key))
            else:
                a, r, gr, b = (int(x) for x in ch[pos])
                hists[g][0][gr] += 1; hists[g][1][r] += 1; hists[g][2][b] += 1; hists[g][3][a] += 1
                toks.append((g, 0, (gr, r, b, a)))
            if cache_bits:
                cache[_cache_key(v, cache_bits)] = v
            pos += 1
    codes = [[write_code(bw, hists[g][k], sizes[k], style, rle, max_symbol and sizes[k] >= 256) for k in range(5)] for g in range(ngroups)]
    if fast:
        vals = np.zeros((n, 4), np.uint64)
        lens = np.zeros((n, 4), np.int64)
        for g in range(ngroups):
            sel = gidx == g
            for k, c in ((0, 2), (1, 1), (2, 3), (3, 0)):
                cl = np.asarray(codes[g][k][0], np.int64); cc = np.asarray(codes[g][k][1], np.uint64)
                vals[sel, k] = cc[ch[sel, c]]
                lens[sel, k] = cl[ch[sel, c]]
        bw.vals += vals.ravel().tolist(); bw.lens += lens.ravel().tolist()
        return
    for g, kind, t in toks:
        C = codes[g]
        if kind == 0:
            for k, s in enumerate(t):
                bw.put(C[k][1][s], C[k][0][s])
        elif kind == 2:
            bw.put(C[0][1][280 + t], C[0][0][280 + t])
        else:
            ls, lb, lv, ds, db, dv = t
            bw.put(C[0][1][256 + ls], C[0][0][256 + ls]); bw.put(lv, lb)
            bw.put(C[4][1][ds], C[4][0][ds]); bw.put(dv, db)


def payload(px, transforms=(), alpha_bit=None, version=0, signature=0x2F, **main):
    """The VP8L chunk payload for RGBA pixels px (h, w, 4).  transforms, in stream order:
        (PREDICTOR, bits, modes)   modes: one mode or a (bh, bw) array
        (CROSS, bits, elements)    elements: (g2r, g2b, r2b) or a (bh, bw, 3) array
        (GREEN,)
        (PALETTE, palette[, indices])   palette: (n,) ARGB dwords, or None = the colours the picture has where the transform stands;
                                        indices: explicit (h, w), may lie beyond the palette
    main: cache_bits, entropy, refs, style, rle, max_symbol, use_map for the main image; sub_cache_bits for the sub-images."""
    px = np.asarray(px, np.uint8)
    h, w, _ = px.shape
    argb = to_argb(px)
    if alpha_bit is None:
        alpha_bit = int((px[..., 3] != 255).any())
    sub_cache = main.pop("sub_cache_bits", 0)
    sub_style = {k: main[k] for k in ("style", "rle") if k in main}
    bw = vm.BitWriter()
    bw.put(signature, 8); bw.put(w - 1, 14); bw.put(h - 1, 14); bw.put(alpha_bit, 1); bw.put(version, 3)
    for t in transforms:
        bw.put(1, 1); bw.put(t[0], 2)
        if t[0] == PREDICTOR:
            argb, sub = forward_predictor(argb, t[1], t[2])
            bw.put(t[1] - 2, 3)
            encode_image(bw, sub, cache_bits=sub_cache, **sub_style)
        elif t[0] == CROSS:
            argb, sub = forward_cross(argb, t[1], t[2])
            bw.put(t[1] - 2, 3)
            encode_image(bw, sub, cache_bits=sub_cache, **sub_style)
        elif t[0] == GREEN:
            argb = forward_green(argb)
        else:
            pal = t[1] if t[1] is not None else np.unique(argb)   # None: the colours the picture has at this point of the list
            assert len(pal) <= 256
            argb, sub = forward_palette(argb, pal, t[2] if len(t) > 2 else None)
            bw.put(len(pal) - 1, 8)
            encode_image(bw, sub, **sub_style)
    bw.put(0, 1)
    encode_image(bw, argb, level0=True, **main)
    data, _ = vm.pack(bw.vals, bw.lens)
    return data


def chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def container(vp8l, extended=None, size=None):
    """RIFF framing.  extended = dict(width, height, alpha=bool, before=[(tag, body)], after=[(tag, body)], flags=extra VP8X flag bits)"""
    if extended is None:
        body = chunk(b"VP8L", vp8l)
    else:
        w, h = extended["width"], extended["height"]
        before, after = extended.get("before", []), extended.get("after", [])
        flags = extended.get("flags", 0) | (0x10 if extended.get("alpha") else 0)
        for tag, _ in before + after:
            flags |= {b"ICCP": 0x20, b"EXIF": 0x08, b"XMP ": 0x04}.get(tag, 0)
        x = bytes([flags, 0, 0, 0]) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3]
        body = chunk(b"VP8X", x) + b"".join(chunk(t, b) for t, b in before) + chunk(b"VP8L", vp8l) + b"".join(chunk(t, b) for t, b in after)
    return b"RIFF" + struct.pack("<I", 4 + len(body) if size is None else size) + b"WEBP" + body


def write(px, transforms=(), extended=None, **kw):
    px = np.asarray(px, np.uint8)
    if extended is not None:
        extended = dict(extended, width=px.shape[1], height=px.shape[0])
    return container(payload(px, transforms, **kw), extended)


def exif(orientation, prefix=False, big_endian=False):
    """An EXIF payload with the Orientation tag: at the TIFF header (the usual WebP form) or behind "Exif\\0\\0"."""
    e = ">" if big_endian else "<"
    tiff = (b"MM\0*" if big_endian else b"II*\0") + struct.pack(e + "I", 8) + struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", 0x0112, 3, 1, orientation, 0) + struct.pack(e + "I", 0)
    return (b"Exif\0\0" if prefix else b"") + tiff


# ---- the blob of csrc/fl_webpsrc.cpp, undone in numpy --------------------------------------------------------------------------

def blob_header(blob):
    d = np.frombuffer(blob[:HEADER_DWORDS * 4], np.uint32)
    assert d[0] == MAGIC
    return {"width": int(d[1]), "height": int(d[2]), "channels": int(d[3]), "ntransforms": int(d[4]), "ttype": d[5:9].tolist(), "tbits": d[9:13].tolist(),
            "twidth": d[13:17].tolist(), "toff": d[17:21].tolist(), "xsize": int(d[21]), "res_off": int(d[22]), "total_bytes": int(d[23])}


def _predict_scalar(mode, L, T, TR, TL):
    """predict() on four-int lists: the same 14 rules, for the pixel-by-pixel inverse"""
    avg = lambda a, b: [(x + y) >> 1 for x, y in zip(a, b)]
    clamp = lambda v: 0 if v < 0 else 255 if v > 255 else v
    if mode in (0, 14, 15): return [255, 0, 0, 0]
    if mode == 1: return L
    if mode == 2: return T
    if mode == 3: return TR
    if mode == 4: return TL
    if mode == 5: return avg(avg(L, TR), T)
    if mode == 6: return avg(L, TL)
    if mode == 7: return avg(L, T)
    if mode == 8: return avg(TL, T)
    if mode == 9: return avg(T, TR)
    if mode == 10: return avg(avg(L, TL), avg(T, TR))
    if mode == 11:
        return L if sum(abs(t - c) for t, c in zip(T, TL)) < sum(abs(l - c) for l, c in zip(L, TL)) else T
    if mode == 12: return [clamp(l + t - c) for l, t, c in zip(L, T, TL)]
    a = avg(L, T)
    return [clamp(x + int((x - c) / 2)) for x, c in zip(a, TL)]


def _inverse_predictor(res, modes, bits):
    h, w = res.shape
    r = _ch(res.reshape(-1)).tolist()
    out = [None] * (h * w)
    mrow = ((modes >> 8) & 15).astype(np.int64).tolist()
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                p = [255, 0, 0, 0] if x == 0 else out[i - 1]
            elif x == 0:
                p = out[i - w]
            else:
                p = _predict_scalar(mrow[y >> bits][x >> bits], out[i - 1], out[i - w], out[i - w + 1], out[i - w - 1])
            out[i] = [(a + b) & 255 for a, b in zip(r[i], p)]
    return _unch(np.asarray(out, np.int64)).reshape(h, w)


def inverse(blob):
    """The decoded picture (h, w, channels) from a residual blob: the transforms inverted last to first, pixel by pixel."""
    H = blob_header(blob)
    h = H["height"]
    assert len(blob) == H["total_bytes"]
    img = np.frombuffer(blob, np.uint32, H["xsize"] * h, H["res_off"]).reshape(h, H["xsize"]).copy()
    for k in reversed(range(H["ntransforms"])):
        t, bits, tw, off = H["ttype"][k], H["tbits"][k], H["twidth"][k], H["toff"][k]
        if t == PALETTE:
            pal = np.frombuffer(blob, np.uint32, 256, off)
            sh = index_shift(bits)
            assert img.shape[1] == subsample(tw, sh), "packed width"
            bpp, per = 8 >> sh, 1 << sh
            x = np.arange(tw)
            g = (img[:, x >> sh] >> 8) & 255
            img = pal[(g >> ((x & (per - 1)) * bpp)) & ((1 << bpp) - 1)]
            continue
        assert img.shape[1] == tw
        if t == GREEN:
            c = _ch(img)
            c[..., 1] += c[..., 2]; c[..., 3] += c[..., 2]
            img = _unch(c)
            continue
        bw_, bh_ = subsample(tw, bits), subsample(h, bits)
        sub = np.frombuffer(blob, np.uint32, bw_ * bh_, off).reshape(bh_, bw_)
        if t == PREDICTOR:
            img = _inverse_predictor(img, sub, bits)
        else:
            per = np.repeat(np.repeat(sub, 1 << bits, 0), 1 << bits, 1)[:h, :tw].astype(np.int64)
            c = _ch(img)
            c[..., 1] = (c[..., 1] + _delta(per & 255, c[..., 2])) & 255
            c[..., 3] += _delta((per >> 8) & 255, c[..., 2]) + _delta((per >> 16) & 255, c[..., 1])
            img = _unch(c)
    assert img.shape == (h, H["width"])
    return from_argb(img, H["channels"])
