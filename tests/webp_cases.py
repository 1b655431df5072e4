"""The lossless WebP files of tests/test_webp_source_host.py and tests/test_webp_source.py, by name: every writer configuration
(tests/vp8l_write.py) either test uses, and the Pillow corpus.  One registry, so the CPU test can hold every writer file against
libwebp and Pillow, and the GPU test decodes exactly the files that were proven valid there.

    CASES[name]()  ->  (file bytes, expected pixels (h, w, channels) or None = "what libwebp decodes")
    pillow_corpus() -> [(name, file bytes, the pixels Pillow was given)]"""
import io
import itertools
import os
import re

import numpy as np

import synth
import vp8l_write as vw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    text = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_webpdec.h")).read()
    return {k: int(v) for k, v in re.findall(r"(kWd(?:Waves|BandRows|Chunk|Lag)) = (\d+)", text)}


K = kernel_constants()
WAVES, BAND, CHUNK, LAG = K["kWdWaves"], K["kWdBandRows"], K["kWdChunk"], K["kWdLag"]
SKEW = 2 * (BAND - 1)
P, X, G, I = vw.PREDICTOR, vw.CROSS, vw.GREEN, vw.PALETTE


def rng(seed):
    return np.random.default_rng(seed)


def noise(h, w, seed, alpha=True):
    px = rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)
    if not alpha:
        px[..., 3] = 255
    return px


def smooth(h, w, seed):
    """RGBA with neighbours that resemble each other, so that Select and the clamped modes take both of their branches"""
    y, x = np.mgrid[0:h, 0:w]
    r = rng(seed).integers(-6, 7, (h, w, 4))
    base = np.stack([x * 5 + y * 2, 255 - x * 3 - y, (x * y) // 2 + 40, 200 - y * 4 + x], axis=2)
    return np.clip(base + r, 0, 255).astype(np.uint8)


MODE_CYCLE = [3, 5, 9, 10, 11, 12, 13, 0, 1, 2, 4, 6, 7, 8]


def mode_mix(w, h, bits, shift=0):
    """a mode per block that walks through all 14, the top-right ones (3, 5, 9, 10) first"""
    bw, bh = vw.subsample(w, bits), vw.subsample(h, bits)
    by, bx = np.mgrid[0:bh, 0:bw]
    return np.asarray(MODE_CYCLE)[(by * 5 + bx + shift) % 14]


def elements(w, h, bits, seed):
    bw, bh = vw.subsample(w, bits), vw.subsample(h, bits)
    return rng(seed).choice([-128, 127, -1, 0, 1, 64, -77], (bh, bw, 3))


def palette_picture(h, w, n, seed, beyond=False):
    """(pixels, palette ARGB, indices)"""
    r = rng(seed)
    pal = r.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    hi = n
    if beyond:
        hi = {3: 8, 2: 4, 1: 16, 0: 256}[vw.index_shift(n)] if n > 1 else 2
    idx = r.integers(0, hi, (h, w))
    if beyond:
        idx[0, 0] = hi - 1
    full = np.zeros(256, np.uint32)
    full[:n] = pal
    return vw.from_argb(full[idx]), pal, idx


CASES = {}


def case(name):
    def reg(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return reg


def add(name, fn):
    assert name not in CASES, name
    CASES[name] = fn


# ---- predictor modes ----------------------------------------------------------------------------------------------------------
SHAPES = {"37x21": (21, 37), "23x1": (1, 23), "1x23": (23, 1), "1x1": (1, 1)}
for m in range(14):
    for sname, (h, w) in SHAPES.items():
        def f(m=m, h=h, w=w):
            px = noise(h, w, 100 + m) if m < 11 else smooth(h, w, 100 + m)
            return vw.write(px, [(P, 2, m)]), px
        add(f"mode{m}_{sname}", f)
for m in (14, 15):
    add(f"mode{m}_37x21", lambda m=m: (vw.write(noise(21, 37, 120 + m), [(P, 2, m)]), None))   # expected: libwebp's decode
for bits in (2, 3):
    add(f"mode_mix_bits{bits}", lambda bits=bits: (lambda px: (vw.write(px, [(P, bits, rng(130 + bits).integers(0, 14, (vw.subsample(21, bits), vw.subsample(37, bits))))]), px))(smooth(21, 37, 130 + bits)))

# ---- block edges ----------------------------------------------------------------------------------------------------------------
for bits in (2, 3):
    sizes = [(1 << bits) * 2 - 1, (1 << bits) * 2, (1 << bits) * 2 + 1]
    for w, h in itertools.product(sizes, sizes):
        add(f"edge_bits{bits}_{w}x{h}", lambda bits=bits, w=w, h=h: (lambda px: (vw.write(px, [(P, bits, mode_mix(w, h, bits, w + h)), (X, bits, elements(w, h, bits, w * h))]), px))(smooth(h, w, 140 + w + h)))
add("edge_bits9_30x20", lambda: (lambda px: (vw.write(px, [(P, 9, 10), (X, 9, (127, -128, 5))]), px))(smooth(20, 30, 150)))

# ---- kernel boundaries ----------------------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
HEIGHTS = [1, 2, BAND - 1, BAND, BAND + 1, WAVES * BAND + 1, 2 * WAVES * BAND + 2]
LONG_W = LAG * WAVES * CHUNK - SKEW + CHUNK + 1   # a band then takes more chunk steps than LAG * WAVES


def boundary(w, h, seed):
    px = smooth(h, w, seed)
    return vw.write(px, [(P, 2, mode_mix(w, h, 2, seed))]), px


for w in WIDTHS:
    add(f"kernel_w{w}", lambda w=w: boundary(w, BAND + 3, 160 + w))
for h in HEIGHTS:
    add(f"kernel_h{h}", lambda h=h: boundary(3, h, 170 + h))
add("kernel_long_row", lambda: boundary(LONG_W, WAVES * BAND + 1, 180))
BIG = {"kernel_long_row"}   # too many pixels for the pixel-by-pixel numpy inverse: held against libwebp only on the CPU

# ---- pointwise transforms --------------------------------------------------------------------------------------------------------
add("cross_extreme", lambda: (lambda px: (vw.write(px, [(X, 2, rng(190).choice([-128, 127], (6, 10, 3)))]), px))(noise(21, 37, 190)))
add("add_green", lambda: (lambda px: (vw.write(px, [(G,)]), px))(noise(21, 37, 191)))
for n in (1, 2, 3, 4, 5, 16, 17, 256):
    for w in (1, 3, 7, 9):
        def f(n=n, w=w):
            px, pal, idx = palette_picture(5, w, n, 200 + n + w)
            return vw.write(px, [(I, pal, idx)]), px
        add(f"palette{n}_w{w}", f)
for n in (1, 3, 5, 17):
    def f(n=n):
        px, pal, idx = palette_picture(5, 9, n, 220 + n, beyond=True)
        return vw.write(px, [(I, pal, idx)], alpha_bit=1), px
    add(f"palette{n}_beyond", f)

# ---- every order of every subset ------------------------------------------------------------------------------------------------
ORDERS = [o for k in range(5) for c in itertools.combinations((P, X, G, I), k) for o in itertools.permutations(c)]
assert len(ORDERS) == 65


def order_case(order):
    """a 9 x 7 picture of six colours in patches.  Colour indexing that stands first takes the picture's own palette (two pixels a
    byte); behind other transforms it takes the colours their output has, and the transforms behind it run at the packed width."""
    px, pal, idx = palette_picture(7, 9, 6, 230)
    idx = np.repeat(np.repeat(idx[:3, :3], 3, 0), 3, 1)[:7, :9]
    full = np.zeros(256, np.uint32)
    full[:6] = pal
    px = vw.from_argb(full[idx])
    w, first = 9, True
    ts = []
    for t in order:
        if t == P: ts.append((P, 2, mode_mix(w, 7, 2, len(ts)) if w else 5))
        elif t == X: ts.append((X, 2, elements(w, 7, 2, 231) if w else (127, -128, 33)))
        elif t == G: ts.append((G,))
        elif first: ts.append((I, pal, idx)); w = vw.subsample(w, vw.index_shift(6))
        else: ts.append((I, None)); w = None   # (its packed width is known only to the writer: one mode / element for what follows)
        first = False
    return vw.write(px, ts, alpha_bit=1), px


for o in ORDERS:
    add("order_" + ("".join("PXGI"[t] for t in o) or "none"), lambda o=o: order_case(o))

# ---- channels ---------------------------------------------------------------------------------------------------------------------
for bit in (0, 1):
    for ext in (False, True):
        def f(bit=bit, ext=ext):
            px = noise(6, 11, 240)
            data = vw.write(px, [(G,), (P, 2, 11)], alpha_bit=bit if not ext else 1 - bit, extended=dict(alpha=bool(bit)) if ext else None)
            return data, px if bit else px[..., :3]
        add(f"channels_alpha{bit}_{'extended' if ext else 'simple'}", f)

# ---- the entropy stage: what the device never sees, for the host half ----------------------------------------------------------
def tiled(h=12, w=20, seed=250):
    return np.tile(rng(seed).integers(0, 256, (1, 5, 4)).astype(np.uint8), (h, w // 5, 1))


add("stream_cache1", lambda: (lambda px: (vw.write(px, cache_bits=1), px))(tiled()))
add("stream_cache4_transforms", lambda: (lambda px: (vw.write(px, [(G,), (P, 2, 11), (X, 3, (3, -7, 100))], cache_bits=4, sub_cache_bits=3), px))(smooth(21, 37, 251)))
add("stream_cache11", lambda: (lambda px: (vw.write(px, cache_bits=11), px))(np.tile(noise(5, 7, 252), (4, 5, 1))))
add("stream_groups", lambda: (lambda px: (vw.write(px, [(P, 3, 1)], entropy=(2, rng(253).integers(0, 5, (6, 10)))), px))(smooth(21, 37, 253)))
add("stream_groups_cache_refs", lambda: (lambda px: (vw.write(px, entropy=(3, np.arange(6).reshape(2, 3)), cache_bits=3, refs=[(5, 15, 5), (20, 20, 20), (60, 7, 40), (100, 60, 19 + 1)]), px))(tiled()))
add("stream_refs_map", lambda: (lambda px: (vw.write(px, refs=[(20, 5, 20), (25, 10, 5), (40, 30, 15), (80, 100, 40), (200, 40, 1 + 0 * 20 + 19)], use_map=True), px))(tiled()))
add("stream_refs_plain", lambda: (lambda px: (vw.write(px, refs=[(20, 5, 20), (25, 10, 5), (40, 30, 15), (80, 100, 40)], use_map=False), px))(tiled()))
add("stream_refs_max_length", lambda: (lambda px: (vw.write(px, refs=[(1, 4096, 1), (4097, 4096, 1), (8193, 64 * 129 - 8193, 4096)]), px))(np.full((64, 129, 4), 9, np.uint8)))
add("stream_normal_codes", lambda: (lambda px: (vw.write(px, [(P, 2, 2)], style="normal", rle=False), px))(noise(9, 13, 254)))
add("stream_normal_single_symbol", lambda: (lambda px: (vw.write(px, style="normal"), px))(np.full((4, 6, 4), 200, np.uint8)))
add("stream_simple_two_symbols", lambda: (lambda px: (vw.write(px, style="auto"), px))(np.where(rng(255).integers(0, 2, (8, 8, 1)) > 0, np.uint8(3), np.uint8(250)).repeat(4, 2)))
add("stream_max_symbol", lambda: (lambda px: (vw.write(px, [(G,)], max_symbol=True), px))((noise(9, 13, 256) // 4).astype(np.uint8)))

# ---- the extended container --------------------------------------------------------------------------------------------------------
def extended_file(before=(), after=(), alpha=True, seed=260):
    px = noise(5, 8, seed)
    return vw.write(px, [(G,)], extended=dict(alpha=alpha, before=list(before), after=list(after))), px if alpha else px[..., :3]


add("extended_plain", lambda: extended_file())
add("extended_iccp_xmp_unknown", lambda: extended_file(before=[(b"ICCP", b"not a profile, skipped"), (b"ABCD", b"odd")], after=[(b"XMP ", b"<x/>"), (b"EXIF", vw.exif(6))]))
for o in range(1, 9):
    add(f"extended_exif{o}_tiff", lambda o=o: extended_file(after=[(b"EXIF", vw.exif(o, big_endian=bool(o & 1)))], alpha=False))
    add(f"extended_exif{o}_prefixed", lambda o=o: extended_file(after=[(b"EXIF", vw.exif(o, prefix=True))]))


_cache = {}


def get(name):
    """(file, expected pixels): built once per process"""
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


# ---- files Pillow (libwebp's own encoder) writes ------------------------------------------------------------------------------------
def _save(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "WEBP", lossless=True, **kw)
    return b.getvalue()


_corpus = None


def pillow_corpus():
    global _corpus
    if _corpus is None:
        out = []
        for method in (0, 3, 6):
            rgb = synth.photo(96, 128, 3, index=method)
            rgba = synth.photo(96, 128, 4, index=10 + method).copy()
            rgba[..., 3] = np.maximum(rgba[..., 3], 1)   # (without exact=True the encoder may rewrite what alpha 0 hides)
            out.append((f"photo_rgb_m{method}", _save(rgb, method=method), rgb))
            out.append((f"photo_rgba_m{method}", _save(rgba, method=method), rgba))
        n = noise(40, 56, 270)
        n[::3, ::5, 3] = 0
        out.append(("noise_alpha0_exact", _save(n, exact=True, method=4), n))
        for k in (2, 4, 16, 200):
            pal = rng(271 + k).integers(0, 256, (k, 3)).astype(np.uint8)
            img = pal[rng(272 + k).integers(0, k, (48, 64))]
            out.append((f"palette{k}", _save(img, method=4), img))
        out.append(("flat", _save(np.full((48, 64, 3), (10, 200, 30), np.uint8), method=4), np.full((48, 64, 3), (10, 200, 30), np.uint8)))
        t = np.tile(rng(273).integers(0, 256, (16, 16, 3)).astype(np.uint8), (6, 8, 1))
        out.append(("tiled16", _save(t, method=4), t))
        _corpus = out
    return _corpus
