"""The lossy WebP decoder's corpus, built at test time and deterministic (tests/test_vp8_source_host.py, tests/test_vp8_source.py).

Two sources of files:
  * tests/vp8_model.py writes valid key frames with an exactly known Y / U / V reconstruction and needs no library: the frame
    sizes at the macroblock edges, 1 / 2 / 4 / 8 token partitions, the ends of the quantiser scale, a raw ALPH chunk -- and, with
    the plane filtered here in numpy and spliced in, ALPH filters 1, 2 and 3 (libwebp picks the filter itself);
  * libwebp through ctypes (tests/vp8_dec_lib.py) writes what the model does not: B_PRED macroblocks, segments, both loop filters,
    sharpness, probability updates.  Expected planes: WebPDecodeYUV; expected pixels: WebPDecodeRGB / WebPDecodeRGBA.
Both also hold the sizes at which the device's scheduling (csrc/fl_vp8dec.hip) takes a second chunk, round or band: SCHEDULING.

get(name) -> dict(data, yuv, pixels, channels): yuv = the expected (y, u, v), pixels = the expected Rgb8 / Rgba8 picture or None
where libwebp is not there to say (a model file's planes are the model's own).  Contents and seeds are fixed: the coverage the
decoder's tests rely on is asserted there on flgpu_vp8_info_of's fields, not hoped for."""
import functools
import re

import numpy as np

import synth
import vp8_dec_lib
import vp8_model
import vp8l_write

MODEL, LIBWEBP = {}, {}


def have_libwebp():
    return vp8_dec_lib.load() is not None


# ---- contents ---------------------------------------------------------------------------------------------------------------------

def textured(h, w, seed, alpha=None):
    """a photograph-like picture with noise on it: libwebp codes it with B_PRED and one-mode macroblocks, segments and large levels"""
    rng = np.random.default_rng(seed)
    img = synth.photo(h, w, 3, index=seed).astype(np.int32) + rng.integers(-40, 40, (h, w, 3))
    a = np.full((h, w), 255, np.uint8) if alpha is None else alpha
    return np.dstack([np.clip(img, 0, 255).astype(np.uint8), a])


def quilt(h, w, seed):
    """textured() with every other macroblock flat, as a chequerboard: at 1040 x 528 libwebp codes textured() itself with B_PRED
    in every macroblock; here half are one-mode ones, and along an anti-diagonal (x - 2, y + 1) the two kinds alternate"""
    img = textured(h, w, seed)
    y, x = np.mgrid[0:h, 0:w]
    flat = (x // 16 + y // 16) % 2 == 1
    for k, v in enumerate(((x // 16) * 37 % 256, (y // 16) * 53 % 256, (x // 16 + y // 16) * 29 % 256)):
        img[..., k][flat] = v[flat]
    return img


def bars(h, w, seed):
    """flat bars beside noise and a gradient: skipped macroblocks, every one-mode prediction, quiet and busy segments"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3), np.int32)
    img[..., 0] = (x // 24) * 60 % 256
    img[..., 1] = (y // 20) * 45 % 256
    img[..., 2] = (x * 255) // max(w - 1, 1)
    busy = (x > w // 2) & (y > h // 3)
    img[busy] += rng.integers(-90, 90, (int(busy.sum()), 3))
    return np.dstack([np.clip(img, 0, 255).astype(np.uint8), np.full((h, w), 255, np.uint8)])


def quiet_and_noise(h, w, seed, gradient):
    """the left half flat or a slow diagonal gradient, the right half noise: at methods 0..2 libwebp flags the quiet macroblocks
    as skipped -- one-mode ones, and with the gradient B_PRED ones too (directional modes, no coefficients)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.full((h, w, 3), 100, np.int32)
    if gradient:
        img[...] = (((x + y) * 255) // (h + w))[..., None]
    img[:, w // 2:] = rng.integers(0, 255, (h, w - w // 2, 3))
    return np.dstack([img.astype(np.uint8), np.full((h, w), 255, np.uint8)])


def ramp_alpha(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 5 + y * 3) % 256).astype(np.uint8)


def ramp(a, b):
    """the plane (a x + b y) % 256 as a function of (h, w); ramp_alpha is ramp(5, 3)"""
    def plane(h, w):
        y, x = np.mgrid[0:h, 0:w]
        return ((x * a + y * b) % 256).astype(np.uint8)
    return plane


def slope_alpha(h, w):
    """a slow ramp: runs of equal samples along both axes"""
    y, x = np.mgrid[0:h, 0:w]
    return ((2 * x + 3 * y) // 4 % 256).astype(np.uint8)


def bowl_alpha(h, w):
    """second-order in x and y: the gradient predictor's kind of plane"""
    y, x = np.mgrid[0:h, 0:w]
    return ((x * x // 50 + y * y // 40 + x * y // 30) % 256).astype(np.uint8)


def random_alpha(seed):
    """seeded random bytes: arbitrary residuals under every filter, so a dropped or doubled carry changes what follows it"""
    return lambda h, w: np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def planes(h, w, seed):
    """Y, U, V for the model's encoder"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = np.clip((xx * 3 + yy * 2) % 256 + rng.integers(-30, 30, (h, w)), 0, 255).astype(np.uint8)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    u = np.clip(rng.integers(60, 200, (ch, cw)), 0, 255).astype(np.uint8)
    v = np.clip(128 + (np.mgrid[0:ch, 0:cw][1] * 7) % 90 - 45, 0, 255).astype(np.uint8)
    return y, u, v


# ---- ALPH filters, forward (the decoder's inverses: csrc/fl_vp8dec_core.h) --------------------------------------------------------------

def alpha_filter(a, method):
    a = a.astype(np.int32)
    h, w = a.shape
    pred = np.zeros_like(a)
    pred[0, 1:] = a[0, :-1]                 # the first row: from the left, whatever the method
    pred[1:, 0] = a[:-1, 0]                 # the first column: from above
    if method == 1:
        pred[1:, 1:] = a[1:, :-1]
    elif method == 2:
        pred[1:, 1:] = a[:-1, 1:]
    elif method == 3:
        pred[1:, 1:] = np.clip(a[1:, :-1] + a[:-1, 1:] - a[:-1, :-1], 0, 255)
    return ((a - pred) & 255).astype(np.uint8) if method else a.astype(np.uint8)


def splice_alpha(data, a, method):
    """the raw ALPH chunk of a model file replaced by the plane filtered with `method`"""
    at = data.index(b"ALPH")
    assert int.from_bytes(data[at + 4:at + 8], "little") == 1 + a.size
    return data[:at + 8] + bytes([method << 2]) + alpha_filter(a, method).tobytes() + data[at + 9 + a.size:]


def extended(data, orientation=None):
    """a simple-format file in the extended container, with an EXIF chunk behind the picture"""
    assert data[12:16] == b"VP8 "
    frame = data[12:]
    w = int.from_bytes(data[26:28], "little") & 0x3fff
    h = int.from_bytes(data[28:30], "little") & 0x3fff

    def chunk(tag, payload):
        return tag + len(payload).to_bytes(4, "little") + bytes(payload) + (b"\0" if len(payload) & 1 else b"")
    flags = 0x08 if orientation else 0
    body = b"WEBP" + chunk(b"VP8X", flags.to_bytes(4, "little") + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")) + frame
    if orientation:
        body += chunk(b"EXIF", vp8l_write.exif(orientation, prefix=bool(orientation & 1)))
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def refused_file(feature):
    """A 16 x 16 key frame that is a header and little more, written bit by bit with the model's boolean coder: one of the features
    the decoder refuses (csrc/fl_vp8src.h) is set, so nothing behind the header is ever read.  feature: "color_space", "clamp",
    "segment_delta", "ref_lf_delta", "mode_lf_delta"."""
    bw = vp8_model.BoolWriter()
    bw.literal(int(feature == "color_space"), 1)
    bw.literal(int(feature == "clamp"), 1)
    if feature == "segment_delta":
        for v in (1, 0, 1, 0) + (0,) * 8:     # segmentation on, no map, values sent, DELTA mode, no quantiser and no filter value
            bw.literal(v, 1)
    else:
        bw.literal(0, 1)
    bw.literal(0, 1); bw.literal(0, 6); bw.literal(0, 3)    # normal filter, level 0, sharpness 0
    if feature in ("ref_lf_delta", "mode_lf_delta"):
        bw.literal(1, 1); bw.literal(1, 1)                  # loop_filter_adj_enable, deltas sent
        for k in range(8):
            hit = k == (1 if feature == "ref_lf_delta" else 6)
            bw.literal(int(hit), 1)
            if hit:
                bw.literal(5, 6); bw.literal(1, 1)          # -5
    else:
        bw.literal(0, 1)
    bw.literal(0, 2); bw.literal(40, 7)                     # one partition, quantiser index 40
    for _ in range(6):
        bw.literal(0, 1)                                    # no quantiser deltas, refresh_entropy_probs
    for p in vp8_model.UPDATE_PROB:
        bw.put(0, p)
    bw.literal(0, 1)                                        # no skip flags
    part0 = bw.finish()
    frame = (1 << 4 | len(part0) << 5).to_bytes(3, "little") + b"\x9d\x01\x2a" + (16).to_bytes(2, "little") * 2 + part0 + b"\0\0"
    body = b"WEBPVP8 " + len(frame).to_bytes(4, "little") + frame + (b"\0" if len(frame) & 1 else b"")
    return b"RIFF" + len(body).to_bytes(4, "little") + body


REFUSED_FEATURES = {"color_space": "colour-space", "clamp": "clamping", "segment_delta": "delta mode", "ref_lf_delta": "ref_lf_delta", "mode_lf_delta": "mode_lf_delta"}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def model(name, w, h, quality, seed, alpha=None, alpha_method=0):
    """alpha: None for an opaque picture, or the plane as a function of (h, w)"""
    def make():
        y, u, v = planes(h, w, seed)
        a = alpha(h, w) if alpha else None
        data, rec, stats = vp8_model.encode(y, u, v, quality, a=a)
        if alpha_method:
            data = splice_alpha(data, a, alpha_method)
        return dict(data=data, yuv=rec, channels=4 if alpha else 3, alpha=a, stats=stats)
    MODEL[name] = make


for _w, _h in ((1, 1), (16, 16), (17, 33), (48, 32)):
    model(f"model_{_w}x{_h}", _w, _h, 75, 300 + _w)
for _h, _n in ((16, 1), (32, 2), (64, 4), (128, 8)):
    model(f"model_partitions{_n}", 16, _h, 60, 310 + _n)
for _q in (1, 30, 75, 99):
    model(f"model_quality{_q}", 32, 32, _q, 320 + _q)
model("model_alpha_raw", 33, 17, 75, 330, alpha=ramp_alpha)
for _m in (1, 2, 3):
    model(f"model_alpha_filter{_m}", 33, 17, 75, 330, alpha=ramp_alpha, alpha_method=_m)
model("model_alpha_filter3_tall", 5, 70, 75, 331, alpha=ramp_alpha, alpha_method=3)
# The seams of vp8dec_alpha_kernel's scheduling at stride 1 (csrc/fl_vp8dec.hip: 64-sample chunks of a row with a carry between them,
# rows dealt over 16 waves, the first column summed 64 rows a pass, columns dealt over 1,024 threads, gradient bands of 1,024 rows):
#   64 x 2     a row is exactly one chunk                 3 x 1030   17 passes of the column sum, columns 1,030 long, a second
#   65 x 2     one sample into the second chunk                      gradient band of 6 rows (which reads the first band's last row)
#   129 x 17   three chunks, more rows than waves         1100 x 3   18 chunks, columns beyond thread 1,023, w + 1,023 gradient steps
ALPHA_SEAM_SIZES = ((64, 2), (65, 2), (129, 17), (3, 1030), (1100, 3))
for _k, (_w, _h) in enumerate(ALPHA_SEAM_SIZES):
    for _m in (1, 2, 3):
        model(f"model_alpha_{_w}x{_h}_filter{_m}", _w, _h, 75, 340 + _k, alpha=random_alpha(350 + 4 * _k + _m), alpha_method=_m)
model("model_alpha_1100x3_filter0", 1100, 3, 75, 344, alpha=random_alpha(366))   # the copy loop, 1,024 samples a pass


def libwebp(name, picture, quality, **settings):
    LIBWEBP[name] = lambda: dict(data=vp8_dec_lib.encode(picture(), quality, **settings))


for _w, _h in ((1, 1), (16, 16), (17, 33), (48, 32), (16, 208), (336, 48), (300, 200)):
    libwebp(f"lib_{_w}x{_h}", lambda w=_w, h=_h: textured(h, w, 400 + w), 75)
libwebp("lib_560x288", lambda: bars(288, 560, 410), 60)          # more macroblocks on a diagonal (17) than waves in the workgroup
libwebp("lib_default", lambda: textured(40, 56, 420), 75)         # segmentation with a map, normal filter
libwebp("lib_quality20", lambda: textured(40, 56, 420), 20)       # level 30
libwebp("lib_quality5", lambda: textured(40, 56, 420), 5)         # a level at and above 40
libwebp("lib_quality99", lambda: textured(40, 56, 420), 99)       # small steps: large levels
libwebp("lib_simple_filter", lambda: textured(40, 56, 420), 75, filter_type=0)
libwebp("lib_sharpness5", lambda: textured(40, 56, 420), 75, filter_sharpness=5)
libwebp("lib_strength0", lambda: textured(40, 56, 420), 75, filter_strength=0)
libwebp("lib_segments1", lambda: textured(40, 56, 420), 75, segments=1)
libwebp("lib_bars", lambda: bars(80, 112, 430), 50)               # skipped macroblocks, flat and busy segments
libwebp("lib_bars_strong", lambda: bars(80, 112, 430), 30, filter_strength=100)
libwebp("lib_skips", lambda: quiet_and_noise(96, 144, 3, False), 50, method=2)          # skipped one-mode macroblocks, level 16
libwebp("lib_skips_bpred", lambda: quiet_and_noise(96, 144, 3, True), 10, method=2)     # ... and skipped B_PRED ones, level 41
libwebp("lib_alpha_raw", lambda: textured(40, 56, 440, ramp_alpha(40, 56)), 75, alpha_compression=0)
libwebp("lib_alpha_raw_filtered", lambda: textured(41, 57, 441, ramp_alpha(41, 57)), 75, alpha_compression=0, alpha_filtering=2)
libwebp("lib_alpha_compressed", lambda: textured(40, 56, 440, ramp_alpha(40, 56)), 75)   # a compressed (VP8L-coded) ALPH

libwebp("lib_alpha_compressed_filtered", lambda: textured(41, 57, 441, ramp_alpha(41, 57)), 75, alpha_filtering=2, alpha_quality=60)


def libwebp_alpha(name, w, h, method, candidates):
    """A VP8L-coded ALPH plane (read at stride 4: the green bytes) under filter `method`.  libwebp picks the filter itself, so the case
    is the first of `candidates` -- (plane, alpha_filtering, alpha_quality) -- whose ALPH header says compression 1 and `method`; with
    none, building the case fails, and so does every test that asks for it."""
    def make():
        seen = []
        for plane, filtering, quality in candidates:
            data = vp8_dec_lib.encode(textured(h, w, 6, plane(h, w)), 75, alpha_filtering=filtering, alpha_quality=quality)
            head = data[data.index(b"ALPH") + 8]
            if (head & 3, head >> 2 & 3) == (1, method):
                return dict(data=data)
            seen.append((head & 3, head >> 2 & 3))
        raise AssertionError(f"{name}: no candidate gave a compressed ALPH plane under filter {method}; (compression, filter) were {seen}")
    LIBWEBP[name] = make


# 200 x 70: four chunks a row and more rows than waves, under every method; 70 x 1030: the second gradient band; 1100 x 3: 18 chunks and
# columns beyond thread 1,023
libwebp_alpha("lib_alpha_200x70_filter0", 200, 70, 0, ((slope_alpha, 1, 100), (ramp_alpha, 0, 100), (bowl_alpha, 0, 100)))
libwebp_alpha("lib_alpha_200x70_filter1", 200, 70, 1, ((slope_alpha, 2, 60), (ramp_alpha, 1, 100), (slope_alpha, 2, 30)))
libwebp_alpha("lib_alpha_200x70_filter2", 200, 70, 2, ((slope_alpha, 2, 100), (ramp_alpha, 2, 100), (ramp(11, 1), 2, 100)))
libwebp_alpha("lib_alpha_200x70_filter3", 200, 70, 3, ((bowl_alpha, 2, 100), (ramp_alpha, 2, 30), (ramp(7, 1), 2, 60)))
libwebp_alpha("lib_alpha_70x1030_filter3", 70, 1030, 3, ((slope_alpha, 2, 60), (slope_alpha, 2, 30), (ramp(5, 1), 2, 60)))
libwebp_alpha("lib_alpha_1100x3_filter1", 1100, 3, 1, ((slope_alpha, 2, 100), (slope_alpha, 2, 60), (bowl_alpha, 2, 100)))
libwebp_alpha("lib_alpha_1100x3_filter2", 1100, 3, 2, ((ramp_alpha, 2, 100), (ramp(7, 2), 2, 100), (ramp(11, 1), 2, 100)))

# Rounds of the macroblock schedule: 16 macroblocks of a diagonal a round in vp8dec_recon_kernel, 32 in vp8dec_filter_kernel.  65 x 33
# macroblocks: the fullest diagonals hold 33 (a second filter round with one slot active, a third reconstruction round with one wave);
# 65 x 32: 32, whole rounds only.  B_PRED and one-mode macroblocks alternate, so every round takes the sixteen sub-steps with waves
# of both kinds in it
libwebp("lib_rounds_1040x528", lambda: quilt(528, 1040, 450), 60)
libwebp("lib_rounds_simple_1040x528", lambda: quilt(528, 1040, 450), 60, filter_type=0)
libwebp("lib_rounds_1040x512", lambda: quilt(512, 1040, 451), 60)
# the cases above that exist for the device's scheduling alone: to the host half they are more of what the others hold
SCHEDULING = sorted(n for n in list(MODEL) + list(LIBWEBP) if re.search(r"_(alpha|rounds\w*)_\d+x\d+", n))

REFUSED = ()
NAMES = sorted(MODEL) + sorted(LIBWEBP)


@functools.lru_cache(maxsize=None)
def get(name):
    if name in MODEL:
        c = MODEL[name]()
        c["pixels"] = vp8_dec_lib.decode_pixels(c["data"], c["channels"]) if have_libwebp() else None
        return c
    c = LIBWEBP[name]()
    c["channels"] = 4 if b"ALPH" in c["data"][:64] else 3
    c["yuv"] = vp8_dec_lib.decode_yuv(c["data"])
    c["pixels"] = vp8_dec_lib.decode_pixels(c["data"], c["channels"])
    return c


def names(libwebp_too=True):
    """the cases that can be built (libwebp_too: with libwebp loaded), the refused ones left out"""
    return [n for n in NAMES if n not in REFUSED and (n in MODEL or libwebp_too)]
