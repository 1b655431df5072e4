"""Inputs for the tests of the GIF quantiser (csrc/fl_gifquant.hip, FLGPU_ENCODE_GIF_QUANTIZE).

CASES are source files written from construction with tests/gif_write.py, as tests/gif_enc_cases.py does.  One frame of a GIF has at
most 256 colours, so a canvas above that is LAYERED: frame k paints the pixels of the k-th group of 255 colours from a local table
and leaves the others transparent, disposal 1 keeps what lies below; the last canvas shows the whole picture and the ones before it
are frames of the animation too (each with fewer colours and a transparent rest, so most cases also carry K = 255 frames).  With the
identity request the composited canvases ARE the encoder's input.  One case gets its frames from the request instead (a grayscale
conversion to LumaA8); its regime is asserted on the device's own pixels.

FRAMES are plain frame arrays for the host tests (model, host twin): every identity case's canvases, the shapes no GIF source can
produce through the identity request (alpha-0 pixels of differing r, g, b, LumaA8), and 128 x 128 noise of 16,384 colours, which
as a file would take 65 layers."""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import gif_cases as gc
import gif_enc_cases as ec
import gif_model as gm
import gif_write as gw
from gif_write import Frame

IDENTITY = ec.IDENTITY


@dataclass
class QCase:
    width: int
    height: int
    frames: List[Frame]
    global_table: Optional[np.ndarray]
    query: str = IDENTITY


def layered(rgb, opaque=None):
    """the frames that leave `rgb` (h, w, 3) on the canvas where `opaque` (h, w), nothing elsewhere"""
    h, w = rgb.shape[:2]
    opaque = np.ones((h, w), bool) if opaque is None else opaque
    packed = rgb[..., 0].astype(np.int64) << 16 | rgb[..., 1].astype(np.int64) << 8 | rgb[..., 2]
    colours = np.unique(packed[opaque])
    frames = []
    for at in range(0, len(colours), 255):
        group = colours[at:at + 255]
        table = np.zeros((256, 3), np.uint8)
        table[:len(group)] = np.stack([group >> 16, group >> 8 & 255, group & 255], 1)
        idx = np.full((h, w), 255, np.uint8)
        mine = opaque & np.isin(packed, group)
        idx[mine] = np.searchsorted(group, packed[mine])
        frames.append(Frame(0, 0, idx, table=table, transparent=255, disposal=1))
    return QCase(w, h, frames, None)


def spread(rng, h, w, colours):
    """(h, w, 3): every one of `colours` (n, 3) at least once (n <= h * w), the rest drawn from them"""
    pick = np.concatenate([np.arange(len(colours)), rng.integers(0, len(colours), h * w - len(colours))])
    rng.shuffle(pick)
    return colours[pick].reshape(h, w, 3)


def bit_reverse(x):
    return int("{:08b}".format(x)[::-1], 2)


BUILDERS = {}


def case(name):
    def reg(fn):
        BUILDERS[name] = fn
        return fn
    return reg


# ---- colour counts and regimes --------------------------------------------------------------------------------------------------------
for _n in (257, 272):
    def _build(rng, n=_n):
        return layered(spread(rng, 16, 17, ec.distinct(rng, n)))
    BUILDERS["colours_%d" % _n] = _build

@case("fallback_in_the_middle")
def _(rng):
    return ec.get("fallback_in_the_middle")[2]                                  # that very file: 256, 257 and 4 colours, only the middle frame is quantised


def _grid(n):
    """n colours of (r, g, b) with r, g < 64 and b < 2: at s = 1 at most 32 x 32 cells"""
    v = np.arange(n)
    return np.stack([v >> 7, v >> 1 & 63, v & 1], 1).astype(np.uint8)


for _n in (4096, 4097):
    def _build(rng, n=_n):
        return layered(spread(rng, 65, 64, _grid(n)))                           # the s = 0 / 1 edge
    BUILDERS["colours_%d" % _n] = _build


@case("dark_s1")
def _(rng):
    return layered(rng.integers(0, 24, (80, 80, 3)).astype(np.uint8))           # 12 ^ 3 cells at s = 1, more than 4,096 colours


@case("dark_s2")
def _(rng):
    return layered(rng.integers(0, 48, (80, 80, 3)).astype(np.uint8))           # 12 ^ 3 cells at s = 2, more than 4,096 at s = 1


@case("noise_128_s3")
def _(rng):
    # 128 x 128 noise over 5,000 colours, every one in a 5 : 5 : 5 cell of its own: more than 4,096 cells at s = 3 (20 layers; all
    # 16,384 colours of plain noise would take 65)
    cell = rng.choice(1 << 15, 5000, replace=False)
    cols = np.stack([cell >> 10, cell >> 5 & 31, cell & 31], 1) << 3 | rng.integers(0, 8, (5000, 3))
    return layered(spread(rng, 128, 128, cols.astype(np.uint8)))


# ---- transparency and channels --------------------------------------------------------------------------------------------------------
@case("one_clear_pixel")
def _(rng):
    opaque = np.ones((16, 17), bool)
    opaque[7, 5] = False
    return layered(spread(rng, 16, 17, ec.distinct(rng, 271)), opaque)          # K = 255 on the last canvas


@case("grayscale_256_and_clear")
def _(rng):
    grey = np.arange(256, dtype=np.uint8)
    idx = np.concatenate([np.arange(256), rng.integers(0, 256, 5)]).astype(np.uint8).reshape(9, 29)
    return QCase(30, 10, [Frame(1, 1, idx)], np.stack([grey] * 3, 1), "grayscale=true")   # LumaA8: 256 greys and the border's alpha 0


# ---- ties and geometry ----------------------------------------------------------------------------------------------------------------
def _ramp(colour_of):
    def build(rng):
        # 256 colours once each and a clear rest: K = 255, so exactly one box keeps two colours -- which one is the tie rules' doing
        table = np.array([colour_of(x) for x in range(256)], np.uint8)
        idx = np.arange(256, dtype=np.uint8)
        rng.shuffle(idx)
        return QCase(17, 16, [Frame(0, 0, idx.reshape(16, 16))], table)
    return build


BUILDERS["ties_between_boxes"] = _ramp(lambda x: (x, 0, 0))                      # mirror halves: equal priorities at every level
BUILDERS["ties_between_axes"] = _ramp(lambda x: (x, bit_reverse(x), 7))          # the same V on r and g, another split on each


@case("pixels_285")
def _(rng):
    return layered(spread(rng, 15, 19, ec.distinct(rng, 280)))                  # no multiple of four pixels


@case("eight_frames_all_marked")
def _(rng):
    cols = ec.distinct(rng, 256 + 7 * 8)
    frames = [Frame(1, 1, ec.all_of(rng, 18, 18, 256), disposal=1)]              # 256 colours and the untouched border: 257 keys
    for k in range(7):
        frames.append(Frame(2 + 2 * k, 3, np.arange(8, dtype=np.uint8).reshape(2, 4), table=cols[256 + 8 * k:264 + 8 * k], disposal=1))
    return QCase(20, 20, frames, cols[:256])


CASES = list(BUILDERS)
_CACHE = {}


def get(name):
    """(file bytes, the composited canvases (F, h, w, 4), the case)"""
    if name not in _CACHE:
        c = BUILDERS[name](gc.rng_of("quant_" + name))
        data = gw.write_gif(c.width, c.height, c.frames, c.global_table, head=gw.application_ext(0))
        _CACHE[name] = (data, gm.from_frames(c.width, c.height, c.frames, c.global_table), c)
    return _CACHE[name]


# ---- plain frames for the host tests --------------------------------------------------------------------------------------------------
def _exact_with_clear_colours(rng):
    # 200 opaque colours; 72 alpha-0 pixels of differing r, g, b: 272 keys, an exact palette of 201 entries
    cols = ec.distinct(rng, 272)
    flat = np.concatenate([np.concatenate([cols[:72], spread(rng, 4, 67, cols[72:]).reshape(-1, 3)]), np.full((340, 1), 255, np.uint8)], -1)
    flat[:72, 3] = 0
    return flat.reshape(1, 17, 20, 4)


def _no_opaque_pixel(rng):
    f = np.concatenate([spread(rng, 16, 17, ec.distinct(rng, 260)), np.zeros((16, 17, 1), np.uint8)], -1)
    return f[None]


def _noise_128(rng):
    return np.concatenate([rng.integers(0, 256, (1, 128, 128, 3)), np.full((1, 128, 128, 1), 255)], -1).astype(np.uint8)


def _luma_alpha(rng):
    l = np.concatenate([np.arange(256), rng.integers(0, 256, 24), np.full(5, 7)]).astype(np.uint8)
    a = np.concatenate([np.full(280, 200), np.zeros(5)]).astype(np.uint8)      # alpha 200 counts as 255
    return np.stack([l, a], -1).reshape(1, 15, 19, 2)


EXTRA = {"exact_with_clear_colours": _exact_with_clear_colours, "no_opaque_pixel": _no_opaque_pixel, "noise_128": _noise_128,
         "luma_alpha_257": _luma_alpha}
IDENTITY_CASES = [n for n in CASES if n != "grayscale_256_and_clear"]
FRAMES = IDENTITY_CASES + list(EXTRA)
_FRAMES = {}


def frames_of(name):
    if name not in _FRAMES:
        _FRAMES[name] = EXTRA[name](gc.rng_of("quant_" + name)) if name in EXTRA else get(name)[1]
    return _FRAMES[name]
