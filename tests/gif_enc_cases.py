"""Source files for the tests of the GIF encoder (csrc/fl_gif.hip), written from construction with tests/gif_write.py: every case is a
small animation and a request; what the encoder sees is the request applied to the composited canvases (tests/gif_model.py).  The
request "webp=true" is the identity for GIF frames (not as_is, no dimensions, Nearest, no front end), so for those cases the
canvases ARE the encoder's input and the properties below (pixel counts against the segment length S, colour counts, which closing
codes are widened, data lengths on a sub-block boundary) are properties of the case.  Where a case needed a search, it was done with
the model (tests/gif_enc_model.py) and the found size / seed is written here; tests/test_gif_encode_host.py checks the property.
Canvases stay at or below 128 x 64 = 8,192 pixels (S + 1 = 3 x 683 and 2 S + 1 = 17 x 241 have no other shape)."""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import gif_cases as gc
import gif_enc_model as em
import gif_model as gm
import gif_write as gw
from gif_write import Frame

S = em.SEG
IDENTITY = "webp=true"


@dataclass
class EncCase:
    width: int
    height: int
    frames: List[Frame]
    global_table: Optional[np.ndarray]
    query: str = IDENTITY
    fallback: bool = False        # a frame above 256 colours: the pixels come back


def distinct(rng, n):
    """n different colours"""
    v = rng.choice(1 << 24, n, replace=False)
    return np.stack([v >> 16, v >> 8 & 255, v & 255], 1).astype(np.uint8)


def pow2(n):
    return max(2, 1 << (n - 1).bit_length())


def all_of(rng, h, w, n):
    """indices 0 .. n - 1, every one used (n <= h * w)"""
    a = np.concatenate([np.arange(n), rng.integers(0, n, h * w - n)]).astype(np.uint8)
    rng.shuffle(a)
    return a.reshape(h, w)


BUILDERS = {}


def case(name):
    def reg(fn):
        BUILDERS[name] = fn
        return fn
    return reg


# ---- pixel counts around the segment length ---------------------------------------------------------------------------------------
for _name, (_w, _h) in {"pixels_1": (1, 1), "pixels_S_minus_1": (89, 23), "pixels_S": (64, 32), "pixels_S_plus_1": (683, 3), "pixels_2S_plus_1": (241, 17)}.items():
    def _build(rng, w=_w, h=_h):
        n = min(64, w * h)
        return EncCase(w, h, [Frame(0, 0, gc.noise(rng, h, w, n)), Frame(0, 0, gc.blotches(rng, h, w, n), disposal=1)], distinct(rng, pow2(n)))
    BUILDERS[_name] = _build

# ---- colour counts: every table size, both sides of every size's edge, and the two that fall back ---------------------------------
for _n in (1, 2, 3, 4, 5, 16, 17, 128, 129, 255, 256):
    def _build(rng, n=_n):
        return EncCase(32, 16, [Frame(0, 0, all_of(rng, 16, 32, n))], distinct(rng, pow2(n)))
    BUILDERS["colours_%d" % _n] = _build

for _n in (257, 300):
    def _build(rng, n=_n):
        cols = distinct(rng, 512)
        extra = n - 256
        patch = np.arange(extra, dtype=np.uint8).reshape(1, extra)
        return EncCase(64, 16, [Frame(0, 0, all_of(rng, 16, 64, 256), disposal=1),
                                Frame(0, 0, patch, table=cols[256:256 + pow2(extra)])], cols[:256], fallback=True)
    BUILDERS["colours_%d" % _n] = _build


@case("fallback_in_the_middle")
def _(rng):
    # 256, 257 and 4 colours: one frame of three is beyond the exact palette
    cols = distinct(rng, 512)
    return EncCase(32, 16, [Frame(0, 0, all_of(rng, 16, 32, 256), disposal=1),
                            Frame(3, 2, np.zeros((1, 1), np.uint8), table=cols[256:258], disposal=1),
                            Frame(0, 0, all_of(rng, 16, 32, 4), table=cols[300:304])], cols[:256], fallback=True)


# ---- what the LZW stage can go wrong at -------------------------------------------------------------------------------------------
@case("noise_256_colours_three_segments")
def _(rng):
    # nearly every pair is new: the code width climbs 9 -> 12 inside every full segment
    return EncCase(128, 40, [Frame(0, 0, all_of(rng, 40, 128, 256))], distinct(rng, 256))


@case("constant_frame")
def _(rng):
    # the longest matches: match k is k indices long
    return EncCase(128, 64, [Frame(0, 0, np.zeros((64, 128), np.uint8))], distinct(rng, 2))


@case("noise_4_colours_code_size_2")
def _(rng):
    return EncCase(100, 50, [Frame(0, 0, all_of(rng, 50, 100, 4))], distinct(rng, 4))


# closing codes: found with the model (see the module's docstring); "wide" = the decoder's table reaches a power of two behind the
# segment's last data code, so the closing code is one bit wider than it
@case("end_code_wide")
def _(rng):
    # three different indices at code size 2: codes 0, 1, 2, the decoder's next entry is 8 = 1 << 3
    return EncCase(3, 1, [Frame(0, 0, np.array([[0, 1, 2]], np.uint8))], distinct(rng, 4))


@case("end_code_plain")
def _(rng):
    return EncCase(2, 1, [Frame(0, 0, np.array([[0, 1]], np.uint8))], distinct(rng, 4))


def clear_code_frame(noisy):
    """S + 64 indices, so the first segment closes with a clear code: `noisy` of 16-colour noise, then one colour (few codes more)"""
    a = np.zeros(33 * 64, np.uint8)
    a[:noisy] = np.random.default_rng(7).integers(0, 16, noisy, dtype=np.uint8)
    return a.reshape(33, 64)


CLEAR_WIDE = 682      # noisy indices with which the first segment's closing clear code is widened
CLEAR_PLAIN = 600     # ... and is not


@case("clear_code_wide")
def _(rng):
    return EncCase(64, 33, [Frame(0, 0, clear_code_frame(CLEAR_WIDE))], distinct(rng, 16))


@case("clear_code_plain")
def _(rng):
    return EncCase(64, 33, [Frame(0, 0, clear_code_frame(CLEAR_PLAIN))], distinct(rng, 16))


# data lengths on a sub-block boundary: noise of DATA_255[name] = (width, seed, colours) gives exactly 255 k / 255 k + 1 data bytes
DATA_255 = {"data_255": (804, 0, 4), "data_256": (365, 2, 16), "data_510": (774, 2, 16), "data_511": (775, 2, 16)}


def data_frame(width, seed, colours):
    a = np.random.default_rng(seed).integers(0, colours, (1, width), dtype=np.uint8)
    a[0, :colours] = np.arange(colours)       # every colour is there
    return a


for _name in DATA_255:
    def _build(rng, name=_name):
        width, seed, colours = DATA_255[name]
        return EncCase(width, 1, [Frame(0, 0, data_frame(width, seed, colours))], distinct(rng, colours))
    BUILDERS[_name] = _build


# ---- transparency, channel counts, tables, many frames --------------------------------------------------------------------------------
def _partial(query):
    def build(rng):
        # the first frame leaves a border of the canvas untouched (alpha 0), the second is transparent in places
        g = distinct(rng, 8)
        return EncCase(40, 24, [Frame(3, 2, gc.noise(rng, 19, 33, 8), disposal=1),
                                Frame(0, 0, gc.noise(rng, 12, 20, 8), transparent=3, disposal=2),
                                Frame(10, 5, gc.blotches(rng, 10, 16, 8), transparent=0)], g, query)
    return build


BUILDERS["transparent_partial_first_frame"] = _partial(IDENTITY)
BUILDERS["transparent_inverse"] = _partial("inverse=true")
BUILDERS["transparent_grayscale"] = _partial("grayscale=true")          # LumaA8: two channels


@case("opaque_grayscale_two_channels")
def _(rng):
    return EncCase(37, 21, [Frame(0, 0, gc.noise(rng, 21, 37, 32)), Frame(5, 5, gc.noise(rng, 9, 11, 32))], distinct(rng, 32), "grayscale=true")


@case("tables_of_different_sizes")
def _(rng):
    return EncCase(32, 16, [Frame(0, 0, all_of(rng, 16, 32, n), table=distinct(rng, pow2(n)), disposal=1) for n in (2, 100, 5, 256, 17)], None)


@case("frames_70")
def _(rng):
    g = distinct(rng, 16)
    return EncCase(20, 20, [Frame(0, 0, gc.noise(rng, 20, 20, 16), disposal=1)] +
                   [Frame(int(rng.integers(0, 10)), int(rng.integers(0, 10)), gc.blotches(rng, 10, 10, 16), disposal=1) for _ in range(69)], g)


# ---- requests that change the frames: a frame, grayscale, inverse and a fill colour, one each ------------------------------------------
def _request(query):
    def build(rng):
        g = distinct(rng, 16)
        return EncCase(30, 20, [Frame(0, 0, gc.noise(rng, 20, 30, 16), disposal=1), Frame(4, 4, gc.blotches(rng, 12, 20, 16), transparent=2, disposal=1),
                                Frame(0, 0, gc.blotches(rng, 20, 30, 16))], g, query)
    return build


BUILDERS["request_letterbox"] = _request("w=64&h=20")
BUILDERS["request_grayscale"] = _request("w=40&h=30&grayscale=true")
BUILDERS["request_inverse"] = _request("w=33&h=21&inverse=true")
BUILDERS["request_fill_colour"] = _request("w=50&h=50&rgb=12,200,7")

CASES = list(BUILDERS)
_CACHE = {}


def get(name):
    """(file bytes, the composited canvases (F, h, w, 4), the case)"""
    if name not in _CACHE:
        c = BUILDERS[name](gc.rng_of("enc_" + name))
        data = gw.write_gif(c.width, c.height, c.frames, c.global_table, head=gw.application_ext(0))
        _CACHE[name] = (data, gm.from_frames(c.width, c.height, c.frames, c.global_table), c)
    return _CACHE[name]


def model_input(name):
    """The frames the encoder sees, where the host can say so without a device: the canvases for the identity request; None for the requests that
    change the frames."""
    data, canvases, c = get(name)
    if c.query == IDENTITY:
        return canvases
    return None
