"""The shared case list of the GIF decode front end's tests: every file is written by tests/gif_write.py from a frame list, and
what it must decode to is tests/gif_model.py applied to that same list.  get(name) -> (file bytes, expected frames (F, H, W, 4),
Case)."""
import struct
import zlib
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

import gif_model as gm
import gif_write as gw
from gif_write import Frame


@dataclass
class Case:
    width: int
    height: int
    frames: List[Frame]
    global_table: Optional[np.ndarray] = None
    kw: dict = field(default_factory=dict)

    @property
    def pillow_comparable(self):
        """Pillow's compositing coincides with the model's where the file names no disposal to the background or to the previous
        canvas (in a graphic control extension that a later one overrides either) and the first frame covers the canvas"""
        f0 = self.frames[0]
        named = [f.disposal for f in self.frames] + [f.gce_first[0] for f in self.frames if f.gce_first is not None]
        return all(d in (0, 1) for d in named) and (f0.x, f0.y) == (0, 0) and f0.size == (self.width, self.height)


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def table(rng, n):
    return rng.integers(0, 256, (n, 3), dtype=np.uint8)


def noise(rng, h, w, n):
    return rng.integers(0, n, (h, w), dtype=np.uint8)


def blotches(rng, h, w, n):
    """runs and repeats, so that the greedy encoder builds long strings"""
    a = rng.integers(0, n, ((h + 3) // 4, (w + 3) // 4), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(a, np.ones((4, 4), np.uint8))[:h, :w])


BUILDERS = {}


def case(name):
    def reg(fn):
        BUILDERS[name] = fn
        return fn
    return reg


def _add(name, fn):
    BUILDERS[name] = fn


# ---- canvases: widths that are no multiple of the pixels a thread owns, more than one workgroup, and the 16-byte path -----------
CANVASES = [(1, 1), (5, 3), (13, 9), (67, 5), (301, 7), (16, 5), (300, 8)]


def _canvas(w, h):
    def build(rng):
        g = table(rng, 64)
        frames = [Frame(0, 0, noise(rng, h, w, 64), disposal=1)]
        rw, rh = max(1, w // 2), max(1, h // 2)
        x, y = min(1, w - rw), min(1, h - rh)
        frames.append(Frame(x, y, noise(rng, rh, rw, 64), disposal=0, transparent=5))
        frames.append(Frame(w - rw, h - rh, noise(rng, rh, rw, 16), table=table(rng, 16), interlace=True, transparent=3))
        return Case(w, h, frames, g)
    return build


for _w, _h in CANVASES:
    _add(f"canvas_{_w}x{_h}", _canvas(_w, _h))


# ---- frame rectangles on a 13 x 9 canvas: (x, y, w, h) ---------------------------------------------------------------------------
RECTS = {"1x1": (6, 4, 1, 1), "odd": (3, 1, 7, 5), "left": (0, 2, 4, 5), "top": (3, 0, 5, 3), "right": (9, 1, 4, 5), "bottom": (2, 6, 6, 3),
         "corner": (12, 8, 1, 1), "cover": (0, 0, 13, 9)}


def _rect(r):
    def build(rng):
        x, y, w, h = r
        g = table(rng, 32)
        return Case(13, 9, [Frame(x, y, noise(rng, h, w, 32), disposal=1, transparent=0),
                            Frame(5, 3, noise(rng, 4, 5, 32), disposal=2),
                            Frame(x, y, noise(rng, h, w, 32), transparent=7)], g)
    return build


for _n, _r in RECTS.items():
    _add(f"rect_{_n}", _rect(_r))


# ---- disposal: every method alone (3 on the first frame included), every pair, mixes over five frames ----------------------------
def _disposal(methods):
    def build(rng):
        g = table(rng, 16)
        spots = [(2, 1, 8, 6), (0, 0, 13, 9), (5, 3, 7, 5), (1, 4, 6, 4), (6, 0, 7, 7)]
        frames = []
        for k, d in enumerate(methods):
            x, y, w, h = spots[(k + len(methods)) % 5]
            frames.append(Frame(x, y, noise(rng, h, w, 16), disposal=d, transparent=(k * 3) % 16 if k % 2 else None))
        return Case(13, 9, frames, g)
    return build


for _d in range(4):
    _add(f"disposal_single_{_d}", _disposal([_d]))
for _a in range(4):
    for _b in range(4):
        _add(f"disposal_pair_{_a}{_b}", _disposal([_a, _b]))
for _m in ([1, 2, 3, 0, 1], [3, 3, 2, 2, 1], [2, 1, 3, 2, 0], [0, 4, 5, 6, 7], [3, 2, 3, 2, 3]):
    _add("disposal_five_" + "".join(map(str, _m)), _disposal(_m))


@case("disposal_2_then_transparent")
def _(rng):
    g = table(rng, 8)
    return Case(13, 9, [Frame(0, 0, noise(rng, 9, 13, 8), disposal=1),
                        Frame(2, 2, noise(rng, 5, 8, 8), disposal=2),
                        Frame(1, 1, noise(rng, 7, 10, 4), transparent=1),
                        Frame(0, 0, np.full((9, 13), 2, np.uint8), transparent=2)], g)


# ---- interlace: every pass count ---------------------------------------------------------------------------------------------------
def _interlace(h):
    def build(rng):
        g = table(rng, 128)
        frames = [Frame(0, 0, noise(rng, h, 7, 128), interlace=True)]
        if h > 2:
            frames.append(Frame(2, 1, noise(rng, h - 1, 4, 128), interlace=True, transparent=9))
        return Case(7, h, frames, g)
    return build


for _h in list(range(1, 10)) + [17]:
    _add(f"interlace_h{_h}", _interlace(_h))


# ---- colour tables -----------------------------------------------------------------------------------------------------------------
@case("tables_local_every_frame")
def _(rng):
    return Case(13, 9, [Frame(k, k, noise(rng, 5, 7, n), table=table(rng, n), disposal=1) for k, n in enumerate((4, 256, 2, 32, 8))], None)


@case("tables_two_colours")
def _(rng):
    return Case(9, 6, [Frame(0, 0, noise(rng, 6, 9, 2)), Frame(3, 2, noise(rng, 3, 4, 2), transparent=1, table=table(rng, 2))], table(rng, 2))


@case("tables_transparent_index_moves")
def _(rng):
    g = table(rng, 8)
    return Case(10, 10, [Frame(0, 0, noise(rng, 10, 10, 8))] + [Frame(k, k, noise(rng, 6, 6, 8), transparent=k) for k in range(1, 5)], g)


@case("tables_local_overrides_global")
def _(rng):
    return Case(8, 8, [Frame(0, 0, noise(rng, 8, 8, 4)), Frame(0, 0, noise(rng, 8, 8, 4), table=table(rng, 4)), Frame(1, 1, noise(rng, 5, 5, 4))], table(rng, 4))


@case("tables_transparent_beyond_table")
def _(rng):
    # the transparent index names no entry of the table: no pixel may use it, and none does
    return Case(6, 4, [Frame(0, 0, noise(rng, 4, 6, 4), transparent=200)], table(rng, 4))


def _sizes(n):
    def build(rng):
        return Case(11, 7, [Frame(0, 0, noise(rng, 7, 11, n))], table(rng, n))
    return build


for _n in (2, 4, 8, 16, 32, 64, 128, 256):
    _add(f"tables_size_{_n}", _sizes(_n))


# ---- LZW ---------------------------------------------------------------------------------------------------------------------------
def _mcs(mcs, encoder):
    def build(rng):
        n = min(1 << mcs, 256)
        return Case(19, 11, [Frame(0, 0, blotches(rng, 11, 19, n), mcs=mcs, encoder=encoder)], table(rng, n))
    return build


for _m in range(2, 9):
    for _e in ("greedy", "plain"):
        _add(f"lzw_mcs{_m}_{_e}", _mcs(_m, _e))


@case("lzw_mcs_wider_than_table")
def _(rng):
    return Case(9, 9, [Frame(0, 0, noise(rng, 9, 9, 4), mcs=6)], table(rng, 4))


@case("lzw_fills_table_immediate_clear")
def _(rng):
    return Case(120, 100, [Frame(0, 0, noise(rng, 100, 120, 256))], table(rng, 256))


@case("lzw_deferred_clear_never")
def _(rng):
    return Case(120, 100, [Frame(0, 0, noise(rng, 100, 120, 256), deferred=10 ** 9)], table(rng, 256))


@case("lzw_deferred_clear_after_50")
def _(rng):
    return Case(120, 100, [Frame(0, 0, noise(rng, 100, 120, 200), deferred=50)], table(rng, 256))


@case("lzw_fills_table_mcs2")
def _(rng):
    return Case(150, 120, [Frame(0, 0, noise(rng, 120, 150, 4), deferred=300)], table(rng, 4))


@case("lzw_kwkwk_runs")
def _(rng):
    idx = np.zeros((40, 40), np.uint8)
    idx[20:] = 3
    return Case(40, 40, [Frame(0, 0, idx), Frame(0, 0, np.ascontiguousarray(idx.T), disposal=1)], table(rng, 4))


@case("lzw_no_leading_clear")
def _(rng):
    return Case(17, 9, [Frame(0, 0, blotches(rng, 9, 17, 16), leading_clear=False), Frame(1, 1, noise(rng, 5, 5, 16), leading_clear=False, encoder="plain")], table(rng, 16))


@case("lzw_no_end_code")
def _(rng):
    return Case(17, 9, [Frame(0, 0, blotches(rng, 9, 17, 16), end_code=False), Frame(1, 1, noise(rng, 5, 5, 16), end_code=False, encoder="plain")], table(rng, 16))


@case("lzw_data_beyond_frame")
def _(rng):
    return Case(17, 9, [Frame(0, 0, blotches(rng, 9, 17, 16), extra=40), Frame(1, 1, noise(rng, 5, 5, 16), extra=7, encoder="plain")], table(rng, 16))


@case("lzw_small_sub_blocks")
def _(rng):
    return Case(31, 17, [Frame(0, 0, noise(rng, 17, 31, 64), block=7), Frame(0, 0, noise(rng, 17, 31, 64), block=1)], table(rng, 64))


# ---- container ---------------------------------------------------------------------------------------------------------------------
@case("container_gif87a")
def _(rng):
    return Case(9, 5, [Frame(0, 0, noise(rng, 5, 9, 8), gce=False)], table(rng, 8), dict(version=b"GIF87a"))


@case("container_extensions_everywhere")
def _(rng):
    ext = gw.comment_ext() + gw.application_ext(3) + gw.plain_text_ext()
    return Case(9, 5, [Frame(0, 0, noise(rng, 5, 9, 8), before=gw.comment_ext(b"x" * 300)),
                       Frame(2, 1, noise(rng, 3, 5, 8), disposal=1, transparent=2, before=gw.plain_text_ext())], table(rng, 8),
                dict(head=ext, tail=gw.comment_ext(b"the end") + b"\x21\x77" + gw.sub_blocks(b"an extension nobody knows")))


@case("container_last_gce_wins")
def _(rng):
    return Case(9, 5, [Frame(0, 0, noise(rng, 5, 9, 8)),
                       Frame(1, 1, noise(rng, 3, 5, 8), disposal=0, transparent=4, gce_first=(2, 1), gce=True),
                       Frame(0, 0, noise(rng, 2, 2, 8))], table(rng, 8))


@case("container_gce_applies_to_one_frame")
def _(rng):
    return Case(9, 5, [Frame(0, 0, noise(rng, 5, 9, 8), disposal=2, transparent=1), Frame(1, 1, noise(rng, 3, 5, 8), gce=False),
                       Frame(0, 0, noise(rng, 5, 9, 8), gce=False)], table(rng, 8))


@case("container_bytes_behind_trailer")
def _(rng):
    return Case(4, 4, [Frame(0, 0, noise(rng, 4, 4, 4))], table(rng, 4), dict(behind=b"\x00\x21 anything at all"))


# ---- random four-frame files Pillow can be held against -------------------------------------------------------------------------
def _random4(k):
    def build(rng):
        w, h = int(rng.integers(5, 41)), int(rng.integers(5, 41))
        n = int(rng.choice([4, 16, 64, 256]))
        frames = [Frame(0, 0, blotches(rng, h, w, n), disposal=int(rng.integers(0, 2)), transparent=(int(rng.integers(0, n)) if k % 2 else None))]
        for _ in range(3):
            fw, fh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            x, y = int(rng.integers(0, w - fw + 1)), int(rng.integers(0, h - fh + 1))
            local = table(rng, n) if rng.integers(0, 3) == 0 else None
            frames.append(Frame(x, y, blotches(rng, fh, fw, n), disposal=int(rng.integers(0, 2)), table=local, interlace=bool(rng.integers(0, 2)),
                                transparent=(int(rng.integers(0, n)) if k % 2 else None)))
        return Case(w, h, frames, table(rng, n))
    return build


for _k in range(12):
    _add(f"random4_{_k:02d}", _random4(_k))


CASES = sorted(BUILDERS)
_CACHE = {}


def get(name):
    if name not in _CACHE:
        c = BUILDERS[name](rng_of(name))
        kw = dict(c.kw)
        behind = kw.pop("behind", b"")
        data = gw.write_gif(c.width, c.height, c.frames, c.global_table, **kw) + behind
        want = gm.from_frames(c.width, c.height, c.frames, c.global_table)
        want.setflags(write=False)
        _CACHE[name] = (data, want, c)
    return _CACHE[name]


def expected_info(c: Case):
    """what flgpu_gif_info_of must say about a case's file"""
    mcs = []
    for f in c.frames:
        n = len(f.table) if f.table is not None else len(c.global_table)
        mcs.append(f.mcs if f.mcs is not None else max(2, (n - 1).bit_length()))
    mask = 0
    for f in c.frames:
        mask |= 1 << f.disposal
    return dict(width=c.width, height=c.height, frames=len(c.frames), has_global_table=int(c.global_table is not None),
                interlaced_frames=sum(f.interlace for f in c.frames), transparent_frames=sum(f.transparent is not None for f in c.frames),
                disposal_mask=mask, max_code_size=max(mcs), decoded_bytes=len(c.frames) * c.width * c.height * 4, supported=1)


# ---- files that must be refused: damaged (FLGPU_ERR_PARSE) and not vouched for (FLGPU_ERR_UNSUPPORTED) ---------------------------

def small_file(rng=None, **kw):
    rng = rng or rng_of("small")
    g = table(rng, 4)
    return gw.write_gif(6, 5, [Frame(1, 1, noise(rng, 3, 4, 4), disposal=1, transparent=2), Frame(0, 0, noise(rng, 5, 6, 4))], g, **kw)


def lzw_frame(raw, mcs=2, w=3, h=2):
    return gw.write_gif(4, 4, [Frame(0, 0, np.zeros((h, w), np.uint8), raw_lzw=raw, mcs=mcs)], table(rng_of("lzw"), 4))


def parse_cases():
    good = small_file()
    cases = {"bad_signature_version": b"GIF88a" + good[6:], "bad_signature_magic": b"GIX89a" + good[6:], "empty": b"", "signature_only": good[:6]}
    # truncated anywhere in front of the trailer: inside the screen descriptor, the global table, the extension, the image
    # descriptor, the data sub-blocks, and with only the trailer missing
    for at in (10, 13, 20, 26, 30, 38, 41, 44, len(good) - 3, len(good) - 2, len(good) - 1):
        cases[f"truncated_at_{at}"] = good[:at]
    cases["truncated_but_trailer_byte_inside_a_sub_block"] = good[:43] + b"\x3b"
    cases["zero_canvas_width"] = good[:6] + struct.pack("<HH", 0, 5) + good[10:]
    cases["zero_canvas_height"] = good[:6] + struct.pack("<HH", 6, 0) + good[10:]
    # clear (4), then code 7 where the next free entry is 6; and code 6 = the next free entry with no code in front of it
    cases["lzw_code_beyond_next_free"] = lzw_frame(gw.pack_codes([(4, 3), (1, 3), (7, 3), (5, 3)]))
    cases["lzw_next_free_first_after_clear"] = lzw_frame(gw.pack_codes([(4, 3), (6, 3), (5, 3)]))
    cases["lzw_next_free_without_clear"] = lzw_frame(gw.pack_codes([(6, 3), (5, 3)]))
    cases["lzw_fewer_indices_end_code"] = lzw_frame(gw.lzw_greedy([0, 1, 2, 3, 0], 2))
    cases["lzw_fewer_indices_no_end_code"] = lzw_frame(gw.lzw_plain([0, 1, 2, 3, 0], 2, end_code=False))
    cases["lzw_no_data_at_all"] = lzw_frame(b"")
    cases["no_colour_table_at_all"] = gw.write_gif(4, 4, [Frame(0, 0, np.zeros((4, 4), np.uint8), mcs=2)], None)
    cases["unknown_block_introducer"] = good[:-1] + b"\x55\x00\x3b"
    cases["unknown_block_introducer_first"] = good[:25] + b"\x00" + good[25:]
    return cases


def unsupported_cases():
    rng = rng_of("unsupported")
    g = table(rng, 4)
    px = noise(rng, 3, 4, 4)
    one = Frame(0, 0, np.zeros((1, 1), np.uint8), encoder="plain")
    cases = {
        "no_frames": gw.write_gif(6, 5, [], g),
        "no_frames_but_extensions": gw.write_gif(6, 5, [], g, head=gw.comment_ext() + gw.gce_block(1, None)),
        "frame_zero_width": gw.write_gif(6, 5, [Frame(1, 1, px, w=0)], g),
        "frame_zero_height": gw.write_gif(6, 5, [Frame(1, 1, px, h=0)], g),
        "frame_beyond_right_edge": gw.write_gif(6, 5, [Frame(3, 1, px)], g),
        "frame_beyond_bottom_edge": gw.write_gif(6, 5, [Frame(1, 3, px)], g),
        "second_frame_outside": gw.write_gif(6, 5, [Frame(0, 0, px), Frame(65535, 65535, px)], g),
        "index_at_table_size": gw.write_gif(6, 5, [Frame(0, 0, np.array([[0, 1, 2, 3]], np.uint8), table=table(rng, 2), mcs=2)], g),
        "index_beyond_global_table": gw.write_gif(6, 5, [Frame(0, 0, np.array([[0, 9, 2, 3]], np.uint8), mcs=4)], g),
        "frames_4097": gw.write_gif(2, 2, [one] * 4097, g),
        "decoded_above_512_mib": gw.write_gif(65535, 2049, [one], g),
        "decoded_above_512_mib_by_frames": gw.write_gif(4096, 4096, [one] * 9, g),
    }
    for m in (0, 1, 9, 12, 255):
        cases[f"min_code_size_{m}"] = gw.write_gif(6, 5, [Frame(1, 1, px, mcs_byte=m)], g)
    return cases
