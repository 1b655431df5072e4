"""A GIF writer from construction, for the tests of the GIF decode front end: any frame rectangles, disposal methods, transparent
indices, local and global colour tables of 2..256 entries, interlace, LZW minimum code sizes 2..8, two LZW encoders (a greedy one
that grows to 12 bits and fills the table, with an immediate or a deferred clear, and a "plain" one that pads with clear codes so
that no string is ever used), comment / application / plain-text extensions and data beyond the frame.  It validates nothing: the
error cases are written with it too."""
import struct
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


class BitWriter:
    """LSB-first codes of varying width"""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc |= code << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def pack_codes(codes):
    """[(code, width), ...] as a bit stream: for streams no encoder would write"""
    bw = BitWriter()
    for c, w in codes:
        bw.put(c, w)
    return bw.done()


def lzw_greedy(indices, mcs, deferred=None, leading_clear=True, end_code=True):
    """The usual encoder: longest match, one new entry per code, the width grows as the decoder's will.  deferred = None: a clear
    code as soon as the table is full; deferred = k: k more codes at 12 bits with the full table first (a large k: never)."""
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    bw = BitWriter()
    table, nxt, width = {}, clear + 2, mcs + 1
    full_for = 0
    if leading_clear:
        bw.put(clear, width)
    it = iter(int(v) for v in indices)
    cur = next(it, None)
    if cur is not None:
        for k in it:
            key = (cur, k)
            if key in table:
                cur = table[key]
                continue
            bw.put(cur, width)
            if nxt < 4096:
                table[key] = nxt
                nxt += 1
                if nxt - 1 == (1 << width) and width < 12:
                    width += 1
            else:
                full_for += 1
                if deferred is None or full_for > deferred:
                    bw.put(clear, width)
                    table, nxt, width, full_for = {}, clear + 2, mcs + 1, 0
            cur = k
        bw.put(cur, width)
    if end_code:
        # (the decoder adds one more entry behind the last code, if that was not the first after a clear; the end code's width follows that)
        if table and nxt < 4096 and nxt == (1 << width) and width < 12:
            width += 1
        bw.put(eoi, width)
    return bw.done()


def lzw_plain(indices, mcs, leading_clear=True, end_code=True):
    """Literals only, a clear code often enough that the width never leaves mcs + 1"""
    clear, eoi, width = 1 << mcs, (1 << mcs) + 1, mcs + 1
    run = max(clear - 2, 1)
    bw = BitWriter()
    for i, v in enumerate(int(v) for v in indices):
        if i % run == 0 and (i or leading_clear):
            bw.put(clear, width)
        bw.put(v, width)
    if end_code:
        bw.put(eoi, width)
    return bw.done()


def sub_blocks(data, size=255):
    out = bytearray()
    for i in range(0, len(data), size):
        part = data[i:i + size]
        out.append(len(part))
        out += part
    out.append(0)
    return bytes(out)


def interlace_order(h):
    return list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))


def table_bits(n):
    """the 3-bit size field of a colour table of n = 2, 4, .. 256 entries"""
    return {2: 0, 4: 1, 8: 2, 16: 3, 32: 4, 64: 5, 128: 6, 256: 7}[n]


@dataclass
class Frame:
    x: int
    y: int
    indices: np.ndarray                    # (h, w) uint8, rows in display order
    disposal: int = 0
    transparent: Optional[int] = None
    table: Optional[np.ndarray] = None     # local colour table (n, 3) uint8, n a power of two; None = the global one
    interlace: bool = False
    mcs: Optional[int] = None              # LZW minimum code size; None = what the table needs, at least 2
    encoder: str = "greedy"                # "greedy" | "plain"
    deferred: Optional[int] = None
    leading_clear: bool = True
    end_code: bool = True
    extra: int = 0                         # indices written beyond w x h
    block: int = 255                       # data sub-block size
    gce: Optional[bool] = None             # None = write a graphic control extension when it says something
    gce_first: Optional[tuple] = None      # (disposal, transparent) of an extra graphic control extension in FRONT of the real one
    delay: int = 0
    before: bytes = b""                    # raw blocks (extensions) in front of the image descriptor
    raw_lzw: Optional[bytes] = None        # the LZW bytes, instead of an encoder's
    mcs_byte: Optional[int] = None         # the code size byte as written, whatever was encoded
    w: Optional[int] = None                # the descriptor's size, if not the array's
    h: Optional[int] = None

    @property
    def size(self):
        return (self.indices.shape[1] if self.w is None else self.w, self.indices.shape[0] if self.h is None else self.h)


def gce_block(disposal, transparent, delay=0):
    packed = (disposal & 7) << 2 | (1 if transparent is not None else 0)
    return b"\x21\xf9\x04" + struct.pack("<BHB", packed, delay, transparent or 0) + b"\x00"


def comment_ext(text=b"written from construction"):
    return b"\x21\xfe" + sub_blocks(text, 100)


def application_ext(loops=0):
    return b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loops) + b"\x00"


def plain_text_ext(text=b"hello"):
    return b"\x21\x01\x0c" + struct.pack("<HHHHBBBB", 0, 0, 8, 8, 8, 8, 1, 0) + sub_blocks(text, 3)


def frame_bytes(f: Frame, global_size):
    out = bytearray(f.before)
    if f.gce_first is not None:
        out += gce_block(f.gce_first[0], f.gce_first[1])
    want_gce = f.gce if f.gce is not None else (f.disposal != 0 or f.transparent is not None or f.delay != 0)
    if want_gce:
        out += gce_block(f.disposal, f.transparent, f.delay)
    w, h = f.size
    packed = (0x40 if f.interlace else 0)
    if f.table is not None:
        packed |= 0x80 | table_bits(len(f.table))
    out += b"\x2c" + struct.pack("<HHHHB", f.x, f.y, w, h, packed)
    if f.table is not None:
        out += np.ascontiguousarray(f.table, np.uint8).tobytes()
    n = len(f.table) if f.table is not None else (global_size or 256)
    mcs = f.mcs if f.mcs is not None else max(2, (n - 1).bit_length())
    rows = f.indices[interlace_order(f.indices.shape[0])] if f.interlace else f.indices
    flat = rows.reshape(-1)
    if f.extra:
        flat = np.concatenate([flat, np.resize(flat, f.extra)])
    if f.raw_lzw is not None:
        data = f.raw_lzw
    elif f.encoder == "plain":
        data = lzw_plain(flat, mcs, f.leading_clear, f.end_code)
    else:
        data = lzw_greedy(flat, mcs, f.deferred, f.leading_clear, f.end_code)
    out.append(mcs if f.mcs_byte is None else f.mcs_byte)
    out += sub_blocks(data, f.block)
    return bytes(out)


def write_gif(width, height, frames: List[Frame], global_table=None, version=b"GIF89a", head=b"", tail=b"", trailer=True, background=0):
    """head: raw blocks between the global table and the first frame; tail: raw blocks in front of the trailer"""
    out = bytearray(version)
    packed = 0x70 | ((0x80 | table_bits(len(global_table))) if global_table is not None else 0)
    out += struct.pack("<HHBBB", width, height, packed, background, 0)
    if global_table is not None:
        out += np.ascontiguousarray(global_table, np.uint8).tobytes()
    out += head
    for f in frames:
        out += frame_bytes(f, len(global_table) if global_table is not None else 0)
    out += tail
    if trailer:
        out += b"\x3b"
    return bytes(out)
