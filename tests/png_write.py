"""Writes PNG files from chosen samples, so that the expected pixels of a decode test come from construction and not from a
decoder: a chosen filter type per row (a numpy forward filter), a chosen zlib level / strategy, a chosen IDAT split, PLTE and
tRNS as given.  `expand` says what Transformations::EXPAND makes of the same samples (the picture the image crate sees)."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(kind: bytes, data: bytes = b"", crc=None) -> bytes:
    c = zlib.crc32(kind + data) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", c)


def pack_rows(samples: np.ndarray, depth: int) -> np.ndarray:
    """samples (h, w, n) with values < 2**depth -> (h, row_bytes) uint8, leftmost sample in the high bits."""
    s = np.asarray(samples)
    h, w, n = s.shape
    if depth == 8:
        return s.astype(np.uint8).reshape(h, w * n)
    assert n == 1 and depth in (1, 2, 4)
    per = 8 // depth
    padded = np.zeros((h, (w + per - 1) // per * per), np.uint16)
    padded[:, :w] = s[:, :, 0]
    out = np.zeros((h, padded.shape[1] // per), np.uint16)
    for k in range(per):
        out |= padded[:, k::per] << (8 - depth * (k + 1))
    return out.astype(np.uint8)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def forward_filter(rows: np.ndarray, bpp: int, filters) -> bytes:
    """rows (h, row_bytes) -> the scanlines, a filter byte in front of each row (PNG 9.2)."""
    h, rb = rows.shape
    if np.isscalar(filters):
        filters = [int(filters)] * h
    r = rows.astype(np.int32)
    left = np.zeros_like(r)
    left[:, bpp:] = r[:, :-bpp] if rb > bpp else 0
    up = np.zeros_like(r)
    up[1:] = r[:-1]
    corner = np.zeros_like(r)
    corner[1:, bpp:] = r[:-1, :-bpp] if rb > bpp else 0
    pred = {0: np.zeros_like(r), 1: left, 2: up, 3: (left + up) >> 1, 4: paeth(left, up, corner)}
    out = bytearray()
    for y in range(h):
        f = int(filters[y])
        out.append(f)
        out += ((r[y] - pred[f][y]) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return co.compress(data) + co.flush()


def split_idat(stream: bytes, split=None) -> bytes:
    """split: None = one chunk; an int n = chunks of n bytes; "empty" = chunks of 1000 bytes with empty ones between."""
    if split is None:
        return chunk(b"IDAT", stream)
    if split == "empty":
        parts = [stream[i:i + 1000] for i in range(0, len(stream), 1000)]
        return chunk(b"IDAT") + b"".join(chunk(b"IDAT", p) + chunk(b"IDAT") for p in parts)
    return b"".join(chunk(b"IDAT", stream[i:i + split]) for i in range(0, len(stream), split))


def ihdr(w, h, depth, color_type, interlace=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace))


def assemble(w, h, depth, color_type, stream: bytes, split=None, plte=None, trns=None, extra=(), interlace=0) -> bytes:
    out = SIGNATURE + ihdr(w, h, depth, color_type, interlace)
    for kind, data in extra:
        out += chunk(kind, data)
    if plte is not None:
        out += chunk(b"PLTE", np.asarray(plte, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", trns_bytes(color_type, trns))
    return out + split_idat(stream, split) + chunk(b"IEND")


def trns_bytes(color_type, trns) -> bytes:
    if color_type == 3:
        return bytes(trns)
    return b"".join(struct.pack(">H", int(v)) for v in np.atleast_1d(trns))


def scanlines(samples, color_type, depth=8, filters=0) -> bytes:
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[:, :, None]
    assert s.shape[2] == SAMPLES[color_type]
    bpp = max(1, SAMPLES[color_type] * depth // 8)
    return forward_filter(pack_rows(s, depth), bpp, filters)


def write_png(samples, color_type, depth=8, filters=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, split=None, plte=None, trns=None,
              extra=(), interlace=0) -> bytes:
    """samples: (h, w) or (h, w, n) raw sample values (palette indices for colour type 3)."""
    s = np.asarray(samples)
    h, w = s.shape[:2]
    stream = deflate(scanlines(s, color_type, depth, filters), level, strategy)
    return assemble(w, h, depth, color_type, stream, split, plte, trns, extra, interlace)


def expand(samples, color_type, depth=8, plte=None, trns=None) -> np.ndarray:
    """What the image crate's PNG decoder (Transformations::EXPAND) hands on: (h, w, channels) uint8."""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[:, :, None]
    h, w = s.shape[:2]
    if color_type == 0:
        grey = (s[:, :, 0].astype(np.uint32) * (255 // ((1 << depth) - 1))).astype(np.uint8)
        if trns is None:
            return grey[:, :, None]
        alpha = np.where(s[:, :, 0] == int(np.atleast_1d(trns)[0]), 0, 255).astype(np.uint8)
        return np.dstack([grey, alpha])
    if color_type == 2:
        rgb = s.astype(np.uint8)
        if trns is None:
            return rgb
        alpha = np.where((s == np.asarray(trns).reshape(1, 1, 3)).all(axis=2), 0, 255).astype(np.uint8)
        return np.dstack([rgb, alpha])
    if color_type == 3:
        table = np.zeros((256, 4), np.uint8)
        table[:, 3] = 255                                   # beyond PLTE: opaque black
        p = np.asarray(plte, np.uint8).reshape(-1, 3)
        table[:len(p), :3] = p
        if trns is not None:
            table[:len(trns), 3] = np.frombuffer(bytes(trns), np.uint8)
        out = table[s[:, :, 0]]
        return out if trns is not None else out[:, :, :3].copy()
    return s.astype(np.uint8)                               # 4, 6


def chunks_of(data: bytes):
    """[(offset, kind, payload)] of a PNG file."""
    out, pos = [], 8
    while pos + 12 <= len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        out.append((pos, data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def idat_payload(data: bytes) -> bytes:
    return b"".join(p for _, k, p in chunks_of(data) if k == b"IDAT")
