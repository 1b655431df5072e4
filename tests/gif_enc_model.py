"""The GIF encoder of csrc/fl_gif.hip restated in numpy / Python: the palette rule of gif 0.13.1's Frame::from_rgba_speed below 257
colours, and the exact file the device writes -- the same segment length, closing-code rule, framing and worst case.  Greedy longest
match is deterministic whatever the dictionary's hash, so the device's bytes are pinned to this model's."""
import struct

import numpy as np

SEG = 2048          # csrc/fl_gif.h kGifSegIndices (tests/test_gif_encode_host.py holds the two together)
FILE_HEAD = b"GIF89a%s\x70\x00\x00" + b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"


def max_frame_bytes(pixels, seg=SEG):
    """control extension 8 + descriptor 10 + table 768 + code size 1 + the data at its worst (a clear code, one code per index,
    every segment's closing code, all at 12 bits) in sub-blocks of 255 + the terminator"""
    d = (12 * (pixels + 1 + (pixels + seg - 1) // seg) + 7) // 8
    return 8 + 10 + 768 + 1 + d + (d + 254) // 255 + 1


def max_file_bytes(frames, pixels, channels, seg=SEG):
    return 64 + frames * max(pixels * channels, max_frame_bytes(pixels, seg))


def keys_of(frame):
    """(h, w, 2 | 4) uint8 -> (h * w) uint32: r, g, b, a big-endian, alpha != 0 as 255 (LumaA8 as l, l, l, a)"""
    px = frame.reshape(-1, frame.shape[-1]).astype(np.uint32)
    if frame.shape[-1] == 2:
        r = g = b = px[:, 0]
        a = px[:, 1]
    else:
        r, g, b, a = px[:, 0], px[:, 1], px[:, 2], px[:, 3]
    return r << 24 | g << 16 | b << 8 | np.where(a != 0, 255, 0).astype(np.uint32)


def colours_of(frame):
    return len(np.unique(keys_of(frame)))


def palette_of(frame):
    """None above 256 colours; else (table (size, 3) uint8 padded with zeros, table bits, indices, transparent index or None)"""
    keys = keys_of(frame)
    pal, idx = np.unique(keys, return_inverse=True)        # ascending dwords = ascending (r, g, b, a) tuples
    if len(pal) > 256:
        return None
    bits = max(1, int(len(pal) - 1).bit_length())
    table = np.zeros((1 << bits, 3), np.uint8)
    table[:len(pal), 0], table[:len(pal), 1], table[:len(pal), 2] = pal >> 24, pal >> 16 & 255, pal >> 8 & 255
    clear = np.flatnonzero(keys & 255 == 0)
    transparent = int(idx.reshape(-1)[clear[-1]]) if len(clear) else None   # the LAST pixel with alpha 0
    return table, bits, idx.reshape(-1).astype(np.uint8), transparent


def lzw_segment(indices, mcs, leading_clear, last):
    """One segment from an empty table: [(code, width)], and whether the closing code was written wider than the last data code.
    The table cannot fill (SEG <= 3838), so the width only ever grows."""
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    codes, table, nxt, width = [], {}, clear + 2, mcs + 1
    if leading_clear:
        codes.append((clear, width))
    cur = int(indices[0])
    for k in indices[1:]:
        k = int(k)
        hit = table.get((cur, k))
        if hit is not None:
            cur = hit
            continue
        codes.append((cur, width))
        table[(cur, k)] = nxt
        nxt += 1
        if nxt - 1 == 1 << width and width < 12:
            width += 1
        cur = k
    codes.append((cur, width))
    # the decoder adds one more entry behind the last data code; the closing code's width follows that (with a code size of at
    # least 2 this is tests/gif_write.py::lzw_greedy's rule: a segment of one code cannot sit on a width boundary)
    bumped = nxt == 1 << width and width < 12
    if bumped:
        width += 1
    codes.append((eoi if last else clear, width))
    assert nxt <= 4096
    return codes, bumped


def frame_segments(indices, mcs, seg=SEG):
    n = (len(indices) + seg - 1) // seg
    return [lzw_segment(indices[s * seg:(s + 1) * seg], mcs, s == 0, s == n - 1) for s in range(n)]


def pack(codes):
    acc = n = 0
    out = bytearray()
    for c, w in codes:
        acc |= c << n
        n += w
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8
    if n:
        out.append(acc & 255)
    return bytes(out)


def sub_blocks(data):
    out = bytearray()
    for i in range(0, len(data), 255):
        out.append(min(255, len(data) - i))
        out += data[i:i + 255]
    out.append(0)
    return bytes(out)


def frame_data(indices, mcs, seg=SEG):
    """the frame's LZW bytes in front of the sub-block framing"""
    return pack([cw for codes, _ in frame_segments(indices, mcs, seg) for cw in codes])


def encode_frame(frame, seg=SEG):
    p = palette_of(frame)
    if p is None:
        return None
    table, bits, idx, transparent = p
    h, w = frame.shape[:2]
    mcs = max(2, bits)
    out = b"\x21\xf9\x04" + struct.pack("<BHB", 0x04 | (transparent is not None), 0, transparent or 0) + b"\x00"
    out += b"\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0x80 | (bits - 1)) + table.tobytes() + bytes([mcs])
    return out + sub_blocks(frame_data(idx, mcs, seg))


def encode_file(frames, seg=SEG):
    """frames: (F, h, w, c) or a list of (h, w, c), c = 2 | 4 -> the file, or None if a frame has more than 256 colours"""
    h, w = frames[0].shape[:2]
    out = bytearray(FILE_HEAD % struct.pack("<HH", w, h))
    for f in frames:
        body = encode_frame(np.ascontiguousarray(f), seg)
        if body is None:
            return None
        out += body
    return bytes(out + b"\x3b")


def to_rgba(frame):
    """what a decoder of the model's file shows for one frame alone: the palette's colour, (0, 0, 0, 0) at the transparent index"""
    table, bits, idx, transparent = palette_of(frame)
    rgba = np.concatenate([table, np.full((len(table), 1), 255, np.uint8)], 1)
    if transparent is not None:
        rgba[transparent] = 0
    return rgba[idx].reshape(frame.shape[0], frame.shape[1], 4)
