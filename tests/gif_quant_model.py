"""The colour quantiser of csrc/fl_gifquant.hip (FLGPU_ENCODE_GIF_QUANTIZE) restated in numpy / Python, on top of tests/gif_enc_model.py:
a frame of at most 256 colours keeps the exact palette and its bytes; a frame above that gets a local table of at most 256 entries by
the rule below and is then coded, packed and framed as every other frame.  Integers only; nothing depends on an order of arrival, so
the device's bytes are pinned to this model's.  The rule is this project's own (a variance-ordered median cut over a histogram whose
precision follows the frame); nothing of NeuQuant is restated or claimed.

  1. alpha != 0 is opaque.  Any alpha-0 pixel reserves ONE entry, behind the opaque ones: K = 255, else K = 256.
  2. s = the least of 0, 1, 2, 3 at which the opaque pixels have at most 4,096 distinct (r >> s, g >> s, b >> s); 3 if none has.
  3. one cell per distinct reduced colour: n, the sums of the exact samples, representative c = (sum + n // 2) // n per channel.
  4. boxes of cells: N = sum n, per axis S = sum n c, Q = sum n c c, V = N Q - S S.  The box's axis has the greatest V (r before g
     before b), its priority is V // N, its cut t = S // N on that axis; splittable iff V > 0.  While boxes < K: the splittable
     box of greatest priority (lowest number on ties) hands its cells with c[axis] > t to box number `boxes`.
  5. entry of a box = (exact sums + N // 2) // N; entries ascending by (r, g, b, box number); the transparent entry (0, 0, 0) behind.
  6. an opaque pixel takes the entry of least squared distance to its exact samples, the lowest index on ties.
A frame above 2 ** 22 pixels is not quantised (the 64-bit products are sized for that): the file falls back as without the bit."""
import struct

import numpy as np

import gif_enc_model as em

MAX_PIXELS = 1 << 22      # csrc/fl_gif_quant_core.h kGifQuantMaxPixels
MAX_CELLS = 4096          # ... kGifQuantHashCells
_QUANTIZED = {}           # the tests ask for the same frames again and again


def rgb_of(frame):
    """(h, w, 2 | 4) uint8 -> ((h * w, 3) int64 samples, (h * w) bool opaque); LumaA8 as l, l, l"""
    px = frame.reshape(-1, frame.shape[-1]).astype(np.int64)
    if frame.shape[-1] == 2:
        return np.stack([px[:, 0]] * 3, 1), px[:, 1] != 0
    return px[:, :3], px[:, 3] != 0


def precision_of(rgb):
    """step 2, and the cell number of every sample at that precision"""
    for s in (0, 1, 2, 3):
        red = rgb >> s
        cell = red[:, 0] << 16 | red[:, 1] << 8 | red[:, 2]
        if s == 3 or len(np.unique(cell)) <= MAX_CELLS:
            return s, cell


def box_stats(n, c, members):
    """N, S[3], Q[3] of a box in Python integers (the device's 64 bits hold them up to MAX_PIXELS)"""
    nn, cc = n[members], c[members]
    return int(nn.sum()), [int((nn * cc[:, a]).sum()) for a in range(3)], [int((nn * cc[:, a] * cc[:, a]).sum()) for a in range(3)]


def box_choice(N, S, Q):
    """(V, axis, priority, cut): the axis of greatest V, r before g before b"""
    V = [N * Q[a] - S[a] * S[a] for a in range(3)]
    axis = max(range(3), key=lambda a: (V[a], -a))
    assert V[axis] < 1 << 64
    return V[axis], axis, V[axis] // N, S[axis] // N


def median_cut(n, sums, K, trace=None):
    """steps 3 - 5 on the cells: the box number of every cell and the boxes' entries (boxes, 3), in box order"""
    c = (sums + (n // 2)[:, None]) // n[:, None]
    box = np.zeros(len(n), np.int64)
    boxes = 1 if len(n) else 0
    choice = {0: box_choice(*box_stats(n, c, box == 0))} if boxes else {}
    while boxes < K:
        open_ = [(-choice[b][2], b) for b in range(boxes) if choice[b][0] > 0]
        if not open_:
            break
        b = min(open_)[1]
        V, axis, priority, cut = choice[b]
        up = (box == b) & (c[:, axis] > cut)
        if trace is not None:
            trace.append(dict(box=b, axis=axis, priority=priority, cut=cut, V=V, low=int(((box == b) & ~up).sum()), high=int(up.sum())))
        box[up] = boxes
        choice[b] = box_choice(*box_stats(n, c, box == b))
        choice[boxes] = box_choice(*box_stats(n, c, box == boxes))
        boxes += 1
    entries = np.zeros((boxes, 3), np.int64)
    for b in range(boxes):
        N = int(n[box == b].sum())
        entries[b] = (sums[box == b].sum(0) + N // 2) // N
    return box, entries


def quantize(frame, trace=None):
    """A frame above 256 colours -> dict(table (entries, 3) uint8 in file order, indices (h * w) uint8, transparent index or None,
    s, cells, boxes, K)"""
    memo = (frame.shape, np.ascontiguousarray(frame).tobytes())
    if trace is None and memo in _QUANTIZED:
        return _QUANTIZED[memo]
    rgb, opaque = rgb_of(frame)
    assert len(rgb) <= MAX_PIXELS
    clear = bool((~opaque).any())
    K = 255 if clear else 256
    orgb = rgb[opaque]
    s, cell = precision_of(orgb) if len(orgb) else (0, np.zeros(0, np.int64))
    ids, inverse = np.unique(cell, return_inverse=True)
    n = np.bincount(inverse, minlength=len(ids)).astype(np.int64)
    sums = np.stack([np.bincount(inverse, orgb[:, a], minlength=len(ids)) for a in range(3)], 1).astype(np.int64) if len(ids) else np.zeros((0, 3), np.int64)
    box, entries = median_cut(n, sums, K, trace)
    boxes = len(entries)
    order = sorted(range(boxes), key=lambda b: (tuple(entries[b]), b))
    table = entries[order].reshape(-1, 3)
    idx = np.full(len(rgb), boxes, np.int64)                 # the transparent entry sits behind the opaque ones
    if boxes:
        # (chunks: 16,384 pixels x 256 entries of int64 at a time)
        near = np.empty(len(orgb), np.int64)
        for at in range(0, len(orgb), 16384):
            d = ((orgb[at:at + 16384, None, :] - table[None, :, :]) ** 2).sum(-1)
            near[at:at + 16384] = d.argmin(1)                 # the first of equal minima: the lowest index
        idx[opaque] = near
    if clear:
        table = np.concatenate([table, np.zeros((1, 3), np.int64)])
    _QUANTIZED[memo] = dict(table=table.astype(np.uint8), indices=idx.astype(np.uint8), transparent=boxes if clear else None, s=s, cells=len(ids), boxes=boxes, K=K)
    return _QUANTIZED[memo]


def marked(frame):
    return em.colours_of(frame) > 256


def palette_of(frame):
    """tests/gif_enc_model.py::palette_of with the quantiser behind it: (padded table, table bits, indices, transparent index or None)"""
    p = em.palette_of(frame)
    if p is not None:
        return p
    q = quantize(frame)
    bits = max(1, int(len(q["table"]) - 1).bit_length())
    table = np.zeros((1 << bits, 3), np.uint8)
    table[:len(q["table"])] = q["table"]
    return table, bits, q["indices"], q["transparent"]


def encode_frame(frame, seg=em.SEG):
    table, bits, idx, transparent = palette_of(frame)
    h, w = frame.shape[:2]
    mcs = max(2, bits)
    out = b"\x21\xf9\x04" + struct.pack("<BHB", 0x04 | (transparent is not None), 0, transparent or 0) + b"\x00"
    out += b"\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0x80 | (bits - 1)) + table.tobytes() + bytes([mcs])
    return out + em.sub_blocks(em.frame_data(idx, mcs, seg))


def encode_file(frames, seg=em.SEG):
    """frames: (F, h, w, c) or a list of (h, w, c) -> the file; None where the limit sends the file back as pixels"""
    h, w = frames[0].shape[:2]
    if h * w > MAX_PIXELS and any(marked(np.ascontiguousarray(f)) for f in frames):
        return None
    out = bytearray(em.FILE_HEAD % struct.pack("<HH", w, h))
    for f in frames:
        out += encode_frame(np.ascontiguousarray(f), seg)
    return bytes(out + b"\x3b")


def to_rgba(frame):
    """what a decoder of the model's file shows for one frame alone: the table's colour, (0, 0, 0, 0) at the transparent index"""
    table, bits, idx, transparent = palette_of(frame)
    rgba = np.concatenate([table, np.full((len(table), 1), 255, np.uint8)], 1)
    if transparent is not None:
        rgba[transparent] = 0
    return rgba[idx].reshape(frame.shape[0], frame.shape[1], 4)


def squared_error(frame, rgba):
    """mean squared error over r, g, b of the opaque pixels"""
    rgb, opaque = rgb_of(frame)
    got = rgba.reshape(-1, rgba.shape[-1])[:, :3].astype(np.int64)
    return float(((rgb[opaque] - got[opaque]) ** 2).mean()) if opaque.any() else 0.0
