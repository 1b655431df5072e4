"""The GIF compositing rules in numpy, for the tests of the GIF decode front end: palette lookup with the transparent index,
de-interlacing, and the disposal chain, as include/fanlin_gpu.h and DESIGN.md state them.  Works from the writer's own frame list
(tests/gif_write.py) and from the blob the host half leaves (flgpu_debug_gif_blob)."""
import struct

import numpy as np

import gif_write as gw

MAGIC = 0x31464947


def compose(width, height, frames):
    """frames: [(x, y, rgba (h, w, 4) with alpha 0 where transparent, disposal)] -> (F, height, width, 4): what every frame shows.
    A pixel of alpha 0 leaves the canvas as it is; disposal 0, 1, 4..7 keep the composited canvas for the next frame, 2 clears
    the frame's rectangle to 0, 0, 0, 0, 3 goes back to the canvas from before the frame."""
    prev = np.zeros((height, width, 4), np.uint8)
    out = np.zeros((len(frames), height, width, 4), np.uint8)
    for f, (x, y, rgba, disposal) in enumerate(frames):
        h, w = rgba.shape[:2]
        cur = prev.copy()
        region = cur[y:y + h, x:x + w]
        opaque = rgba[..., 3] != 0
        region[opaque] = rgba[opaque]
        out[f] = cur
        if disposal == 2:
            prev = cur.copy()
            prev[y:y + h, x:x + w] = 0
        elif disposal != 3:
            prev = cur
    return out


def palette_of(table, transparent):
    pal = np.zeros((256, 4), np.uint8)
    pal[:len(table), :3] = table
    pal[:len(table), 3] = 255
    if transparent is not None:
        pal[transparent] = 0
    return pal


def from_frames(width, height, frames, global_table):
    """the model applied to the writer's frame list"""
    rgba = []
    for f in frames:
        table = f.table if f.table is not None else global_table
        rgba.append((f.x, f.y, palette_of(table, f.transparent)[f.indices], f.disposal))
    return compose(width, height, rgba)


def blob_header(blob):
    magic, width, height, frames, palettes, pal_off, idx_off, total = struct.unpack_from("<8I", blob, 0)
    return dict(magic=magic, width=width, height=height, frames=frames, palettes=palettes, pal_off=pal_off, idx_off=idx_off, total_bytes=total)


def blob_records(blob):
    H = blob_header(blob)
    names = ("x", "y", "w", "h", "disposal", "interlaced", "pal_off", "idx_off")
    return [dict(zip(names, struct.unpack_from("<8I", blob, 32 + 32 * f))) for f in range(H["frames"])]


def from_blob(blob):
    """the model applied to the blob: its inverse"""
    H = blob_header(blob)
    assert H["magic"] == MAGIC and H["total_bytes"] == len(blob)
    buf = np.frombuffer(blob, np.uint8)
    frames = []
    for r in blob_records(blob):
        assert r["pal_off"] % 16 == 0 and H["pal_off"] <= r["pal_off"] <= len(blob) - 1024
        assert H["idx_off"] <= r["idx_off"] and r["idx_off"] + r["w"] * r["h"] <= H["pal_off"]
        pal = buf[r["pal_off"]:r["pal_off"] + 1024].reshape(256, 4)
        stored = buf[r["idx_off"]:r["idx_off"] + r["w"] * r["h"]].reshape(r["h"], r["w"])
        idx = stored
        if r["interlaced"]:
            idx = np.empty_like(stored)
            idx[gw.interlace_order(r["h"])] = stored
        frames.append((r["x"], r["y"], pal[idx], r["disposal"]))
    return compose(H["width"], H["height"], frames)
