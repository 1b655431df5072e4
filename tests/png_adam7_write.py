"""Writes Adam7-interlaced PNG files from chosen samples, on top of tests/png_write.py: every non-empty pass is the reduced
picture samples[y0::dy, x0::dx], filtered and packed as a picture of its own (png_write.scanlines), the passes concatenated, one
zlib stream around them, IHDR's interlace byte 1.  The expected pixels are png_write.expand of the same samples: they come from
construction, not from a decoder.  tests/test_png_adam7_host.py pins the files against Pillow's reader."""
import zlib

import numpy as np

import png_write as pw

# PNG specification 8.2: x origin, y origin, x step, y step of passes 1..7
PASSES = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]


def pass_shapes(w, h):
    """[(pass width, pass height)] of the seven passes; a pass with a zero side is absent from the stream."""
    return [(len(range(x0, w, dx)), len(range(y0, h, dy))) for x0, y0, dx, dy in PASSES]


def pass_row_bytes(w, h, color_type, depth):
    return [(pw_ * pw.SAMPLES[color_type] * depth + 7) // 8 for pw_, _ in pass_shapes(w, h)]


def scan_bytes(w, h, color_type, depth):
    """Bytes of the inflated stream: the sum over the non-empty passes of pass height x (1 + pass row bytes)."""
    return sum(ph * (1 + rb) for (pw_, ph), rb in zip(pass_shapes(w, h), pass_row_bytes(w, h, color_type, depth)) if pw_ and ph)


def pass_filters(filters, k, ph):
    """The filter types of pass k's rows.  filters: an int (every row of every pass); a list of seven entries, one per pass, each an int
    or a list per pass row; a callable (pass index, pass height) -> int or list."""
    if callable(filters):
        return filters(k, ph)
    if np.isscalar(filters):
        return int(filters)
    return filters[k]


def scanlines(samples, color_type, depth=8, filters=0) -> bytes:
    """The seven passes' filtered scanlines back to back: what the IDAT stream inflates to."""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[:, :, None]
    h, w = s.shape[:2]
    out = b""
    for k, (x0, y0, dx, dy) in enumerate(PASSES):
        sub = s[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        out += pw.scanlines(sub, color_type, depth, pass_filters(filters, k, sub.shape[0]))
    return out


def write_png(samples, color_type, depth=8, filters=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, split=None, plte=None, trns=None, extra=()) -> bytes:
    """samples: (h, w) or (h, w, n) raw sample values (palette indices for colour type 3); see pass_filters for `filters`."""
    s = np.asarray(samples)
    h, w = s.shape[:2]
    stream = pw.deflate(scanlines(s, color_type, depth, filters), level, strategy)
    return pw.assemble(w, h, depth, color_type, stream, split, plte, trns, extra, interlace=1)
