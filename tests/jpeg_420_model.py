"""FLGPU_FEO_JPEG_420 restated in numpy ("4:2:0 chroma subsampling"): the oracle's per-pixel Y, Cb, Cr bytes
(oracle.jpeg_ycbcr444) edge-padded to multiples of 16, the 2 x 2 average of Cb and Cr, the oracle's fdct per block, the quantiser
restated, and one interleaved scan of 16 x 16 MCUs -- Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr -- coded by tests/jpeg_opt_model.py's coder with
the Annex K tables of the oracle's header, whose SOF0 gets the one byte 0x22.  With FEO_JPEG_OPTIMIZE as well, the counts of this scan
go through that model's unchanged rule and decision.  The reference never writes 4:2:0: these bytes are the project's own rule."""
import numpy as np

import jpeg_opt_model as jm

UNZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                     28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                     47, 55, 62, 63])
COMPONENTS = (0, 0, 0, 0, 1, 2)      # of the six units of an MCU
SOF0_Y_SAMPLING = 31                 # offset of the sampling byte of SOF0's first component: SOI 2, APP0 18, SOF0's marker and length 4, 6 fixed bytes, id 1


def planes(oracle, img):
    """(Y, Cb, Cr): Y on the area rounded up to 16s, Cb and Cr averaged 2 x 2 on it; replicated edge pixels take part in the average."""
    h, w = img.shape[:2]
    ph, pw = (h + 15) & ~15, (w + 15) & ~15
    full = [np.pad(p, ((0, ph - p.shape[0]), (0, pw - p.shape[1])), mode="edge") for p in oracle.jpeg_ycbcr444(img)]

    def half(c):
        c = c.astype(np.uint32)
        return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return full[0], half(full[1]), half(full[2])


def quantise(d, q):
    """encode_rgb: ((d / 8) as f32 / f32::from(q)).round() as i32 -- i32 division truncates, f32::round is half away from zero."""
    d = np.asarray(d, np.int64)
    t = np.sign(d) * (np.abs(d) // 8)
    x = t.astype(np.float32) / np.asarray(q, np.float32)
    return (np.sign(x) * np.floor(np.abs(x).astype(np.float64) + 0.5)).astype(np.int64)


def _unit(oracle, plane, by, bx, qtab):
    d = oracle.jpeg_fdct(plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8]).reshape(64)
    return quantise(d, qtab.astype(np.int64)).reshape(64)[UNZIGZAG]


def coefficients(oracle, img, q):
    """[unit][64] int16 in scan order, unit = 6 * MCU + slot, zig-zag order."""
    y, cb, cr = planes(oracle, img)
    luma, chroma = oracle.jpeg_qtables(q)
    out = []
    for my in range(y.shape[0] // 16):
        for mx in range(y.shape[1] // 16):
            out += [_unit(oracle, y, 2 * my + (k >> 1), 2 * mx + (k & 1), luma) for k in range(4)]
            out += [_unit(oracle, cb, my, mx, chroma), _unit(oracle, cr, my, mx, chroma)]
    return np.array(out, np.int16)


def symbols(coef):
    """jpeg_opt_model.symbols for this scan: the DC predictor runs per component along the scan's order."""
    out = []
    prev = [0, 0, 0]
    for u, c in enumerate(np.asarray(coef, np.int64)):
        comp = COMPONENTS[u % 6]
        diff = int(c[0]) - prev[comp]
        prev[comp] = int(c[0])
        s = jm._size(diff)
        out.append((2 if comp else 0, s, jm._value(diff, s), s))
        t = 3 if comp else 1
        last = 0
        for pos in np.nonzero(c[1:])[0] + 1:
            run = int(pos) - last - 1
            last = int(pos)
            while run > 15:
                out.append((t, 0xF0, 0, 0))
                run -= 16
            s = jm._size(c[pos])
            out.append((t, (run << 4) | s, jm._value(c[pos], s), s))
        if last != 63:
            out.append((t, 0x00, 0, 0))
    return out


def header(oracle, w, h, q):
    hd = bytearray(oracle.jpeg_header(w, h, q))
    assert len(hd) == jm.STD_HEADER_BYTES and hd[SOF0_Y_SAMPLING - 1:SOF0_Y_SAMPLING + 1] == b"\x01\x11"
    hd[SOF0_Y_SAMPLING] = 0x22
    return bytes(hd)


def encode(oracle, img, q, optimize=False, fallback=False):
    """(file, info) of FE_JPEG with FEO_JPEG_420 (and FEO_JPEG_OPTIMIZE); info: coef, syms, and with optimize tables_of's fields and the counts."""
    h, w = img.shape[:2]
    hd = header(oracle, w, h, q)
    coef = coefficients(oracle, img, q)
    syms = symbols(coef)
    std = jm.standard_tables(hd)
    info = dict(coef=coef, syms=syms, optimized=False)
    if optimize:
        cnt = jm.counts(syms)
        info.update(jm.tables_of(cnt, std, fallback))
        info["counts"] = cnt
    if not info["optimized"]:
        return hd + jm.code_scan(syms, std) + b"\xff\xd9", info
    return hd[:jm.PREFIX_BYTES] + info["dht"] + hd[-jm.SOS_BYTES:] + jm.code_scan(syms, info["luts"]) + b"\xff\xd9", info


def file_order(coef, w, h):
    """The model's coefficients as oracle.jpeg_file_coefficients lists a file's: per component, blocks in raster order of the padded plane."""
    mw, mh = (w + 15) // 16, (h + 15) // 16
    c = np.asarray(coef).reshape(mh, mw, 6, 64)
    y = c[:, :, :4].reshape(mh, mw, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)
    return np.concatenate([y, c[:, :, 4].reshape(-1, 64), c[:, :, 5].reshape(-1, 64)])
