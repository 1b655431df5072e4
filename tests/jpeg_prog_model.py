"""FLGPU_FEO_JPEG_PROGRESSIVE restated in numpy: from the oracle's quantised coefficients (oracle.jpeg_coefficients) and its header
(oracle.jpeg_header) to a progressive file (SOF2) of five scans by spectral selection -- DC of all components interleaved, then Y 1-5,
Cb 1-63, Cr 1-63, Y 6-63 -- each AC scan coded as T.81 G.1.2.2 says (end-of-band runs across blocks), every table built by the rule of
csrc/fl_jpeg_opt_core.h (jpeg_opt_model.rule) from the scan's own counts.  Tables are numbered in file order:
0 DC luma, 1 DC chroma, 2 .. 5 the AC tables of scans 2 .. 5."""
import numpy as np

import jpeg_opt_model as jm

PREFIX_BYTES = jm.PREFIX_BYTES
SOF_MARKER_AT = 21                                    # the one prefix byte that differs from the baseline file: 0xC0 -> 0xC2
AC_SCANS = ((0, 1, 5), (1, 1, 63), (2, 1, 63), (0, 6, 63))   # (component, Ss, Se) of scans 2 .. 5
EOB_RUN_LIMIT = 32767
DC_SOS = bytes([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x10, 3, 0x10, 0, 0, 0])


def ac_sos(comp, ss, se):
    return bytes([0xFF, 0xDA, 0, 8, 1, comp + 1, 0x00, ss, se, 0])


def dc_symbols(coef):
    """[(table 0 / 1, size, value, size)] of scan 1: per block Y, Cb, Cr, the baseline's differential DC coding"""
    dc = np.asarray(coef, np.int64)[:, 0].reshape(-1, 3)
    diff = dc - np.vstack([np.zeros((1, 3), np.int64), dc[:-1]])
    out = []
    for row in diff:
        for comp in range(3):
            s = jm._size(row[comp])
            out.append((1 if comp else 0, s, jm._value(row[comp], s), s))
    return out


def ac_symbols(blocks, ss, se):
    """[(0, symbol, value, value bits)] of one AC scan over one component's blocks [block][64] in raster order: encode_mcu_AC_first
    without restarts.  Only the blocks that hold a coefficient in the band are walked."""
    band = np.asarray(blocks, np.int64)[:, ss:se + 1]
    n = len(band)
    busy = np.nonzero(band.any(axis=1))[0]
    tail = band[:, -1] == 0
    out = []
    run = 0

    def flush():
        nonlocal run
        if run:
            k = run.bit_length() - 1
            out.append((0, k << 4, run - (1 << k), k))
            run = 0

    def lengthen(k):
        nonlocal run
        while k:
            step = min(k, EOB_RUN_LIMIT - run)
            run += step
            k -= step
            if run == EOB_RUN_LIMIT:
                flush()

    prev = -1
    for b in busy:
        lengthen(int(b) - prev - 1)           # the empty blocks in between: each ends in a zero
        flush()                               # the pending run goes out in front of this block's first coefficient
        zeros = 0
        for v in band[b]:
            if v == 0:
                zeros += 1
                continue
            while zeros > 15:
                out.append((0, 0xF0, 0, 0))
                zeros -= 16
            s = jm._size(v)
            out.append((0, (zeros << 4) | s, jm._value(v, s), s))
            zeros = 0
        if tail[b]:
            lengthen(1)
        prev = int(b)
    lengthen(n - prev - 1)
    flush()
    return out


def _counts(syms, tables):
    cnt = np.zeros((tables, 256), np.uint32)
    for t, s, _, _ in syms:
        cnt[t, s] += 1
    return cnt


def encode_coefficients(header, coef):
    """(file, info) from the baseline header and coefficients [unit][64], unit = 3 * block + component.  info: counts uint32[6][256],
    rules (jpeg_opt_model.rule per table), scans = the five scans' symbol lists."""
    coef = np.asarray(coef, np.int16)
    comps = coef.reshape(-1, 3, 64)
    scans = [dc_symbols(coef)] + [ac_symbols(comps[:, c], ss, se) for c, ss, se in AC_SCANS]
    counts = np.concatenate([_counts(scans[0], 2)] + [_counts(s, 1) for s in scans[1:]])
    rules = [jm.rule(c) for c in counts]
    out = bytearray(header[:PREFIX_BYTES])
    assert out[SOF_MARKER_AT - 1] == 0xFF and out[SOF_MARKER_AT] == 0xC0
    out[SOF_MARKER_AT] = 0xC2
    out += jm.dht_segment(0, rules[0]) + jm.dht_segment(2, rules[1]) + DC_SOS
    out += jm.code_scan(scans[0], [rules[0]["lut"], rules[1]["lut"]])
    for k, (c, ss, se) in enumerate(AC_SCANS):
        out += jm.dht_segment(1, rules[2 + k]) + ac_sos(c, ss, se) + jm.code_scan(scans[1 + k], [rules[2 + k]["lut"]])
    out += b"\xff\xd9"
    return bytes(out), dict(counts=counts, rules=rules, scans=scans)


def encode(oracle, img, q):
    """(file, info) of FE_JPEG with FEO_JPEG_PROGRESSIVE"""
    h, w = img.shape[:2]
    return encode_coefficients(oracle.jpeg_header(w, h, q), oracle.jpeg_coefficients(img, q))
