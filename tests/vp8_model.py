"""The lossy WebP encoder (FLGPU_FE_WEBP_LOSSY, csrc/fl_vp8.hip) restated in numpy: planes + quality -> the file's bytes, with the
reconstruction the encoder predicts from.  Test infrastructure only.

The stream.  A simple-container file RIFF / WEBP / `VP8 ` (for a translucent picture RIFF / WEBP / VP8X (alpha flag) / ALPH
(compression 0, filter 0, the A plane raw) / `VP8 `) holding one key frame:
  * planes are padded to whole macroblocks by repeating the last row / column;
  * every macroblock is I16; the luma mode and the chroma mode (U and V together) are each the one of DC, V, H, TM with the least
    integer SSE of prediction against source, ties to the first in that order; borders as the decoder sees them (127 above the
    frame, 129 left of it, the corner 127 in the first row, else 129 in the first column; DC without neighbours 128);
  * quantiser index from quality by QUALITY_TO_INDEX (libwebp's curve for one segment -- recalled, unpinned); steps by the
    format's rules (Y2 DC x 2, Y2 AC x 155 / 100 with floor 8, UV DC index capped at 117, i.e. step 132), no deltas;
  * forward DCT / WHT in integers (fdct, fwht below); level = (|c| + bias) // step, bias = step >> 1 for a DC and 3 step >> 3
    for an AC coefficient, magnitude at most 2047; the reconstruction is the format's (dequantise, inverse WHT / DCT, clamp);
  * one segment, loop filter level 0, default coefficient probabilities (all 1056 update flags written as 0 with their update
    probabilities), mb_no_coeff_skip = 1 with prob_skip_false = max(1, (255 coded + total // 2) // total);
  * token partitions: 8 if there are at least 8 macroblock rows, else 4 if at least 4, else 2 if at least 2, else 1; row r goes
    to partition r mod n; the boolean coder ends every partition with 32 zero bits at probability 128.

The constant tables are read from csrc/fl_vp8_tables.h rather than typed a second time: their proof is not this model but
libwebp's decoder, which one wrong byte desynchronises (tests/test_webp_lossy_host.py)."""
import os
import re

import numpy as np

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fanlin-rs_amd", "csrc", "fl_vp8_tables.h")


def _tables():
    src = open(_HDR).read()
    out = {}
    for name, body in re.findall(r"constexpr uint\d+_t (\w+)\[[^\]]*\](?:\[[^\]]*\])? = \{(.*?)\};", src, re.S):
        body = re.sub(r"//[^\n]*", "", body)
        out[name] = [int(x) for x in re.findall(r"\d+", body)]
    return out


_T = _tables()
COEF_PROB = np.array(_T["kVp8CoefProb"], np.int64).reshape(4, 8, 3, 11).tolist()
UPDATE_PROB = _T["kVp8CoefUpdateProb"]
DC_STEP, AC_STEP = _T["kVp8DcStep"], _T["kVp8AcStep"]
ZIGZAG, BAND = _T["kVp8Zigzag"], _T["kVp8Band"]
QUALITY_TO_INDEX = _T["kVp8QualityToIndex"]
assert len(UPDATE_PROB) == 1056 and len(DC_STEP) == len(AC_STEP) == 128 and len(QUALITY_TO_INDEX) == 101
YMODE_PROB, UVMODE_PROB = (145, 156, 163, 128), (142, 114, 183)
CAT_PROB = ((159,), (165, 145), (173, 148, 140), (176, 155, 140, 135), (180, 157, 141, 134, 130),
            (254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129))
CAT_BASE = (5, 7, 11, 19, 35, 67)
DC, V, H, TM = 0, 1, 2, 3
MAX_LEVEL = 2047
MAX_SIDE = 16383


def quality_index_formula(quality):
    c = quality / 100.0
    lin = c * (2.0 / 3.0) if c < 0.75 else 2.0 * c - 1.0
    return 127.0 * (1.0 - lin ** (1.0 / 3.0))


def partitions(mb_rows):
    return 8 if mb_rows >= 8 else 4 if mb_rows >= 4 else 2 if mb_rows >= 2 else 1


def max_out_bytes(w, h):
    """A boolean costs at most 7 bits; partition 0 has 1126 + 7 per macroblock, a macroblock's tokens 384 x 19, every token
    partition's flush 32; framing 80 bytes and the raw alpha plane."""
    mbs = ((w + 15) // 16) * ((h + 15) // 16)
    return 80 + w * h + (7 * (1126 + 7 * mbs) + 7) // 8 + (7 * (384 * 19 * mbs + 8 * 32) + 7) // 8


def fits(w, h):
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        return False
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    max_mbs = (((1 << 19) - 1) * 8 // 7 - 1126) // 7
    n = partitions(mbh)
    rows = (mbh + n - 1) // n
    return mbw * mbh <= max_mbs and (7 * (384 * 19 * rows * mbw + 32) + 7) // 8 < (1 << 24)


def quant_steps(qi):
    return dict(y1=(DC_STEP[qi], AC_STEP[qi]), y2=(DC_STEP[qi] * 2, max(8, AC_STEP[qi] * 155 // 100)),
                uv=(DC_STEP[min(qi, 117)], AC_STEP[qi]))


# ---- transforms on arrays of 4x4 blocks [..., row, column], int64 -----------------------------------------------------------------

def fdct(d):
    x0, x1, x2, x3 = (d[..., :, k] for k in range(4))
    a0, a1, a2, a3 = x0 + x3, x1 + x2, x1 - x2, x0 - x3
    t = np.stack([(a0 + a1) * 8, (a2 * 2217 + a3 * 5352 + 1812) >> 9, (a0 - a1) * 8, (a3 * 2217 - a2 * 5352 + 937) >> 9], axis=-1)
    r0, r1, r2, r3 = (t[..., k, :] for k in range(4))
    a0, a1, a2, a3 = r0 + r3, r1 + r2, r1 - r2, r0 - r3
    return np.stack([(a0 + a1 + 7) >> 4, ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0), (a0 - a1 + 7) >> 4,
                     (a3 * 2217 - a2 * 5352 + 51000) >> 16], axis=-2)


def fwht(d):
    x0, x1, x2, x3 = (d[..., :, k] for k in range(4))
    a0, a1, a2, a3 = x0 + x2, x1 + x3, x1 - x3, x0 - x2
    t = np.stack([a0 + a1, a3 + a2, a3 - a2, a0 - a1], axis=-1)
    r0, r1, r2, r3 = (t[..., k, :] for k in range(4))
    a0, a1, a2, a3 = r0 + r2, r1 + r3, r1 - r3, r0 - r2
    return np.stack([(a0 + a1) >> 1, (a3 + a2) >> 1, (a3 - a2) >> 1, (a0 - a1) >> 1], axis=-2)


def iwht(c):
    r0, r1, r2, r3 = (c[..., k, :] for k in range(4))
    a0, a1, a2, a3 = r0 + r3, r1 + r2, r1 - r2, r0 - r3
    t = np.stack([a0 + a1, a3 + a2, a0 - a1, a3 - a2], axis=-2)
    x0, x1, x2, x3 = (t[..., :, k] for k in range(4))
    d = x0 + 3
    a0, a1, a2, a3 = d + x3, x1 + x2, x1 - x2, d - x3
    return np.stack([(a0 + a1) >> 3, (a3 + a2) >> 3, (a0 - a1) >> 3, (a3 - a2) >> 3], axis=-1)


def _mul1(a):
    return ((a * 20091) >> 16) + a


def _mul2(a):
    return (a * 35468) >> 16


def idct(c):
    r0, r1, r2, r3 = (c[..., k, :] for k in range(4))
    a, b = r0 + r2, r0 - r2
    cc, d = _mul2(r1) - _mul1(r3), _mul1(r1) + _mul2(r3)
    t = np.stack([a + d, b + cc, b - cc, a - d], axis=-2)
    x0, x1, x2, x3 = (t[..., :, k] for k in range(4))
    dc = x0 + 4
    a, b = dc + x2, dc - x2
    cc, d = _mul2(x1) - _mul1(x3), _mul1(x1) + _mul2(x3)
    return np.stack([(a + d) >> 3, (b + cc) >> 3, (b - cc) >> 3, (a - d) >> 3], axis=-1)


def quantise(c, step_dc, step_ac, with_dc=True):
    """c: [..., 4, 4] raster -> levels, raster."""
    step = np.full((4, 4), step_ac, np.int64)
    bias = np.full((4, 4), (step_ac * 3) >> 3, np.int64)
    step[0, 0], bias[0, 0] = step_dc, step_dc >> 1
    lev = np.minimum((np.abs(c) + bias) // step, MAX_LEVEL) * np.sign(c)
    if not with_dc:
        lev[..., 0, 0] = 0
    return lev, lev * step


# ---- prediction -------------------------------------------------------------------------------------------------------------------

def predictions(rec, mbx, mby, n):
    """The four predictions of the n x n square at macroblock (mbx, mby) of the reconstructed plane rec (padded)."""
    x0, y0 = mbx * n, mby * n
    top = rec[y0 - 1, x0:x0 + n].astype(np.int64) if mby else np.full(n, 127, np.int64)
    left = rec[y0:y0 + n, x0 - 1].astype(np.int64) if mbx else np.full(n, 129, np.int64)
    corner = 127 if mby == 0 else 129 if mbx == 0 else int(rec[y0 - 1, x0 - 1])
    sh = 4 if n == 16 else 3
    if mby and mbx:
        dc = (int(top.sum()) + int(left.sum()) + n) >> (sh + 1)
    elif mby:
        dc = (int(top.sum()) + n // 2) >> sh
    elif mbx:
        dc = (int(left.sum()) + n // 2) >> sh
    else:
        dc = 128
    return [np.full((n, n), dc, np.int64), np.tile(top, (n, 1)), np.tile(left[:, None], (1, n)),
            np.clip(top[None, :] + left[:, None] - corner, 0, 255)]


def _blocks(sq):
    """n x n square -> its 4x4 blocks in raster order, [blocks, 4, 4]."""
    n = sq.shape[0] // 4
    return sq.reshape(n, 4, n, 4).transpose(0, 2, 1, 3).reshape(n * n, 4, 4)


def _unblocks(b):
    n = int(round(len(b) ** 0.5))
    return b.reshape(n, n, 4, 4).transpose(0, 2, 1, 3).reshape(4 * n, 4 * n)


# ---- boolean coder ----------------------------------------------------------------------------------------------------------------

class BoolWriter:
    def __init__(self):
        self.low, self.range, self.count, self.buf = 0, 255, -24, bytearray()

    def put(self, bit, prob):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.low += split
            self.range -= split
        else:
            self.range = split
        shift = 8 - self.range.bit_length()
        self.range <<= shift
        self.count += shift
        if self.count >= 0:
            offset = shift - self.count
            if (self.low << (offset - 1)) & 0x80000000:
                x = len(self.buf) - 1
                while x >= 0 and self.buf[x] == 0xFF:
                    self.buf[x] = 0
                    x -= 1
                self.buf[x] += 1
            self.buf.append((self.low >> (24 - offset)) & 0xFF)
            self.low = (self.low << offset) & 0xFFFFFF
            shift = self.count
            self.count -= 8
        self.low <<= shift

    def literal(self, v, bits):
        for b in range(bits - 1, -1, -1):
            self.put((v >> b) & 1, 128)

    def finish(self):
        for _ in range(32):
            self.put(0, 128)
        return bytes(self.buf)


def put_block(bw, lev, btype, first, ctx, stats):
    """lev: 16 levels in coding order."""
    last = -1
    for i in range(first, 16):
        if lev[i]:
            last = i
    n = first
    p = COEF_PROB[btype][BAND[n]][ctx]
    bw.put(last >= 0, p[0])
    if last < 0:
        return
    while n < 16:
        c = lev[n]
        n += 1
        v = abs(c)
        if v == 0:
            bw.put(0, p[1])
            p = COEF_PROB[btype][BAND[n]][0]
            continue
        bw.put(1, p[1])
        if v == 1:
            bw.put(0, p[2])
            p = COEF_PROB[btype][BAND[n]][1]
        else:
            bw.put(1, p[2])
            if v <= 4:
                bw.put(0, p[3])
                bw.put(v != 2, p[4])
                if v != 2:
                    bw.put(v == 4, p[5])
            else:
                bw.put(1, p[3])
                if v <= 10:
                    bw.put(0, p[6])
                    cat = int(v > 6)
                    bw.put(cat, p[7])
                else:
                    bw.put(1, p[6])
                    cat = 2 if v < 19 else 3 if v < 35 else 4 if v < 67 else 5
                    bw.put(cat >= 4, p[8])
                    bw.put(cat & 1, p[10 if cat >= 4 else 9])
                    stats["cat6"] = stats["cat6"] or cat == 5
                extra = v - CAT_BASE[cat]
                probs = CAT_PROB[cat]
                for t, pr in enumerate(probs):
                    bw.put((extra >> (len(probs) - 1 - t)) & 1, pr)
            p = COEF_PROB[btype][BAND[n]][2]
        bw.put(c < 0, 128)
        if n == 16:
            return
        bw.put(n <= last, p[0])
        if n > last:
            return


# ---- the encoder --------------------------------------------------------------------------------------------------------------------

def encode(y, u, v, quality, a=None):
    """y: [h, w]; u, v: [ceil(h / 2), ceil(w / 2)]; a: the alpha plane of a translucent picture or None.
    -> (file bytes, (reconstructed y, u, v), stats) with stats = dict(ymodes, uvmodes (sets), cat6, skipped, partitions)."""
    h, w = y.shape
    assert fits(w, h) and u.shape == v.shape == ((h + 1) // 2, (w + 1) // 2)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    qi = QUALITY_TO_INDEX[min(max(int(quality), 1), 100)]
    steps = quant_steps(qi)
    src = [np.pad(p, ((0, n * mbh - p.shape[0]), (0, n * mbw - p.shape[1])), mode="edge").astype(np.int64)
           for p, n in ((y, 16), (u, 8), (v, 8))]
    rec = [np.zeros_like(s, dtype=np.uint8) for s in src]
    zz = np.array(ZIGZAG)
    levels = np.zeros((mbh, mbw, 25, 16), np.int64)   # coding order; block 24 is Y2
    nz = np.zeros((mbh, mbw, 25), np.int64)
    modes = np.zeros((mbh, mbw, 2), np.int64)
    stats = dict(ymodes=set(), uvmodes=set(), cat6=False, skipped=0, partitions=partitions(mbh))
    for mby in range(mbh):
        for mbx in range(mbw):
            sy = src[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16]
            py = predictions(rec[0], mbx, mby, 16)
            ym = int(np.argmin([int(((sy - p) ** 2).sum()) for p in py]))     # argmin: the first of equals
            pc = [predictions(rec[k], mbx, mby, 8) for k in (1, 2)]
            sc = [src[k][mby * 8:mby * 8 + 8, mbx * 8:mbx * 8 + 8] for k in (1, 2)]
            uvm = int(np.argmin([int(((sc[0] - pc[0][m]) ** 2).sum()) + int(((sc[1] - pc[1][m]) ** 2).sum()) for m in range(4)]))
            modes[mby, mbx] = ym, uvm
            stats["ymodes"].add(ym)
            stats["uvmodes"].add(uvm)
            # luma: DCT, the DCs through the WHT
            cy = fdct(_blocks(sy - py[ym]))
            y2 = fwht(cy[:, 0, 0].reshape(4, 4))
            l2, dq2 = quantise(y2, *steps["y2"])
            dcs = iwht(dq2).reshape(16)
            ly, dqy = quantise(cy, *steps["y1"], with_dc=False)
            dqy[:, 0, 0] = dcs
            rec[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = np.clip(py[ym] + _unblocks(idct(dqy)), 0, 255)
            levels[mby, mbx, :16] = ly.reshape(16, 16)[:, zz]
            levels[mby, mbx, 24] = l2.reshape(16)[zz]
            for k in (0, 1):
                cc = fdct(_blocks(sc[k] - pc[k][uvm]))
                lc, dqc = quantise(cc, *steps["uv"])
                rec[1 + k][mby * 8:mby * 8 + 8, mbx * 8:mbx * 8 + 8] = np.clip(pc[k][uvm] + _unblocks(idct(dqc)), 0, 255)
                levels[mby, mbx, 16 + 4 * k:20 + 4 * k] = lc.reshape(4, 16)[:, zz]
            nz[mby, mbx] = (levels[mby, mbx] != 0).any(axis=1)
    skip = ~nz.any(axis=2)
    stats["skipped"] = int(skip.sum())
    nparts = stats["partitions"]

    # partition 0
    bw = BoolWriter()
    for v_, bits in ((0, 1), (0, 1), (0, 1), (0, 1), (0, 6), (0, 3), (0, 1), ({1: 0, 2: 1, 4: 2, 8: 3}[nparts], 2), (qi, 7),
                     (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        bw.literal(v_, bits)
    for p in UPDATE_PROB:
        bw.put(0, p)
    total = mbw * mbh
    ps = max(1, ((total - stats["skipped"]) * 255 + total // 2) // total)
    bw.literal(1, 1)
    bw.literal(ps, 8)
    for mby in range(mbh):
        for mbx in range(mbw):
            ym, uvm = int(modes[mby, mbx, 0]), int(modes[mby, mbx, 1])
            bw.put(bool(skip[mby, mbx]), ps)
            bw.put(1, YMODE_PROB[0])
            bw.put(ym >= 2, YMODE_PROB[1])
            bw.put(ym & 1, YMODE_PROB[3] if ym >= 2 else YMODE_PROB[2])
            bw.put(uvm != 0, UVMODE_PROB[0])
            if uvm:
                bw.put(uvm != 1, UVMODE_PROB[1])
                if uvm != 1:
                    bw.put(uvm == 3, UVMODE_PROB[2])
    parts = [bw.finish()]

    # token partitions
    zero = np.zeros(25, np.int64)
    for part in range(nparts):
        bw = BoolWriter()
        for mby in range(part, mbh, nparts):
            for mbx in range(mbw):
                if skip[mby, mbx]:
                    continue
                me, lf, tp = nz[mby, mbx], (nz[mby, mbx - 1] if mbx else zero), (nz[mby - 1, mbx] if mby else zero)
                lev = levels[mby, mbx].tolist()
                put_block(bw, lev[24], 1, 0, int(lf[24] + tp[24]), stats)
                for b in range(16):
                    l = me[b - 1] if b & 3 else lf[b + 3]
                    t = me[b - 4] if b >> 2 else tp[b + 12]
                    put_block(bw, lev[b], 0, 1, int(l + t), stats)
                for b in range(16, 24):
                    l = me[b - 1] if b & 1 else lf[b + 1]
                    t = me[b - 2] if b & 2 else tp[b + 2]
                    put_block(bw, lev[b], 2, 0, int(l + t), stats)
        parts.append(bw.finish())

    # the file
    frame = bytearray()
    frame += (0 | 0 << 1 | 1 << 4 | len(parts[0]) << 5).to_bytes(3, "little") + b"\x9d\x01\x2a"
    frame += w.to_bytes(2, "little") + h.to_bytes(2, "little")
    frame += parts[0]
    for p in parts[1:-1]:
        frame += len(p).to_bytes(3, "little")
    for p in parts[1:]:
        frame += p

    def chunk(tag, payload):
        return tag + len(payload).to_bytes(4, "little") + bytes(payload) + (b"\0" if len(payload) & 1 else b"")
    body = b"WEBP"
    if a is not None:
        body += chunk(b"VP8X", (0x10).to_bytes(4, "little") + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little"))
        body += chunk(b"ALPH", b"\0" + np.ascontiguousarray(a, dtype=np.uint8).tobytes())
    body += chunk(b"VP8 ", frame)
    data = b"RIFF" + len(body).to_bytes(4, "little") + body
    return data, (rec[0][:h, :w].copy(), rec[1][:(h + 1) // 2, :(w + 1) // 2].copy(), rec[2][:(h + 1) // 2, :(w + 1) // 2].copy()), stats
