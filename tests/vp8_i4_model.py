"""The I4 variant of the lossy WebP encoder (FLGPU_FE_WEBP_LOSSY_I4, csrc/fl_vp8_i4_core.h) restated in numpy on top of
tests/vp8_model.py: planes + quality -> the file's bytes, the reconstruction and the per-macroblock mode map.  Test infrastructure
only.

The stream is vp8_model's, except that a macroblock's luma may be B_PRED.  Per macroblock, in raster order:
  1. the I16 trial, exactly vp8_model's; S16 = the SSE of the chosen luma prediction against the source.  Chroma never changes.
  2. the I4 trial: the sixteen 4x4 luma sub-blocks in raster order.  Each forms the ten predictions B_DC, B_TM, B_VE, B_HE, B_LD,
     B_RD, B_VR, B_VL, B_HD, B_HU (RFC 6386's numbering, 0..9) from the reconstruction -- the sub-blocks before it in this trial, the
     committed row above / column to the left of the macroblock; 127 above the frame, 129 left of it; the four samples above and to
     the right come, for the sub-blocks of the last column in every row, from the row above the macroblock (past the frame's right
     edge: that row's last sample) --, takes the one with the least SSE against the source (ties: the lowest number), transforms
     the residual (vp8_model.fdct), quantises all sixteen coefficients with the y1 steps (DC to nearest, AC with the dead zone),
     dequantises, inverts, adds the prediction and clamps.  S4 = the sum of the sixteen chosen SSEs.
  3. the macroblock is B_PRED iff S4 + penalty(y1 AC step) < S16, penalty = max(1, step^4 >> PENALTY_SHIFT).
  4. the chosen trial is committed; later macroblocks see only that.
Partition 0 codes a B_PRED macroblock as 0 at the luma tree's root and sixteen modes through the sub-block tree in the context of
the modes above and to the left (an I16 macroblock stands for B_DC / B_VE / B_HE / B_TM, outside the frame is B_DC); its tokens
have no Y2 block, luma blocks of type 3 from coefficient 0, and leave the Y2 context of its column and row alone; it is skipped
when its 24 blocks are zero.

The tree's probabilities are read from csrc/fl_vp8_dtables.h (numbered DC, TM, VE, HE, RD, VR, LD, VL, HD, HU there): libwebp's
decoder is their proof, as for vp8_model's tables."""
import os
import re

import numpy as np

import vp8_model as vm

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fanlin-rs_amd", "csrc", "fl_vp8_dtables.h")
_body = re.search(r"kVp8BModeProb\[[^\]]*\] = \{(.*?)\};", open(_HDR).read(), re.S).group(1)
BMODE_PROB = np.array([int(x) for x in re.findall(r"\d+", re.sub(r"//[^\n]*", "", _body))], np.int64).reshape(10, 10, 9).tolist()

# RFC numbering (the order of the trial and of its ties) and the table's numbering (what the mode map and the contexts hold)
RFC_NAMES = ("B_DC", "B_TM", "B_VE", "B_HE", "B_LD", "B_RD", "B_VR", "B_VL", "B_HD", "B_HU")
T_DC, T_TM, T_VE, T_HE, T_RD, T_VR, T_LD, T_VL, T_HD, T_HU = range(10)
RFC_TO_TABLE = (T_DC, T_TM, T_VE, T_HE, T_LD, T_RD, T_VR, T_VL, T_HD, T_HU)
# the tree of section 11.2 as (node, bit) paths, by the table's numbering
_TREE = {T_DC: ((0, 0),), T_TM: ((0, 1), (1, 0)), T_VE: ((0, 1), (1, 1), (2, 0)),
         T_HE: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 0)), T_RD: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 0)),
         T_VR: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 1)), T_LD: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 0)),
         T_VL: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 0)), T_HD: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 0)),
         T_HU: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 1))}
I16_CONTEXT = {vm.DC: T_DC, vm.V: T_VE, vm.H: T_HE, vm.TM: T_TM}

PENALTY_SHIFT = 9
PART0_MB_BOOLS = 1 + 1 + 16 * 7 + 3
MAX_MBS = (((1 << 19) - 1) * 8 // 7 - 1126) // PART0_MB_BOOLS


def penalty(ac_step, shift=None):
    return max(1, ac_step ** 4 >> (PENALTY_SHIFT if shift is None else shift))


def max_out_bytes(w, h):
    """vp8_model's, with 117 booleans per macroblock in partition 0 instead of 7."""
    mbs = ((w + 15) // 16) * ((h + 15) // 16)
    return vm.max_out_bytes(w, h) - (7 * (1126 + 7 * mbs) + 7) // 8 + (7 * (1126 + PART0_MB_BOOLS * mbs) + 7) // 8


def fits(w, h):
    return vm.fits(w, h) and ((w + 15) // 16) * ((h + 15) // 16) <= MAX_MBS


def _avg2(a, b):
    return (a + b + 1) >> 1


def _avg3(a, b, c):
    return (a + 2 * b + c + 2) >> 2


def predictions4(A, L, P):
    """A: the 8 samples above and above-right, L: the 4 to the left (top to bottom), P: the corner -> the ten 4x4 predictions in RFC
    order, B[row][column] as section 12.3 writes them out."""
    A, L, P = [int(x) for x in A], [int(x) for x in L], int(P)
    E = [L[3], L[2], L[1], L[0], P] + A      # the edge, from the bottom of the left column to the end of the row above
    out = []
    out.append(np.full((4, 4), (sum(A[:4]) + sum(L) + 4) >> 3, np.int64))
    out.append(np.clip(np.array(A[:4])[None, :] + np.array(L)[:, None] - P, 0, 255).astype(np.int64))
    out.append(np.tile(np.array([_avg3(E[4 + x], E[5 + x], E[6 + x]) for x in range(4)], np.int64), (4, 1)))
    out.append(np.tile(np.array([_avg3(P, L[0], L[1]), _avg3(L[0], L[1], L[2]), _avg3(L[1], L[2], L[3]), _avg3(L[2], L[3], L[3])], np.int64)[:, None], (1, 4)))
    B = np.zeros((4, 4), np.int64)           # LD
    for r in range(4):
        for c in range(4):
            i = r + c
            B[r, c] = _avg3(A[i], A[i + 1], A[i + 2]) if i < 6 else _avg3(A[6], A[7], A[7])
    out.append(B)
    B = np.zeros((4, 4), np.int64)           # RD
    for r in range(4):
        for c in range(4):
            i = 4 + c - r
            B[r, c] = _avg3(E[i - 1], E[i], E[i + 1])
    out.append(B)
    B = np.zeros((4, 4), np.int64)           # VR
    B[3, 0] = _avg3(E[1], E[2], E[3]); B[2, 0] = _avg3(E[2], E[3], E[4])
    B[3, 1] = B[1, 0] = _avg3(E[3], E[4], E[5]); B[2, 1] = B[0, 0] = _avg2(E[4], E[5])
    B[3, 2] = B[1, 1] = _avg3(E[4], E[5], E[6]); B[2, 2] = B[0, 1] = _avg2(E[5], E[6])
    B[3, 3] = B[1, 2] = _avg3(E[5], E[6], E[7]); B[2, 3] = B[0, 2] = _avg2(E[6], E[7])
    B[1, 3] = _avg3(E[6], E[7], E[8]); B[0, 3] = _avg2(E[7], E[8])
    out.append(B)
    B = np.zeros((4, 4), np.int64)           # VL
    B[0, 0] = _avg2(A[0], A[1]); B[1, 0] = _avg3(A[0], A[1], A[2])
    B[2, 0] = B[0, 1] = _avg2(A[1], A[2]); B[1, 1] = B[3, 0] = _avg3(A[1], A[2], A[3])
    B[2, 1] = B[0, 2] = _avg2(A[2], A[3]); B[3, 1] = B[1, 2] = _avg3(A[2], A[3], A[4])
    B[2, 2] = B[0, 3] = _avg2(A[3], A[4]); B[3, 2] = B[1, 3] = _avg3(A[3], A[4], A[5])
    B[2, 3] = _avg3(A[4], A[5], A[6]); B[3, 3] = _avg3(A[5], A[6], A[7])
    out.append(B)
    B = np.zeros((4, 4), np.int64)           # HD
    B[3, 0] = _avg2(E[0], E[1]); B[3, 1] = _avg3(E[0], E[1], E[2])
    B[2, 0] = B[3, 2] = _avg2(E[1], E[2]); B[2, 1] = B[3, 3] = _avg3(E[1], E[2], E[3])
    B[2, 2] = B[1, 0] = _avg2(E[2], E[3]); B[2, 3] = B[1, 1] = _avg3(E[2], E[3], E[4])
    B[1, 2] = B[0, 0] = _avg2(E[3], E[4]); B[1, 3] = B[0, 1] = _avg3(E[3], E[4], E[5])
    B[0, 2] = _avg3(E[4], E[5], E[6]); B[0, 3] = _avg3(E[5], E[6], E[7])
    out.append(B)
    B = np.zeros((4, 4), np.int64)           # HU
    B[0, 0] = _avg2(L[0], L[1]); B[0, 1] = _avg3(L[0], L[1], L[2])
    B[0, 2] = B[1, 0] = _avg2(L[1], L[2]); B[0, 3] = B[1, 1] = _avg3(L[1], L[2], L[3])
    B[1, 2] = B[2, 0] = _avg2(L[2], L[3]); B[1, 3] = B[2, 1] = _avg3(L[2], L[3], L[3])
    B[2, 2] = B[2, 3] = B[3, 0] = B[3, 1] = B[3, 2] = B[3, 3] = L[3]
    out.append(B)
    return out


def i4_trial(sy, rec, mbx, mby, steps):
    """-> (S4, the 16x16 reconstruction, levels [16, 16] in coding order, modes [16] in RFC numbering)."""
    zz = np.array(vm.ZIGZAG)
    x0, y0 = mbx * 16, mby * 16
    wide = rec.shape[1]
    # a frame around the working copy: row 0 = the row above with the corner and 4 samples to the right, column 0 = the left column
    f = np.zeros((17, 21), np.int64)
    if mby:
        f[0, 1:] = [rec[y0 - 1, min(x0 + i, wide - 1)] for i in range(20)]
    else:
        f[0, 1:] = 127
    f[1:, 0] = rec[y0:y0 + 16, x0 - 1] if mbx else 129
    f[0, 0] = 127 if mby == 0 else 129 if mbx == 0 else int(rec[y0 - 1, x0 - 1])
    s4, levels, modes = 0, np.zeros((16, 16), np.int64), []
    for b in range(16):
        bx, by = (b & 3) * 4, (b >> 2) * 4
        A = list(f[by, 1 + bx:1 + bx + 4]) + (list(f[0, 17:21]) if bx == 12 else list(f[by, 5 + bx:9 + bx]))
        preds = predictions4(A, f[1 + by:5 + by, bx], f[by, bx])
        s = sy[by:by + 4, bx:bx + 4]
        sse = [int(((s - p) ** 2).sum()) for p in preds]
        m = int(np.argmin(sse))
        s4 += sse[m]
        modes.append(m)
        lev, dq = vm.quantise(vm.fdct(s - preds[m]), *steps)
        f[1 + by:5 + by, 1 + bx:5 + bx] = np.clip(preds[m] + vm.idct(dq), 0, 255)
        levels[b] = lev.reshape(16)[zz]
    return s4, f[1:, 1:17].astype(np.uint8), levels, modes


def encode(y, u, v, quality, a=None, penalty_shift=None):
    """As vp8_model.encode -> (file bytes, (reconstructed y, u, v), stats); stats adds
    i4 [mbh, mbw] bool, bmodes [mbh, mbw, 16] (RFC numbering; -1 in an I16 macroblock), ymode [mbh, mbw] (-1 in a B_PRED macroblock),
    skip [mbh, mbw] bool."""
    h, w = y.shape
    assert fits(w, h) and u.shape == v.shape == ((h + 1) // 2, (w + 1) // 2)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    qi = vm.QUALITY_TO_INDEX[min(max(int(quality), 1), 100)]
    steps = vm.quant_steps(qi)
    pen = penalty(steps["y1"][1], penalty_shift)
    src = [np.pad(p, ((0, n * mbh - p.shape[0]), (0, n * mbw - p.shape[1])), mode="edge").astype(np.int64)
           for p, n in ((y, 16), (u, 8), (v, 8))]
    rec = [np.zeros_like(s, dtype=np.uint8) for s in src]
    zz = np.array(vm.ZIGZAG)
    levels = np.zeros((mbh, mbw, 25, 16), np.int64)
    nz = np.zeros((mbh, mbw, 25), np.int64)
    modes = np.zeros((mbh, mbw, 2), np.int64)
    is4 = np.zeros((mbh, mbw), bool)
    bmodes = np.full((mbh, mbw, 16), -1, np.int64)
    stats = dict(ymodes=set(), uvmodes=set(), cat6=False, skipped=0, partitions=vm.partitions(mbh))
    for mby in range(mbh):
        for mbx in range(mbw):
            sy = src[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16]
            py = vm.predictions(rec[0], mbx, mby, 16)
            sse16 = [int(((sy - p) ** 2).sum()) for p in py]
            ym = int(np.argmin(sse16))
            pc = [vm.predictions(rec[k], mbx, mby, 8) for k in (1, 2)]
            sc = [src[k][mby * 8:mby * 8 + 8, mbx * 8:mbx * 8 + 8] for k in (1, 2)]
            uvm = int(np.argmin([int(((sc[0] - pc[0][m]) ** 2).sum()) + int(((sc[1] - pc[1][m]) ** 2).sum()) for m in range(4)]))
            modes[mby, mbx] = ym, uvm
            stats["uvmodes"].add(uvm)
            if pen < sse16[ym]:  # (else S4 >= 0 cannot win)
                s4, wrk, l4, m4 = i4_trial(sy, rec[0], mbx, mby, steps["y1"])
                is4[mby, mbx] = s4 + pen < sse16[ym]
            if is4[mby, mbx]:
                rec[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = wrk
                levels[mby, mbx, :16] = l4
                bmodes[mby, mbx] = m4
                modes[mby, mbx, 0] = -1
            else:
                stats["ymodes"].add(ym)
                cy = vm.fdct(vm._blocks(sy - py[ym]))
                y2 = vm.fwht(cy[:, 0, 0].reshape(4, 4))
                l2, dq2 = vm.quantise(y2, *steps["y2"])
                dcs = vm.iwht(dq2).reshape(16)
                ly, dqy = vm.quantise(cy, *steps["y1"], with_dc=False)
                dqy[:, 0, 0] = dcs
                rec[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = np.clip(py[ym] + vm._unblocks(vm.idct(dqy)), 0, 255)
                levels[mby, mbx, :16] = ly.reshape(16, 16)[:, zz]
                levels[mby, mbx, 24] = l2.reshape(16)[zz]
            for k in (0, 1):
                cc = vm.fdct(vm._blocks(sc[k] - pc[k][uvm]))
                lc, dqc = vm.quantise(cc, *steps["uv"])
                rec[1 + k][mby * 8:mby * 8 + 8, mbx * 8:mbx * 8 + 8] = np.clip(pc[k][uvm] + vm._unblocks(vm.idct(dqc)), 0, 255)
                levels[mby, mbx, 16 + 4 * k:20 + 4 * k] = lc.reshape(4, 16)[:, zz]
            nz[mby, mbx] = (levels[mby, mbx] != 0).any(axis=1)
    skip = ~nz.any(axis=2)
    stats.update(skipped=int(skip.sum()), i4=is4, bmodes=bmodes, ymode=modes[..., 0].copy(), skip=skip)
    nparts = stats["partitions"]

    # partition 0
    bw = vm.BoolWriter()
    for v_, bits in ((0, 1), (0, 1), (0, 1), (0, 1), (0, 6), (0, 3), (0, 1), ({1: 0, 2: 1, 4: 2, 8: 3}[nparts], 2), (qi, 7),
                     (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        bw.literal(v_, bits)
    for p in vm.UPDATE_PROB:
        bw.put(0, p)
    total = mbw * mbh
    ps = max(1, ((total - stats["skipped"]) * 255 + total // 2) // total)
    bw.literal(1, 1)
    bw.literal(ps, 8)
    top_ctx = [T_DC] * (4 * mbw)          # the modes along the bottom of the row above, as the decoder keeps them
    for mby in range(mbh):
        left_ctx = [T_DC] * 4
        for mbx in range(mbw):
            ym, uvm = int(modes[mby, mbx, 0]), int(modes[mby, mbx, 1])
            bw.put(bool(skip[mby, mbx]), ps)
            if is4[mby, mbx]:
                bw.put(0, vm.YMODE_PROB[0])
                for by in range(4):
                    for bx in range(4):
                        m = RFC_TO_TABLE[int(bmodes[mby, mbx, 4 * by + bx])]
                        pr = BMODE_PROB[top_ctx[4 * mbx + bx]][left_ctx[by]]
                        for node, bit in _TREE[m]:
                            bw.put(bit, pr[node])
                        top_ctx[4 * mbx + bx] = left_ctx[by] = m
            else:
                bw.put(1, vm.YMODE_PROB[0])
                bw.put(ym >= 2, vm.YMODE_PROB[1])
                bw.put(ym & 1, vm.YMODE_PROB[3] if ym >= 2 else vm.YMODE_PROB[2])
                top_ctx[4 * mbx:4 * mbx + 4] = [I16_CONTEXT[ym]] * 4
                left_ctx = [I16_CONTEXT[ym]] * 4
            bw.put(uvm != 0, vm.UVMODE_PROB[0])
            if uvm:
                bw.put(uvm != 1, vm.UVMODE_PROB[1])
                if uvm != 1:
                    bw.put(uvm == 3, vm.UVMODE_PROB[2])
    parts = [bw.finish()]

    # token partitions: the non-zero contexts as the decoder keeps them, nine per column and nine per row (the ninth is Y2's)
    top_nz = np.zeros((mbw, 9), np.int64)
    writers = [vm.BoolWriter() for _ in range(nparts)]
    for mby in range(mbh):
        bw = writers[mby % nparts]
        left_nz = [0] * 9
        for mbx in range(mbw):
            tnz, i4 = top_nz[mbx], bool(is4[mby, mbx])
            if skip[mby, mbx]:
                tnz[:8] = 0
                left_nz[:8] = [0] * 8
                if not i4:
                    tnz[8] = left_nz[8] = 0
                continue
            lev = levels[mby, mbx].tolist()
            if not i4:
                vm.put_block(bw, lev[24], 1, 0, int(tnz[8] + left_nz[8]), stats)
                tnz[8] = left_nz[8] = int(nz[mby, mbx, 24])
            for b in range(16):
                x, yy = b & 3, b >> 2
                vm.put_block(bw, lev[b], 3 if i4 else 0, 0 if i4 else 1, int(tnz[x] + left_nz[yy]), stats)
                tnz[x] = left_nz[yy] = int(nz[mby, mbx, b])
            for b in range(16, 24):
                x = 4 + ((b - 16) >> 2) * 2 + (b & 1)
                yy = 4 + ((b - 16) >> 2) * 2 + ((b >> 1) & 1)
                vm.put_block(bw, lev[b], 2, 0, int(tnz[x] + left_nz[yy]), stats)
                tnz[x] = left_nz[yy] = int(nz[mby, mbx, b])
    parts += [bw.finish() for bw in writers]

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
