"""The loop-filtered variants of the lossy WebP encoder (FLGPU_FE_WEBP_LOSSY_LF, _I4_LF, _AP_LF, _I4_AP_LF, csrc/fl_vp8_lf_core.h)
restated in numpy on top of tests/vp8_ap_model.py.  Test infrastructure only.

The macroblock loop (`analyse`), the counts and the probability rule are vp8_ap_model's.  What is stated here:
  * the format's normal loop filter, written from RFC 6386 section 15 (not from the C++): signed arithmetic on samples minus 128,
    `common_adjust`, the sub-block filter and the macroblock filter, the filter decision `abs(p0 - q0) * 2 + abs(p1 - q1) / 2 <= E`
    and the interior tests.  The lines of one edge are independent, so an edge is filtered in one vectorised step;
  * the rule (integer only): base level L0 from the quantiser index (s = min(y1_ac >> 2, 63), f = s * 300 // 256, 0 if f < 2 else
    min(f, 63)); candidates 0, ceil(L0 / 2), L0, min(63, L0 + ceil(L0 / 2)); each candidate c > 0 filters a copy of the padded
    reconstruction as a decoder will (macroblocks in raster order; left edge, inner vertical edges, top edge, inner horizontal
    edges; inner edges iff the macroblock is B_PRED or has a coefficient left, where a luma DC that the inverse WHT of the
    dequantised Y2 block leaves non-zero counts); D(c) = the squared error against the source over the visible samples of Y, U, V;
    the level written is the candidate with the least D, ties to the lowest level; L0 = 0: nothing is evaluated (D = 0, 0, 0, 0)
    and the file is the twin's;
  * `write`: vp8_ap_model.write with the level in the frame header's 6-bit literal.  With level 0 it returns vp8_ap_model.write's
    bytes (tests/test_webp_lossy_filter_host.py pins that)."""
import numpy as np

import vp8_ap_model as ap
import vp8_i4_model as m4
import vp8_model as vm


def base_level(qi):
    s = min(vm.AC_STEP[qi] >> 2, 63)
    f = s * 300 // 256
    return 0 if f < 2 else min(f, 63)


def candidates(base):
    half = (base + 1) // 2
    return [0, half, base, min(63, base + half)]


def limits(level, sharpness=0):
    """RFC 6386 section 15.2 / 9.6 -> (interior limit, hev threshold of a key frame, macroblock edge limit, sub-block edge limit)."""
    interior = level
    if sharpness:
        interior >>= 2 if sharpness > 4 else 1
        interior = min(interior, 9 - sharpness)
    interior = max(interior, 1)
    hev = 2 if level >= 40 else 1 if level >= 15 else 0
    return interior, hev, ((level + 2) * 2) + interior, (level * 2) + interior


# ---- section 15: the filters, on int64 arrays [8, lines]: P3 P2 P1 P0 | Q0 Q1 Q2 Q3 ------------------------------------------------

def _c(v):
    return np.clip(v, -128, 127)


def _common_adjust(use_outer_taps, p1, p0, q0, q1):
    """-> (new p0, new q0, a), all in the signed domain."""
    a = _c(np.where(use_outer_taps, _c(p1 - q1), 0) + 3 * (q0 - p0))
    b = _c(a + 3) >> 3
    a = _c(a + 4) >> 3
    return _c(p0 + b), _c(q0 - a), a


def _filter_lines(px, mb_edge, interior, hev_t, edge_limit):
    """px: uint8 samples [8, n] across an edge -> the filtered ones."""
    s = px.astype(np.int64) - 128                         # u2s
    p3, p2, p1, p0, q0, q1, q2, q3 = s
    yes = ((np.abs(p0 - q0) * 2 + (np.abs(p1 - q1) >> 1)) <= edge_limit)
    for a_, b_ in ((p3, p2), (p2, p1), (p1, p0), (q3, q2), (q2, q1), (q1, q0)):
        yes &= np.abs(a_ - b_) <= interior
    hev = (np.abs(p1 - p0) > hev_t) | (np.abs(q1 - q0) > hev_t)
    out = s.copy()
    if mb_edge:
        # high edge variance: common_adjust with the outer taps; else the three-tap macroblock filter
        hp0, hq0, _ = _common_adjust(True, p1, p0, q0, q1)
        w = _c(_c(p1 - q1) + 3 * (q0 - p0))
        a1, a2, a3 = _c((27 * w + 63) >> 7), _c((18 * w + 63) >> 7), _c((9 * w + 63) >> 7)
        new = [p3, _c(p2 + a3), _c(p1 + a2), _c(p0 + a1), _c(q0 - a1), _c(q1 - a2), _c(q2 - a3), q3]
        hv = [p3, p2, p1, hp0, hq0, q1, q2, q3]
    else:
        np0, nq0, a = _common_adjust(hev, p1, p0, q0, q1)
        a = (a + 1) >> 1
        new = [p3, p2, _c(p1 + a), np0, nq0, _c(q1 - a), q2, q3]
        hv = [p3, p2, p1, np0, nq0, q1, q2, q3]
    for k in range(8):
        out[k] = np.where(yes, np.where(hev, hv[k], new[k]), s[k])
    return (out + 128).astype(np.uint8)                   # s2u


def inner_edges(an):
    """[mbh, mbw] bool: does a decoder filter the macroblock's inner edges?"""
    steps = vm.quant_steps(an["qi"])["y2"]
    zz = np.array(vm.ZIGZAG)
    mbh, mbw = an["mbh"], an["mbw"]
    out = np.zeros((mbh, mbw), bool)
    y2_only = np.zeros((mbh, mbw), bool)
    for mby in range(mbh):
        for mbx in range(mbw):
            if an["is4"][mby, mbx] or an["nz"][mby, mbx, :24].any():
                out[mby, mbx] = True
            elif an["nz"][mby, mbx, 24]:
                lev = an["levels"][mby, mbx, 24]
                dq = np.zeros(16, np.int64)
                dq[zz] = lev * np.array([steps[0]] + [steps[1]] * 15)
                out[mby, mbx] = bool(vm.iwht(dq.reshape(4, 4)).any())
                y2_only[mby, mbx] = not out[mby, mbx]
    return out, y2_only


def loop_filter(planes, level, inner):
    """The padded planes (Y 16 mbw x 16 mbh, U, V 8 mbw x 8 mbh) filtered at `level` (> 0), as new arrays."""
    interior, hev_t, mbe, sbe = limits(level)
    out = [p.copy() for p in planes]
    mbh, mbw = inner.shape
    for mby in range(mbh):
        for mbx in range(mbw):
            for vertical in (True, False):               # the edge is vertical: lines run across it horizontally
                for k, p in enumerate(out):
                    n = 16 if k == 0 else 8
                    x0, y0 = mbx * n, mby * n
                    for e in range(0, n, 4):
                        if e == 0 and (mbx == 0 if vertical else mby == 0):
                            continue
                        if e and not inner[mby, mbx]:
                            continue
                        if vertical:
                            px = p[y0:y0 + n, x0 + e - 4:x0 + e + 4].T
                            p[y0:y0 + n, x0 + e - 4:x0 + e + 4] = _filter_lines(px, e == 0, interior, hev_t, mbe if e == 0 else sbe).T
                        else:
                            px = p[y0 + e - 4:y0 + e + 4, x0:x0 + n]
                            p[y0 + e - 4:y0 + e + 4, x0:x0 + n] = _filter_lines(px, e == 0, interior, hev_t, mbe if e == 0 else sbe)
    return out


# ---- the picture ---------------------------------------------------------------------------------------------------------------------

def analyse(y, u, v, quality, i4):
    """vp8_ap_model.analyse, with the reconstruction padded to whole macroblocks as well (`rec_padded`): the same analysis run on
    the planes padded the way it pads them itself."""
    h, w = y.shape
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    assert ap.fits(w, h, i4)
    pad = [np.pad(p, ((0, n * mbh - p.shape[0]), (0, n * mbw - p.shape[1])), mode="edge") for p, n in ((y, 16), (u, 8), (v, 8))]
    an = ap.analyse(pad[0], pad[1], pad[2], quality, i4)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rp = an["rec"]
    an.update(w=w, h=h, rec_padded=rp, rec=(rp[0][:h, :w].copy(), rp[1][:ch, :cw].copy(), rp[2][:ch, :cw].copy()))
    return an


def sse(planes, y, u, v):
    """Squared error of padded planes against the source over the visible samples."""
    return sum(int(((p[:s.shape[0], :s.shape[1]].astype(np.int64) - s.astype(np.int64)) ** 2).sum()) for p, s in zip(planes, (y, u, v)))


def choose(levels, D):
    best = 0
    for k in range(1, 4):
        if D[k] < D[best]:
            best = k
    return levels[best]


def write(an, probs, level, a=None):
    """vp8_ap_model.write with the loop filter level."""
    w, h, mbw, mbh, qi, modes, is4, bmodes, skip = (an[k] for k in ("w", "h", "mbw", "mbh", "qi", "modes", "is4", "bmodes", "skip"))
    nparts = vm.partitions(mbh)
    bw = vm.BoolWriter()
    # colour space, clamping, no segments; filter type 0 (normal), the level, sharpness 0, no deltas; partitions; quantiser, no deltas;
    # refresh_entropy_probs 0
    for v_, bits in ((0, 1), (0, 1), (0, 1), (0, 1), (level, 6), (0, 3), (0, 1), ({1: 0, 2: 1, 4: 2, 8: 3}[nparts], 2), (qi, 7),
                     (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        bw.literal(v_, bits)
    for i in range(ap.N):
        bw.put(probs[i] != ap.DEFAULT[i], vm.UPDATE_PROB[i])
        if probs[i] != ap.DEFAULT[i]:
            bw.literal(probs[i], 8)
    total = mbw * mbh
    ps = max(1, ((total - int(skip.sum())) * 255 + total // 2) // total)
    bw.literal(1, 1)
    bw.literal(ps, 8)
    top_ctx = [m4.T_DC] * (4 * mbw)
    for mby in range(mbh):
        left_ctx = [m4.T_DC] * 4
        for mbx in range(mbw):
            ym, uvm = int(modes[mby, mbx, 0]), int(modes[mby, mbx, 1])
            bw.put(bool(skip[mby, mbx]), ps)
            if is4[mby, mbx]:
                bw.put(0, vm.YMODE_PROB[0])
                for by in range(4):
                    for bx in range(4):
                        m = m4.RFC_TO_TABLE[int(bmodes[mby, mbx, 4 * by + bx])]
                        pr = m4.BMODE_PROB[top_ctx[4 * mbx + bx]][left_ctx[by]]
                        for node, bit in m4._TREE[m]:
                            bw.put(bit, pr[node])
                        top_ctx[4 * mbx + bx] = left_ctx[by] = m
            else:
                bw.put(1, vm.YMODE_PROB[0])
                bw.put(ym >= 2, vm.YMODE_PROB[1])
                bw.put(ym & 1, vm.YMODE_PROB[3] if ym >= 2 else vm.YMODE_PROB[2])
                top_ctx[4 * mbx:4 * mbx + 4] = [m4.I16_CONTEXT[ym]] * 4
                left_ctx = [m4.I16_CONTEXT[ym]] * 4
            bw.put(uvm != 0, vm.UVMODE_PROB[0])
            if uvm:
                bw.put(uvm != 1, vm.UVMODE_PROB[1])
                if uvm != 1:
                    bw.put(uvm == 3, vm.UVMODE_PROB[2])
    parts = [bw.finish()]
    coders = [ap._Coder(probs) for _ in range(nparts)]
    ap._walk(an, coders)
    parts += [c.bw.finish() for c in coders]

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
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def evaluate(an, y, u, v, base=None):
    """The rule on an analysed picture -> dict(base, levels, D, chosen, inner, y2_only (macroblocks coded with Y2 levels alone whose
    sixteen DCs are 0), filtered (level -> padded planes))."""
    base = base_level(an["qi"]) if base is None else int(base)
    levels = candidates(base)
    inner, y2_only = inner_edges(an)
    filtered = {0: an["rec_padded"]}
    if base == 0:
        return dict(base=0, levels=levels, D=[0, 0, 0, 0], chosen=0, inner=inner, y2_only=y2_only, filtered=filtered)
    for c in levels:
        if c not in filtered:
            filtered[c] = loop_filter(an["rec_padded"], c, inner)
    D = [sse(filtered[c], y, u, v) for c in levels]
    return dict(base=base, levels=levels, D=D, chosen=choose(levels, D), inner=inner, y2_only=y2_only, filtered=filtered)


def encode_analysed(an, y, u, v, a=None, adapt=True, base=None, ev=None):
    """-> (file, unfiltered reconstruction, filtered reconstruction, stats); both reconstructions cut to the picture.  ev: what
    evaluate(an, y, u, v, base) returned, if the caller has it already."""
    h, w = y.shape
    z, o = ap.count(an)
    probs = [ap.decide(i, z[i], o[i]) for i in range(ap.N)] if adapt else list(ap.DEFAULT)
    ev = evaluate(an, y, u, v, base) if ev is None else ev
    f = ev["filtered"][ev["chosen"]]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    shown = (f[0][:h, :w].copy(), f[1][:ch, :cw].copy(), f[2][:ch, :cw].copy())
    stats = dict(an, probs=probs, base=ev["base"], levels=ev["levels"], D=ev["D"], chosen=ev["chosen"], inner=ev["inner"], y2_only=ev["y2_only"])
    return write(an, probs, ev["chosen"], a), an["rec"], shown, stats


def encode(y, u, v, quality, a=None, i4=False, adapt=True, base=None):
    return encode_analysed(analyse(y, u, v, quality, i4), y, u, v, a, adapt, base)
