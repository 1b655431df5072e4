"""Segment-adaptive quantisers of the lossy WebP encoder (FLGPU_FEO_SEGMENTS, csrc/fl_vp8_seg_core.h) restated in numpy on top of
tests/vp8_model.py, vp8_i4_model.py, vp8_ap_model.py and vp8_lf_model.py (by import only).  Test infrastructure only.

The arithmetic -- predictions, transforms, quantiser, the I4 trial, the boolean coder, the token walk, the probability rule, the
loop filter and its choice -- is imported.  What is stated here:
  * the rule (`rule`), integer only, from the luma plane padded to whole macroblocks by edge replication and the base index qi:
      1. activity of a macroblock: act = sum |Y - m| over its 256 samples, m = (sum Y + 128) >> 8;
      2. bin = min(255, act >> 5);
      3. bin 0 is flat: out of steps 4-6, class 0.  No non-flat macroblock, or one occupied bin among them: no segmentation;
      4. histogram over bins 1..255, lo / hi the least / greatest occupied bin, centres c_k = lo + (2 k + 1)(hi - lo) // 8;
      5. six rounds: each bin of [lo, hi] to the class of least |a - c_k| (ties: lowest k), c_k = (sum a hist[a] + n_k // 2) // n_k
         where n_k > 0; then one more assignment;
      6. mid = (sum c_k n_k + N // 2) // N; amp = max(1, 3 qi >> 3); off_k = (c_k - mid) amp / 96 towards zero, clamped to +-amp;
         qi_k = clamp(qi + off_k, 0, 127);
      7. classes with a macroblock are used (flat ones count in class 0); every used class at qi: no segmentation;
      8. tree probabilities from the counts (left, right) = (n0 + n1, n2 + n3), (n0, n1), (n2, n3): 255 if right == 0, else
         clamp((255 left + (l + r) // 2) // (l + r), 1, 255);
  * `analyse`: vp8_ap_model.analyse's macroblock loop with each macroblock's steps and B_PRED penalty taken from its class (on planes
    padded as vp8_lf_model.analyse pads them, so the padded reconstruction is there for the loop filter);
  * `inner_edges` / `evaluate`: vp8_lf_model's with the Y2 steps of each macroblock's class (a decoder dequantises with those);
  * `write`: vp8_lf_model.write with the segment header behind the clamping bit (segmentation_enabled 1, update map 1, update data
    1, absolute mode 1, four quantisers as flag 1 + 7 bits + sign 0, four filter strengths as flag 0 at level 0 else flag 1 + the
    frame's level in 6 bits + sign 0, three probabilities as flag 0 for 255 else flag 1 + 8 bits) and each macroblock's id in front
    of its skip flag: put(s >= 2, p0), put(s & 1, p2 if s >= 2 else p1).
With segmentation off, `analyse` and `write` give vp8_lf_model's (and so vp8_ap_model's, vp8_i4_model's and vp8_model's) bytes;
tests/test_webp_lossy_segments_host.py pins that."""
import numpy as np

import vp8_ap_model as ap
import vp8_i4_model as m4
import vp8_lf_model as lf
import vp8_model as vm

BIN_SHIFT, AMP_NUM, SPAN, ROUNDS = 5, 3, 96, 6
PART0_SEG_BOOLS = 3 + 4 * 9 + 4 * 8 + 3 * 9
PART0_MB_SEG_BOOLS = 2


def _part0(fixed, per_mb, mbs):
    return (7 * (fixed + per_mb * mbs) + 7) // 8


def max_mbs(i4, adapt):
    fixed = (ap.PART0_BOOLS if adapt else 1126) + PART0_SEG_BOOLS
    return (((1 << 19) - 1) * 8 // 7 - fixed) // ((m4.PART0_MB_BOOLS if i4 else 7) + PART0_MB_SEG_BOOLS)


def fits(w, h, i4=False, adapt=False):
    return vm.fits(w, h) and ((w + 15) // 16) * ((h + 15) // 16) <= max_mbs(i4, adapt)


def max_out_bytes(w, h, i4=False, adapt=False):
    """The front end's, with 98 more booleans in partition 0's fixed part and 2 more per macroblock."""
    mbs = ((w + 15) // 16) * ((h + 15) // 16)
    fixed, per_mb = (ap.PART0_BOOLS if adapt else 1126), (m4.PART0_MB_BOOLS if i4 else 7)
    return vm.max_out_bytes(w, h) - _part0(1126, 7, mbs) + _part0(fixed + PART0_SEG_BOOLS, per_mb + PART0_MB_SEG_BOOLS, mbs)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------

def activity(y):
    """[mbh, mbw] act of the luma plane (any size: padded here by edge replication)."""
    h, w = y.shape
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    p = np.pad(y, ((0, 16 * mbh - h), (0, 16 * mbw - w)), mode="edge").astype(np.int64)
    b = p.reshape(mbh, 16, mbw, 16).transpose(0, 2, 1, 3).reshape(mbh, mbw, 256)
    m = (b.sum(axis=2) + 128) >> 8
    return np.abs(b - m[..., None]).sum(axis=2)


def tree_prob(left, right):
    return 255 if right == 0 else min(max((255 * left + (left + right) // 2) // (left + right), 1), 255)


def _trunc_div(a, b):
    q = abs(a) // b
    return -q if a < 0 else q


def rule(y, qi):
    """-> dict(on, qi [4], prob [3], map [mbh, mbw] (class of every macroblock), bins [mbh, mbw], counts [4] (flat ones in class 0),
    centres [4])."""
    act = activity(y)
    bins = np.minimum(255, act >> BIN_SHIFT)
    off = dict(on=False, qi=[qi] * 4, prob=[255] * 3, map=np.zeros(bins.shape, np.int64), bins=bins, counts=[bins.size, 0, 0, 0], centres=[0] * 4)
    hist = np.bincount(bins.reshape(-1), minlength=256).tolist()
    occupied = [a for a in range(1, 256) if hist[a]]
    if len(occupied) < 2:
        return off
    lo, hi = occupied[0], occupied[-1]
    c = [lo + ((2 * k + 1) * (hi - lo)) // 8 for k in range(4)]
    cls, n = {}, [0] * 4
    for rnd in range(ROUNDS + 1):
        n, s = [0] * 4, [0] * 4
        for a in range(lo, hi + 1):
            k = min(range(4), key=lambda j: (abs(a - c[j]), j))
            cls[a] = k
            n[k] += hist[a]
            s[k] += a * hist[a]
        if rnd < ROUNDS:
            c = [(s[k] + n[k] // 2) // n[k] if n[k] else c[k] for k in range(4)]
    N = sum(n)
    mid = (sum(c[k] * n[k] for k in range(4)) + N // 2) // N
    amp = max(1, (AMP_NUM * qi) >> 3)
    qis = [min(max(qi + min(max(_trunc_div((c[k] - mid) * amp, SPAN), -amp), amp), 0), 127) for k in range(4)]
    counts = [n[0] + hist[0], n[1], n[2], n[3]]
    if all(qis[k] == qi for k in range(4) if counts[k]):
        return off
    cls[0] = 0
    seg_map = np.vectorize(lambda a: cls[int(a)])(bins).astype(np.int64)
    prob = [tree_prob(counts[0] + counts[1], counts[2] + counts[3]), tree_prob(counts[0], counts[1]), tree_prob(counts[2], counts[3])]
    return dict(on=True, qi=qis, prob=prob, map=seg_map, bins=bins, counts=counts, centres=c)


# ---- the picture before entropy coding ---------------------------------------------------------------------------------------------

def analyse(y, u, v, quality, i4, segments=True, adapt=False):
    """vp8_lf_model.analyse with per-macroblock steps -> its dict plus seg (what `rule` returned; on False without `segments`) and
    mbqi [mbh, mbw], the index each macroblock was coded at."""
    h, w = y.shape
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    assert fits(w, h, i4, adapt) if segments else ap.fits(w, h, i4)
    qi = vm.QUALITY_TO_INDEX[min(max(int(quality), 1), 100)]
    seg = rule(y, qi) if segments else dict(on=False, qi=[qi] * 4, prob=[255] * 3, map=np.zeros((mbh, mbw), np.int64), counts=[mbw * mbh, 0, 0, 0])
    src = [np.pad(p, ((0, n * mbh - p.shape[0]), (0, n * mbw - p.shape[1])), mode="edge").astype(np.int64) for p, n in ((y, 16), (u, 8), (v, 8))]
    rec = [np.zeros_like(s, dtype=np.uint8) for s in src]
    zz = np.array(vm.ZIGZAG)
    levels = np.zeros((mbh, mbw, 25, 16), np.int64)
    nz = np.zeros((mbh, mbw, 25), np.int64)
    modes = np.zeros((mbh, mbw, 2), np.int64)
    is4 = np.zeros((mbh, mbw), bool)
    bmodes = np.full((mbh, mbw, 16), -1, np.int64)
    mbqi = np.zeros((mbh, mbw), np.int64)
    for mby in range(mbh):
        for mbx in range(mbw):
            mbqi[mby, mbx] = seg["qi"][int(seg["map"][mby, mbx])]
            steps = vm.quant_steps(int(mbqi[mby, mbx]))
            pen = m4.penalty(steps["y1"][1])
            sy = src[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16]
            py = vm.predictions(rec[0], mbx, mby, 16)
            sse16 = [int(((sy - p) ** 2).sum()) for p in py]
            ym = int(np.argmin(sse16))
            pc = [vm.predictions(rec[k], mbx, mby, 8) for k in (1, 2)]
            sc = [src[k][mby * 8:mby * 8 + 8, mbx * 8:mbx * 8 + 8] for k in (1, 2)]
            uvm = int(np.argmin([int(((sc[0] - pc[0][m]) ** 2).sum()) + int(((sc[1] - pc[1][m]) ** 2).sum()) for m in range(4)]))
            modes[mby, mbx] = ym, uvm
            if i4 and pen < sse16[ym]:
                s4, wrk, l4, mo4 = m4.i4_trial(sy, rec[0], mbx, mby, steps["y1"])
                is4[mby, mbx] = s4 + pen < sse16[ym]
            if is4[mby, mbx]:
                rec[0][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = wrk
                levels[mby, mbx, :16] = l4
                bmodes[mby, mbx] = mo4
                modes[mby, mbx, 0] = -1
            else:
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
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return dict(w=w, h=h, mbw=mbw, mbh=mbh, qi=qi, levels=levels, nz=nz, modes=modes, is4=is4, bmodes=bmodes, skip=skip, seg=seg, mbqi=mbqi,
                rec_padded=tuple(rec), rec=(rec[0][:h, :w].copy(), rec[1][:ch, :cw].copy(), rec[2][:ch, :cw].copy()))


def inner_edges(an):
    """vp8_lf_model.inner_edges with the Y2 steps of each macroblock's class."""
    zz = np.array(vm.ZIGZAG)
    mbh, mbw = an["mbh"], an["mbw"]
    out = np.zeros((mbh, mbw), bool)
    for mby in range(mbh):
        for mbx in range(mbw):
            if an["is4"][mby, mbx] or an["nz"][mby, mbx, :24].any():
                out[mby, mbx] = True
            elif an["nz"][mby, mbx, 24]:
                steps = vm.quant_steps(int(an["mbqi"][mby, mbx]))["y2"]
                dq = np.zeros(16, np.int64)
                dq[zz] = an["levels"][mby, mbx, 24] * np.array([steps[0]] + [steps[1]] * 15)
                out[mby, mbx] = bool(vm.iwht(dq.reshape(4, 4)).any())
    return out


def evaluate(an, y, u, v):
    """vp8_lf_model.evaluate: the base level from the picture's base index, the candidates filtered and measured."""
    base = lf.base_level(an["qi"])
    levels = lf.candidates(base)
    inner = inner_edges(an)
    filtered = {0: an["rec_padded"]}
    if base == 0:
        return dict(base=0, levels=levels, D=[0, 0, 0, 0], chosen=0, inner=inner, filtered=filtered)
    for c in levels:
        if c not in filtered:
            filtered[c] = lf.loop_filter(an["rec_padded"], c, inner)
    D = [lf.sse(filtered[c], y, u, v) for c in levels]
    return dict(base=base, levels=levels, D=D, chosen=lf.choose(levels, D), inner=inner, filtered=filtered)


# ---- the file ------------------------------------------------------------------------------------------------------------------------

def write(an, probs, level=0, a=None):
    """The file of the analysed picture: vp8_lf_model.write with the segment header and the ids where an["seg"]["on"]."""
    w, h, mbw, mbh, qi, modes, is4, bmodes, skip, seg = (an[k] for k in ("w", "h", "mbw", "mbh", "qi", "modes", "is4", "bmodes", "skip", "seg"))
    nparts = vm.partitions(mbh)
    bw = vm.BoolWriter()
    bw.literal(0, 1)  # colour space
    bw.literal(0, 1)  # clamping
    bw.literal(int(seg["on"]), 1)
    if seg["on"]:
        for v_ in (1, 1, 1):                 # update the map, update the data, absolute values
            bw.literal(v_, 1)
        for k in range(4):
            bw.literal(1, 1)
            bw.literal(seg["qi"][k], 7)
            bw.literal(0, 1)
        for k in range(4):
            bw.literal(int(level != 0), 1)
            if level:
                bw.literal(level, 6)
                bw.literal(0, 1)
        for k in range(3):
            bw.literal(int(seg["prob"][k] != 255), 1)
            if seg["prob"][k] != 255:
                bw.literal(seg["prob"][k], 8)
    for v_, bits in ((0, 1), (level, 6), (0, 3), (0, 1), ({1: 0, 2: 1, 4: 2, 8: 3}[nparts], 2), (qi, 7),
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
            if seg["on"]:
                s = int(seg["map"][mby, mbx])
                bw.put(s >= 2, seg["prob"][0])
                bw.put(s & 1, seg["prob"][2] if s >= 2 else seg["prob"][1])
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


def encode_analysed(an, y, u, v, a=None, adapt=False, filt=False):
    """-> (file, unfiltered reconstruction, what a decoder shows, stats); both cut to the picture.  filt: a loop-filtered family."""
    h, w = y.shape
    probs = list(ap.DEFAULT)
    if adapt:
        z, o = ap.count(an)
        probs = [ap.decide(i, z[i], o[i]) for i in range(ap.N)]
    stats = dict(an, probs=probs, chosen=0)
    shown = an["rec"]
    if filt:
        ev = evaluate(an, y, u, v)
        f = ev["filtered"][ev["chosen"]]
        cw, ch = (w + 1) // 2, (h + 1) // 2
        shown = (f[0][:h, :w].copy(), f[1][:ch, :cw].copy(), f[2][:ch, :cw].copy())
        stats.update(base=ev["base"], levels=ev["levels"], D=ev["D"], chosen=ev["chosen"], inner=ev["inner"])
    return write(an, probs, stats["chosen"], a), an["rec"], shown, stats


def encode(y, u, v, quality, a=None, i4=False, adapt=False, filt=False, segments=True):
    return encode_analysed(analyse(y, u, v, quality, i4, segments, adapt), y, u, v, a, adapt, filt)
