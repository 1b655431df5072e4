"""The adaptive-probability variants of the lossy WebP encoder (FLGPU_FE_WEBP_LOSSY_AP, FLGPU_FE_WEBP_LOSSY_I4_AP,
csrc/fl_vp8_ap_core.h) restated in numpy on top of tests/vp8_model.py and tests/vp8_i4_model.py.  Test infrastructure only.

The arithmetic -- predictions, transforms, quantiser, the I4 trial, the boolean coder -- is imported from those two models.  What is
restated here is the macroblock loop (`analyse`, which leaves levels, modes and the reconstruction: the picture before any
entropy coding) and the partition writers with a probability table as an argument (`write`).  With updates forced off, `encode`
returns exactly vp8_model.encode's / vp8_i4_model.encode's bytes (tests/test_webp_lossy_probs_host.py pins that), so this
restatement cannot have drifted from theirs.

The rule, integer only:
  * counts: for every coded macroblock, every boolean of the token walk whose probability is an entry of the table
    [type 4][band 8][ctx 3][node 11] adds to that entry's zeros z or ones o -- with the coder's contexts (a B_PRED macroblock has
    no Y2 block, passes the Y2 context on untouched, and its luma blocks are type 3 from coefficient 0); sign bits, extra bits
    and partition 0 are not counted;
  * candidate: 255 if o == 0, else clamp((255 z + (z + o) // 2) // (z + o), 1, 255);
  * entry i is updated iff z + o > 0, p_new != p_old and, with u = UPDATE_PROB[i] and C = BIT_COST,
        z C[p_new] + o C[256 - p_new] + C[256 - u] + 8 * 256 < z C[p_old] + o C[256 - p_old] + C[u];
  * partition 0 writes every flag with its update probability, an updated one followed by the 8-bit p_new; the token partitions
    are coded with the picture's table.
BIT_COST is read from csrc/fl_vp8_tables.h like the other tables; the test compares it with its formula."""
import numpy as np

import vp8_i4_model as m4
import vp8_model as vm

BIT_COST = vm._T["kVp8BitCost"]
assert len(BIT_COST) == 256
N = 4 * 8 * 3 * 11
DEFAULT = [p for t in vm.COEF_PROB for b in t for c in b for p in c]
assert len(DEFAULT) == N
PART0_BOOLS = 29 + 1056 * 9 + 9 + 32
I4_MAX_MBS = (((1 << 19) - 1) * 8 // 7 - PART0_BOOLS) // m4.PART0_MB_BOOLS
MAX_MBS = (((1 << 19) - 1) * 8 // 7 - PART0_BOOLS) // 7


def max_out_bytes(w, h, i4=False):
    """The non-adaptive front end's, with 9574 booleans in partition 0's fixed part instead of 1126."""
    mbs = ((w + 15) // 16) * ((h + 15) // 16)
    per_mb = m4.PART0_MB_BOOLS if i4 else 7
    base = m4.max_out_bytes(w, h) if i4 else vm.max_out_bytes(w, h)
    return base - (7 * (1126 + per_mb * mbs) + 7) // 8 + (7 * (PART0_BOOLS + per_mb * mbs) + 7) // 8


def fits(w, h, i4=False):
    return vm.fits(w, h) and ((w + 15) // 16) * ((h + 15) // 16) <= (I4_MAX_MBS if i4 else MAX_MBS)


def candidate(z, o):
    return 255 if o == 0 else min(max((255 * z + (z + o) // 2) // (z + o), 1), 255)


def decide(i, z, o):
    """-> the picture's probability for entry i."""
    p_old, u, p_new = DEFAULT[i], vm.UPDATE_PROB[i], candidate(z, o)
    if z + o == 0 or p_new == p_old:
        return p_old
    new = z * BIT_COST[p_new] + o * BIT_COST[256 - p_new] + BIT_COST[256 - u] + 8 * 256
    old = z * BIT_COST[p_old] + o * BIT_COST[256 - p_old] + BIT_COST[u]
    return p_new if new < old else p_old


# ---- the picture before entropy coding ---------------------------------------------------------------------------------------------

def analyse(y, u, v, quality, i4):
    """The macroblock loop of vp8_model.encode (i4 False) / vp8_i4_model.encode (i4 True) -> dict(w, h, mbw, mbh, qi, levels
    [mbh, mbw, 25, 16], nz [mbh, mbw, 25], modes [mbh, mbw, 2], is4 [mbh, mbw], bmodes [mbh, mbw, 16], skip, rec)."""
    h, w = y.shape
    assert fits(w, h, i4) and u.shape == v.shape == ((h + 1) // 2, (w + 1) // 2)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    qi = vm.QUALITY_TO_INDEX[min(max(int(quality), 1), 100)]
    steps = vm.quant_steps(qi)
    pen = m4.penalty(steps["y1"][1])
    src = [np.pad(p, ((0, n * mbh - p.shape[0]), (0, n * mbw - p.shape[1])), mode="edge").astype(np.int64)
           for p, n in ((y, 16), (u, 8), (v, 8))]
    rec = [np.zeros_like(s, dtype=np.uint8) for s in src]
    zz = np.array(vm.ZIGZAG)
    levels = np.zeros((mbh, mbw, 25, 16), np.int64)
    nz = np.zeros((mbh, mbw, 25), np.int64)
    modes = np.zeros((mbh, mbw, 2), np.int64)
    is4 = np.zeros((mbh, mbw), bool)
    bmodes = np.full((mbh, mbw, 16), -1, np.int64)
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
    return dict(w=w, h=h, mbw=mbw, mbh=mbh, qi=qi, levels=levels, nz=nz, modes=modes, is4=is4, bmodes=bmodes, skip=skip,
                rec=(rec[0][:h, :w].copy(), rec[1][:ch, :cw].copy(), rec[2][:ch, :cw].copy()))


# ---- the token walk with a table ---------------------------------------------------------------------------------------------------

class _TableSink:
    """vm.put_block indexes vm.COEF_PROB[type][band][ctx][node] and calls bw.put(bit, that); this stands in for the table and for
    the writer at once: an entry is an index, and `put` of an index is a node, `put` of anything else (128, a category's
    probability) is not.  Indices are offset so that they cannot be mistaken for probabilities."""
    BASE = 1000

    def __init__(self):
        self.table = np.arange(self.BASE, self.BASE + N).reshape(4, 8, 3, 11).tolist()


class _Counter(_TableSink):
    def __init__(self):
        super().__init__()
        self.z, self.o = [0] * N, [0] * N

    def put(self, bit, prob):
        if prob >= self.BASE:
            (self.o if bit else self.z)[prob - self.BASE] += 1


class _Coder(_TableSink):
    def __init__(self, probs):
        super().__init__()
        self.probs, self.bw = probs, vm.BoolWriter()

    def put(self, bit, prob):
        self.bw.put(bit, self.probs[prob - self.BASE] if prob >= self.BASE else prob)


def _walk(an, sinks):
    """The token partitions' macroblock walk of vp8_i4_model.encode (which is vp8_model.encode's where no macroblock is B_PRED):
    macroblock row r goes to sinks[r % len(sinks)]."""
    mbw, mbh, nz, levels, is4, skip = an["mbw"], an["mbh"], an["nz"], an["levels"], an["is4"], an["skip"]
    stats = dict(cat6=False)
    top_nz = np.zeros((mbw, 9), np.int64)
    saved = vm.COEF_PROB
    try:
        for mby in range(mbh):
            bw = sinks[mby % len(sinks)]
            vm.COEF_PROB = bw.table          # vm.put_block reads its probabilities through this name
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
    finally:
        vm.COEF_PROB = saved
    return stats


def count(an):
    """-> (z[1056], o[1056]) of the picture."""
    c = _Counter()
    _walk(an, [c])
    return c.z, c.o


def write(an, probs, a=None):
    """The file of the analysed picture coded with `probs` (1056 entries; an entry that differs from DEFAULT is an update)."""
    w, h, mbw, mbh, qi, modes, is4, bmodes, skip = (an[k] for k in ("w", "h", "mbw", "mbh", "qi", "modes", "is4", "bmodes", "skip"))
    nparts = vm.partitions(mbh)
    bw = vm.BoolWriter()
    for v_, bits in ((0, 1), (0, 1), (0, 1), (0, 1), (0, 6), (0, 3), (0, 1), ({1: 0, 2: 1, 4: 2, 8: 3}[nparts], 2), (qi, 7),
                     (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        bw.literal(v_, bits)
    for i in range(N):
        bw.put(probs[i] != DEFAULT[i], vm.UPDATE_PROB[i])
        if probs[i] != DEFAULT[i]:
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
    coders = [_Coder(probs) for _ in range(nparts)]
    _walk(an, coders)
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


def encode_analysed(an, a=None, adapt=True):
    """-> (file bytes, (reconstructed y, u, v), stats); stats: the analysis plus z, o (the counts), probs (the picture's table) and
    updated (the indices of the updated entries).  adapt=False: the default table, no update -- the non-adaptive front end's file."""
    z, o = count(an)
    probs = [decide(i, z[i], o[i]) for i in range(N)] if adapt else list(DEFAULT)
    stats = dict(an, z=z, o=o, probs=probs, updated=[i for i in range(N) if probs[i] != DEFAULT[i]])
    return write(an, probs, a), an["rec"], stats


def encode(y, u, v, quality, a=None, i4=False, adapt=True):
    return encode_analysed(analyse(y, u, v, quality, i4), a, adapt)
