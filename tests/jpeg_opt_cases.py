"""The corpus of FLGPU_FEO_JPEG_OPTIMIZE, shared by tests/test_jpeg_optimize_host.py (CPU) and tests/test_jpeg_optimize.py (GPU): the
smallest pictures at which each part of the option can go wrong.  (name, picture, quality); pictures are built once per process."""
import functools
import heapq

import numpy as np

import synth
import test_jpeg_unit_coder as uc

QUALITIES = (1, 50, 75, 100)
ROW_BLOCKS = (15, 16, 17, 31, 32, 33)     # one row of blocks around the wave (16) and workgroup (32) edges of the statistics and coding grids
FOLD_BX, FOLD_BY, FOLD_Q = 32, 22, 75     # the built picture whose luma AC code would be deeper than 16 bits: 256 x 176


def fold_counts(nblocks):
    """Counts of 17 luma AC symbols -- end-of-block once per block, (run r, size 1) for r = 0..15 -- that with the reserved leaf make
    the minimum-redundancy tree a chain 17 deep: every count exceeds the weight of the node two merges before it."""
    leaves = [1, 1]                         # the reserved leaf, then the rarest symbol
    nodes = [1, 2]                          # nodes[k] = leaves[0] + .. + leaves[k]
    while len(leaves) < 18:
        nxt = max(nodes[-2] + 1, leaves[-1])
        if nxt <= nblocks < nodes[-1] + 1:
            nxt = nblocks                   # the end-of-block count takes its place in the chain: the last step it is large enough for
        leaves.append(nxt)
        nodes.append(nodes[-1] + nxt)
    return leaves[1:]


def fold_units(bx=FOLD_BX, by=FOLD_BY):
    """{block: {0: {zig-zag position: +-1}}}: the luma units of the built picture, every block with an end-of-block code."""
    n = bx * by
    want = fold_counts(n)
    assert n in want, want
    rest = sorted((c for c in want if c != n), reverse=True)             # the most frequent symbol gets the shortest run
    heap = [(0, b) for b in range(n)]
    heapq.heapify(heap)
    runs = [[] for _ in range(n)]
    for r in range(15, -1, -1):                                          # long runs first, each to the emptiest block
        for _ in range(rest[r]):
            used, b = heapq.heappop(heap)
            assert used + r + 1 <= 62
            runs[b].append(r)
            heapq.heappush(heap, (used + r + 1, b))
    units = {}
    for b in range(n):
        pos, coefs = 0, {}
        for k, r in enumerate(runs[b]):
            pos += r + 1
            coefs[pos] = 1 if (k + b) % 2 else -1
        if coefs:
            units[b] = {0: coefs}
    return units


def _fold(oracle):
    units = fold_units()
    return uc._tile({b: uc._block(oracle, FOLD_Q, c.get(0)) for b, c in units.items()}, FOLD_BX, FOLD_BY)


@functools.lru_cache(maxsize=None)
def _corpus(oracle):
    out = [("photo_1x1_c3_q75", synth.photo(1, 1, 3, index=1), 75), ("photo_8x8_c1_q50", synth.photo(8, 8, 1, index=2), 50),
           ("photo_9x7_c4_q1", synth.photo(7, 9, 4, index=3), 1), ("photo_9x7_c3_q100", synth.photo(7, 9, 3, index=4), 100),
           ("photo_83x61_c4_q75", synth.photo(61, 83, 4, index=5), 75)]
    for k, nb in enumerate(ROW_BLOCKS):
        q = QUALITIES[k % 4]
        out.append((f"row_{nb}_blocks_q{q}", synth.photo(8, 8 * nb, 3, index=10 + nb), q))
    flat = np.empty((16, 24, 3), np.uint8)
    flat[:] = (90, 140, 200)
    out.append(("flat_24x16_q75", flat, 75))
    for name, q, units in uc._patterns():
        out.append((name, uc._build(oracle, name, q, units), q))
    out.append(("busy_lanes", *uc._busy_lanes(oracle)))
    out.append(("dc_only", *uc._dc_only(oracle)))
    out.append(("photo_300x200_q100", synth.photo(200, 300, 3, index=7), 100))
    out.append(("fold_256x176_q75", _fold(oracle), FOLD_Q))
    return tuple(out)


def corpus(oracle):
    return _corpus(oracle)


NAMES = (["photo_1x1_c3_q75", "photo_8x8_c1_q50", "photo_9x7_c4_q1", "photo_9x7_c3_q100", "photo_83x61_c4_q75"]
         + [f"row_{nb}_blocks_q{QUALITIES[k % 4]}" for k, nb in enumerate(ROW_BLOCKS)]
         + ["flat_24x16_q75", "zrl_eob_c0", "zrl_eob_c1", "zrl_eob_c2", "all_ac", "busy_lanes", "dc_only", "photo_300x200_q100", "fold_256x176_q75"])


def get(oracle, name):
    for n, img, q in corpus(oracle):
        if n == name:
            return img, q
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def model(oracle, name, fallback=False):
    """(file, info) of the model for a corpus case, computed once"""
    import jpeg_opt_model as jm
    img, q = get(oracle, name)
    return jm.encode(oracle, img, q, fallback)
