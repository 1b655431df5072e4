"""FLGPU_FEO_JPEG_PROGRESSIVE probe: what progressive files cost and save on the flagship batch (N x 1080p -> w=300&h=200, FLGPU_FE_JPEG) and
on a lone 300 x 200 picture.  In interleaved rounds, the three codings -- standard, FLGPU_FEO_JPEG_OPTIMIZE, progressive -- at each
quality: the host's clock around synchronised device batches (ms per batch, images/s), the mean file bytes and the encoder's scratch
bytes per picture.  Prints plain text.

    python tools/jpeg_progressive_probe.py [--batch 1024] [--iters 5] [--rounds 5] [--qualities 75,30]
    python tools/jpeg_progressive_probe.py --timing-only --variant prog [--lone] [--qualities 75]

--timing-only: one variant only (--variant std | opt | prog), 1 + --iters times -- the run to put under
`rocprofv3 --kernel-trace --stats` (--lone: one 300 x 200 picture per batch instead of the flagship batch)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VARIANTS = {"std": dict(), "opt": dict(jpeg_optimize=True), "prog": dict(jpeg_progressive=True)}


def _prepare(fl, st, torch, srcs, shape, batch, p):
    h, w, c = shape
    cap = (int(fl.plan_output(p, w, h, c).max_out_bytes) + 255) // 256 * 256
    dst = torch.empty(batch * cap, dtype=torch.uint8, device="cuda")
    run = st.prepared_batch([srcs[i % len(srcs)].data_ptr() for i in range(batch)], [shape] * batch, p, [dst.data_ptr() + i * cap for i in range(batch)], [cap] * batch)
    run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return run, dst, [r[1] for r in st.batch_results()]


def scratch_bytes(w, h, variant):
    """The encoder's scratch per picture (csrc/fl_encode.cpp jpeg_scratch): 16-byte records, 32-bit bit offsets, the 208-byte slots of the
    codes past a record -- three per block, four for a progressive picture; with FLGPU_FEO_JPEG_OPTIMIZE the picture's record, its DC
    terms and its counts; a progressive picture's record (1,424 words), 14 bytes per block of DC terms and runs, and 4 KB of counts."""
    up = lambda n: (n + 255) // 256 * 256
    blocks = ((w + 7) // 8) * ((h + 7) // 8)
    units = blocks * (4 if variant == "prog" else 3)
    extra = {"std": 0, "opt": up(704 * 4 + units * 2) + 2048, "prog": up(1424 * 4 + blocks * 14) + 4096}[variant]
    return units, up(units * 16) + up((units + 1) * 4) + up(units * 208) + extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--qualities", default="75,30")
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="prog")
    ap.add_argument("--lone", action="store_true")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g
    import synth
    fl = g._load_package()
    qualities = [int(q) for q in a.qualities.split(",")]
    with fl.State(device=0) as st:
        big = [torch.from_numpy(synth.photo(1080, 1920, 3, index=40 + i)).cuda() for i in range(16)]
        small = [torch.from_numpy(st.process_pixels(synth.photo(1080, 1920, 3, index=40), fl.make_params(300, 200))).cuda()]
        stream = torch.cuda.current_stream().cuda_stream
        sets = {"flagship": (big, (1080, 1920, 3), a.batch, dict(w=300, h=200)), "lone 300 x 200": (small, (200, 300, 4), 1, {})}
        if a.timing_only:
            sets = {k: v for k, v in sets.items() if (k != "flagship") == a.lone}
        runs = {}
        for name, (srcs, shape, batch, dims) in sets.items():
            for q in qualities:
                for variant in ((a.variant,) if a.timing_only else VARIANTS):
                    p = fl.make_params(quality=q, front_end=fl.FE_JPEG, **VARIANTS[variant], **dims)
                    runs[(name, q, variant)] = _prepare(fl, st, torch, srcs, shape, batch, p) + (batch,)
        times = {k: [] for k in runs}
        for _ in range(1 if a.timing_only else a.rounds):  # interleaved, so that a drift of the clocks falls on every variant alike
            for k, (run, dst, nbytes, batch) in runs.items():
                iters = a.iters * (200 if batch == 1 else 1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    run(stream)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / iters * 1e3)
        for (name, q, variant), ts in times.items():
            batch, nbytes = runs[(name, q, variant)][3], runs[(name, q, variant)][2]
            med = float(np.median(ts))
            print(f"{name} quality {q} {variant}: {batch} picture(s), ms per batch {' '.join(f'{t:.3f}' for t in ts)} (median {med:.3f}, "
                  f"{batch / med * 1e3:.0f} images/s), mean file {np.mean(nbytes):.0f} bytes")
        for variant in VARIANTS:
            units, nbytes = scratch_bytes(300, 200, variant)
            print(f"scratch per 300 x 200 picture, {variant}: {units} records, {nbytes} bytes")
        print("jpeg_progressive:", st.debug_get("jpeg_progressive"), "jpeg_optimized:", st.debug_get("jpeg_optimized"))


if __name__ == "__main__":
    main()
