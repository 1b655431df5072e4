"""FLGPU_FEO_JPEG_OPTIMIZE probe: what per-picture Huffman tables cost and save on the flagship batch (N x 1080p -> w=300&h=200,
FLGPU_FE_JPEG) and on a lone 300 x 200 picture.  In interleaved rounds, without and with the option at each quality: the host's
clock around synchronised device batches (ms per batch, images/s) and the mean file bytes.  Prints plain text.

    python tools/jpeg_optimize_probe.py [--batch 1024] [--iters 5] [--rounds 5] [--qualities 75,30]
    python tools/jpeg_optimize_probe.py --timing-only [--no-option] [--lone] [--qualities 75]

--timing-only: one variant only, 1 + --iters times -- the run to put under `rocprofv3 --kernel-trace --stats` (--no-option: the batch
without the option; --lone: one 300 x 200 picture per batch instead of the flagship batch)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _prepare(fl, st, torch, srcs, shape, batch, p):
    h, w, c = shape
    cap = (int(fl.plan_output(p, w, h, c).max_out_bytes) + 255) // 256 * 256
    dst = torch.empty(batch * cap, dtype=torch.uint8, device="cuda")
    run = st.prepared_batch([srcs[i % len(srcs)].data_ptr() for i in range(batch)], [shape] * batch, p, [dst.data_ptr() + i * cap for i in range(batch)], [cap] * batch)
    run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return run, dst, [r[1] for r in st.batch_results()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--qualities", default="75,30")
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--no-option", action="store_true")
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
                for opt in ((not a.no_option,) if a.timing_only else (False, True)):
                    p = fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_optimize=opt, **dims)
                    runs[(name, q, opt)] = _prepare(fl, st, torch, srcs, shape, batch, p) + (batch,)
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
        for (name, q, opt), ts in times.items():
            batch, nbytes = runs[(name, q, opt)][3], runs[(name, q, opt)][2]
            med = float(np.median(ts))
            print(f"{name} quality {q} option {int(opt)}: {batch} picture(s), ms per batch {' '.join(f'{t:.3f}' for t in ts)} (median {med:.3f}, "
                  f"{batch / med * 1e3:.0f} images/s), mean file {np.mean(nbytes):.0f} bytes")
        print("jpeg_optimized:", st.debug_get("jpeg_optimized"))


if __name__ == "__main__":
    main()
