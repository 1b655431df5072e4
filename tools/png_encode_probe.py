"""PNG encode probe (FLGPU_FE_PNG): sizes against zlib, throughput against FE_NONE, and a host stand-in for the crate's
encoder.  Prints plain text; under `rocprofv3 --kernel-trace --stats` (a run of its own) the kernel statistics attribute
device time to png_filter_kernel / png_deflate_kernel / png_frame_kernel and the resample kernel of the same batches.

    python tools/png_encode_probe.py [--batch 1024] [--iters 5] [--sizes-only] [--timing-only]
"""
import argparse
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def filtered(px):
    """The filtered rows the device deflates (numpy restatement of the adaptive rule, tests/test_png_encode.py)."""
    from test_png_encode import filter_rows
    return filter_rows(px)[1]


def idat_payload(data):
    from test_png_encode import chunks_of
    return b"".join(b for t, b in chunks_of(data)[1:-1])


def sizes(fl, st):
    import synth
    big = synth.photo(1080, 1920, 3, index=3)
    cases = [
        ("photo 1080p rgb -> w=300&h=200 (rgba8)", big, dict(w=300, h=200)),
        ("photo 1080p rgb -> w=300&h=200 crop", big, dict(w=300, h=200, crop=True)),
        ("photo 1080p rgb -> w=300&h=200 blur=10", big, dict(w=300, h=200, blur_sigma=10.0)),
        ("photo 1080p rgb -> w=300&h=200 crop grayscale (l8)", big, dict(w=300, h=200, crop=True, grayscale=True)),
        ("edges checker 300x200 rgba", synth.edges(200, 300, 4)["checker"], {}),
        ("flat 300x200 rgba", np.full((200, 300, 4), 77, np.uint8), {}),
        ("noise 300x200 rgba", np.random.default_rng(5).integers(0, 256, (200, 300, 4), dtype=np.uint8), {}),
        ("photo 4k rgb (no resize)", synth.photo(2160, 3840, 3, index=12), {}),
    ]
    print("# zlib stream bytes (IDAT payloads): device at Best / Default / Fast against Python zlib -9 / -6 / -1 on the same filtered rows")
    for name, img, kw in cases:
        px = st.process_pixels(img, fl.make_params(**kw))
        raw = filtered(px)
        dev = [len(idat_payload(st.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_PNG, **kw)))) for q in (30, 75, 95)]
        ref = [len(zlib.compress(raw, lv)) for lv in (9, 6, 1)]
        ratio = " ".join(f"{d / r:.3f}" for d, r in zip(dev, ref))
        print(f"{name}: pixels {px.nbytes} filtered {len(raw)} | device {dev[0]} {dev[1]} {dev[2]} | zlib {ref[0]} {ref[1]} {ref[2]} | ratio {ratio}")


def timing(fl, st, batch, iters):
    import torch
    import synth
    nsrc = 16
    srcs = [torch.from_numpy(synth.photo(1080, 1920, 3, index=40 + i)).cuda() for i in range(nsrc)]
    shapes = [(1080, 1920, 3)] * batch
    ptrs = [srcs[i % nsrc].data_ptr() for i in range(batch)]
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, fe in (("FE_NONE", fl.FE_NONE), ("FE_PNG", fl.FE_PNG), ("FE_JPEG", fl.FE_JPEG)):
        p = fl.make_params(300, 200, quality=75, front_end=fe)
        cap = int(fl.plan_output(p, 1920, 1080, 3).max_out_bytes)
        cap = (cap + 255) // 256 * 256
        dst = torch.empty(batch * cap, dtype=torch.uint8, device="cuda")
        run = st.prepared_batch(ptrs, shapes, p, [dst.data_ptr() + i * cap for i in range(batch)], [cap] * batch)
        run(stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            run(stream)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
        res = st.batch_results() if fe != fl.FE_NONE else None
        nbytes = [r[1] for r in res] if res else [300 * 200 * 4] * batch
        out[name] = (dt, nbytes)
        print(f"{name}: {batch} x 1080p RGB8 -> w=300&h=200: {dt * 1e3:.2f} ms per batch, {batch / dt:.0f} images/s, "
              f"mean output {np.mean(nbytes):.0f} bytes (raw Rgba8 pixels {300 * 200 * 4})")
    dt_png, nb = out["FE_PNG"]
    print(f"PNG streams: {np.sum(nb) / (batch * 300 * 200 * 4):.3f} of the raw pixel bytes cross PCIe "
          f"({batch * 300 * 200 * 4 - int(np.sum(nb))} bytes per batch no longer do)")
    # host stand-in for the png crate's encoder: Python zlib level 6 over the same filtered rows, 16 threads (a stand-in,
    # not the crate: no Rust toolchain here)
    px = [st.process_pixels(srcs[i].cpu().numpy(), fl.make_params(300, 200)) for i in range(nsrc)]
    rows = [filtered(x) for x in px]
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda r: zlib.compress(r, 6), rows))
        t0 = time.perf_counter()
        n = 0
        for _ in range(max(1, batch // nsrc)):
            list(ex.map(lambda r: zlib.compress(r, 6), rows))
            n += nsrc
        dt = time.perf_counter() - t0
    print(f"host stand-in (Python zlib -6 on the filtered rows, 16 threads): {n / dt:.0f} images/s ({dt / n * 1e3:.3f} ms per picture)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sizes-only", action="store_true")
    ap.add_argument("--timing-only", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    fl = g._load_package()
    with fl.State(device=0) as st:
        if not a.timing_only:
            sizes(fl, st)
        if not a.sizes_only:
            timing(fl, st, a.batch, a.iters)


if __name__ == "__main__":
    main()
