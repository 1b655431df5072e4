"""Lossless WebP probe (FLGPU_FE_WEBP_LOSSLESS): stream sizes against libwebp's own lossless encoder and the device PNG stream,
throughput against FE_NONE.  Prints plain text; under `rocprofv3 --kernel-trace --stats` (a run of its own) the kernel
statistics attribute device time to the eight webpll_* kernels and the resample kernel of the same batches.

    python tools/webp_lossless_probe.py [--batch 1024] [--iters 5] [--sizes-only] [--timing-only]
"""
import argparse
import ctypes as C
import ctypes.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def libwebp_lossless(rgba):
    """WebPEncodeLosslessRGBA (libwebp's defaults for its simple lossless API) -> file bytes, or None without libwebp."""
    name = ctypes.util.find_library("webp") or "libwebp.so.7"
    try:
        lib = C.CDLL(name)
    except OSError:
        return None
    lib.WebPEncodeLosslessRGBA.restype = C.c_size_t
    lib.WebPEncodeLosslessRGBA.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(C.c_uint8))]
    lib.WebPFree.argtypes = [C.c_void_p]
    rgba = np.ascontiguousarray(rgba)
    h, w, _ = rgba.shape
    out = C.POINTER(C.c_uint8)()
    n = lib.WebPEncodeLosslessRGBA(rgba.ctypes.data, w, h, 4 * w, C.byref(out))
    try:
        return C.string_at(out, n) if n else None
    finally:
        if n:
            lib.WebPFree(out)


def sizes(fl, st):
    import synth
    import vp8l_model as vm
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
    print("# file bytes: device lossless WebP | libwebp WebPEncodeLosslessRGBA | device PNG (Default) -- same pixels")
    for name, img, kw in cases:
        px = st.process_pixels(img, fl.make_params(**kw))
        dev = st.process_pixels(img, fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS, **kw))
        ok = np.array_equal(vm.decode_rgba(dev), vm.into_rgba8(px))
        ref = libwebp_lossless(vm.into_rgba8(px))
        png = st.process_pixels(img, fl.make_params(quality=75, front_end=fl.FE_PNG, **kw))
        rl = len(ref) if ref else 0
        print(f"{name}: rgba8 {vm.into_rgba8(px).nbytes} | device {len(dev)} | libwebp {rl} ({len(dev) / max(rl, 1):.3f} x) | "
              f"png {len(png)} ({len(dev) / len(png):.3f} x) | round trip {'ok' if ok else 'FAILED'}")


def timing(fl, st, batch, iters):
    import torch
    import synth
    nsrc = 16
    srcs = [torch.from_numpy(synth.photo(1080, 1920, 3, index=40 + i)).cuda() for i in range(nsrc)]
    shapes = [(1080, 1920, 3)] * batch
    ptrs = [srcs[i % nsrc].data_ptr() for i in range(batch)]
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, fe in (("FE_NONE", fl.FE_NONE), ("FE_WEBP_LOSSLESS", fl.FE_WEBP_LOSSLESS)):
        p = fl.make_params(300, 200, quality=100, front_end=fe)
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
        print(f"{name}: {batch} x 1080p RGB8 -> w=300&h=200&webp=true&quality=100: {dt * 1e3:.2f} ms per batch, {batch / dt:.0f} images/s, "
              f"mean output {np.mean(nbytes):.0f} bytes (raw Rgba8 pixels {300 * 200 * 4})")
    dt_none, _ = out["FE_NONE"]
    dt_w, nb = out["FE_WEBP_LOSSLESS"]
    print(f"encode adds {(dt_w - dt_none) * 1e3:.2f} ms per batch; streams are {np.sum(nb) / (batch * 300 * 200 * 4):.3f} of the raw "
          f"pixel bytes that crossed PCIe before")


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
