"""Measurements of the lossless WebP decode front end (profiles/pr_webp_source.txt) on two 1920x1080 files Pillow wrote with
lossless=True, method=4: a photograph (tests/synth.py photo) and a 16-colour picture.
  python tools/webp_source_probe.py host            the host half alone, one thread, beside libwebp's full decode (WebPDecodeRGBA through ctypes)
  python tools/webp_source_probe.py kernels <reps>  one picture alone and a 64-picture batch: kernel times by HIP events, beside the resample time
  python tools/webp_source_probe.py callers <k>     64 caller threads x k requests through the queue: WebP files, then pixel sources, in the same run"""
import ctypes as C, io, json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
import synth, vp8l_model
fl = g._load_package()

def files():
    from PIL import Image
    photo = synth.photo(1080, 1920, 3, index=3)
    rng = np.random.default_rng(7)
    pal = rng.integers(0, 256, (16, 3)).astype(np.uint8)
    y, x = np.mgrid[0:1080, 0:1920]
    idx = ((x // 24 + y // 16) + (rng.integers(0, 8, (1080, 1920)) == 0) * rng.integers(0, 16, (1080, 1920))) % 16
    out = {}
    for name, img in (("photo", photo), ("palette16", pal[idx])):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "WEBP", lossless=True, method=4)
        out[name] = (b.getvalue(), img)
    return out

def out(d):
    print(json.dumps(d), flush=True)

def counters(st):
    st.stats()   # (resolves the HIP events)
    return {k: st.debug_get(k) for k in ("webp_sources", "webp_file_bytes", "webp_upload_bytes", "webp_predict_ns", "webp_pointwise_ns")}

mode = sys.argv[1]
F = files()
if mode == "host":
    for name, (data, img) in F.items():
        info = fl.webp_info(data)
        t, z = [], []
        blob = fl.debug_webp_residuals(data)
        lib, buf, used = fl.load_library(), np.empty(len(blob), np.uint8), C.c_uint64()
        for _ in range(8):
            a = time.perf_counter(); rc = lib.flgpu_debug_webp_residuals(data, len(data), buf.ctypes.data, buf.nbytes, C.byref(used)); t.append(time.perf_counter() - a)
            assert rc == 0 and buf.tobytes() == blob
        for _ in range(8):
            a = time.perf_counter(); px = vp8l_model.decode_rgba(data); z.append(time.perf_counter() - a)
        assert np.array_equal(px[..., :3], img)
        out({"what": "host half alone (container, header walk for the size, prefix codes, LZ77, colour cache; flgpu_debug_webp_residuals, which copies the blob once), one thread",
             "file": name, "file_bytes": len(data), "blob_bytes": len(blob), "decoded_bytes": img.size, "transforms": info["transforms"],
             "color_cache_bits": info["color_cache_bits"], "prefix_groups": info["prefix_groups"],
             "ms_min": 1e3 * min(t), "ms_median": 1e3 * sorted(t)[4], "libwebp_full_decode_ms_min": 1e3 * min(z), "libwebp_full_decode_ms_median": 1e3 * sorted(z)[4]})
elif mode == "kernels":
    reps = int(sys.argv[2])
    with fl.State(device=0, profile=True) as st:
        p = fl.make_params(300, 200)
        for name, (data, img) in F.items():
            assert np.array_equal(st.decode_webp(data), img)
            one = st.process_webp_pixels(data, p)
            for n in (1, 64):
                for r in range(reps + 1):   # the first is the warm-up
                    st.reset_stats()
                    a = time.perf_counter()
                    res = st.process_batch([data] * n, [p] * n)
                    dt = time.perf_counter() - a
                    s = st.stats()
                    c = counters(st)
                    assert all(np.array_equal(x, one) for x in res[:: max(1, n // 8)])
                    out({"what": "flgpu_transform_batch (entropy decode serial on the calling thread), w=300&h=200", "file": name, "n": n, "rep": r, "wall_s": dt,
                         "predict_kernel_us": c["webp_predict_ns"] / 1e3, "pointwise_kernels_us": c["webp_pointwise_ns"] / 1e3, "resample_us": s["resample_ms"] * 1e3,
                         "upload_bytes_per_file": c["webp_upload_bytes"] // n, "decoded_bytes_per_file": img.size})
elif mode == "callers":
    threads, per = 64, int(sys.argv[2])
    def run(fn, label, extra):
        with fl.State(device=0) as st:
            fn(st)  # warm-up
            def worker():
                for _ in range(per): fn(st)
            ts = [threading.Thread(target=worker) for _ in range(threads)]
            a = time.perf_counter()
            for t in ts: t.start()
            for t in ts: t.join()
            dt = time.perf_counter() - a
            out(dict({"what": label, "callers": threads, "requests": threads * per, "wall_s": dt, "per_s": threads * per / dt, "usable_cpus": len(os.sched_getaffinity(0))}, **extra(st)))
    p = fl.make_params(300, 200)
    for rep in range(2):
        for name, (data, img) in F.items():
            run(lambda st: st.process_webp_pixels(data, p), f"WebP-file sources ({name}) through flgpu_transform (w=300&h=200, pixels out)", lambda st: {"webp_sources": st.debug_get("webp_sources")})
            run(lambda st: st.process_pixels(img, p), f"pixel sources ({name}) through flgpu_transform, same request", lambda st: {})
