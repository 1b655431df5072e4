"""Measurements of the PNG decode front end (profiles/pr_png_source.txt) on a 1920x1080 RGB8 photograph written with Paeth on every row, zlib level 6.
  python tools/png_source_probe.py host             the host half alone, one thread
  python tools/png_source_probe.py callers <k>      64 caller threads x k requests: PNG files, then pixel sources, then Pillow on 16 threads
  python tools/png_source_probe.py batch <n> <reps> flgpu_transform_batch of n files (run it under rocprofv3 --kernel-trace --stats for kernel times)
A trailing `device` on batch and callers hands the files over with FLGPU_IMG_PNG_INFLATE: the deflate stream is inflated on the device
(profiles/pr_png_inflate_device.txt).  `host` also times what is left on the calling thread then, and `model` prints the host twin's stats."""
import io, json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
import png_write, synth
fl = g._load_package()

def the_file(index=3):
    img = synth.photo(1080, 1920, 3, index=index)
    return png_write.write_png(img, 2, filters=4, level=6), img

def out(d):
    print(json.dumps(d), flush=True)

mode = sys.argv[1]
device = sys.argv[-1] == "device"
data, img = the_file()
if mode == "host":
    t = []
    for _ in range(8):
        a = time.perf_counter(); fl.debug_png_scanlines(data); t.append(time.perf_counter() - a)
    import zlib
    payload = png_write.idat_payload(data)
    z = []
    for _ in range(8):
        a = time.perf_counter(); zlib.decompress(payload); z.append(time.perf_counter() - a)
    out({"what": "host half alone (container walk with CRCs, inflate, Adler-32), 1920x1080 RGB8 Paeth level 6, one thread", "file_bytes": len(data),
         "scanline_bytes": 1080 * (1 + 5760), "ms_min": 1e3 * min(t), "ms_median": 1e3 * sorted(t)[4], "zlib_inflate_only_ms_min": 1e3 * min(z)})
    # with FLGPU_IMG_PNG_INFLATE the calling thread keeps the container walk with its CRCs (what flgpu_png_info_of does) and one copy of the payload
    w, c = [], []
    for _ in range(8):
        a = time.perf_counter(); fl.png_info(data); w.append(time.perf_counter() - a)
        src = np.frombuffer(payload, np.uint8); dst = np.empty_like(src)
        a = time.perf_counter(); dst[:] = src; c.append(time.perf_counter() - a)
    out({"what": "what stays on the calling thread with the device inflate: container walk with CRCs (flgpu_png_info_of) + one copy of the payload (numpy)",
         "payload_bytes": len(payload), "walk_ms_min": 1e3 * min(w), "copy_ms_min": 1e3 * min(c), "sum_ms_min": 1e3 * (min(w) + min(c))})
elif mode == "model":
    a = time.perf_counter(); scan, stats = fl.debug_png_inflate_model(data); dt = time.perf_counter() - a
    assert scan == fl.debug_png_scanlines(data)
    out({"what": "host twin of the inflate kernel on the same file", "stats": stats, "sync_rounds_per_strip": stats["sync_rounds"] / max(1, stats["strips"]),
         "resolve_rounds_per_strip": stats["resolve_rounds"] / max(1, stats["strips"]), "share_of_tokens_decoded_again": stats["tokens_again"] / max(1, stats["tokens"]), "model_s": dt})
elif mode == "batch":
    n, reps = int(sys.argv[2]), int(sys.argv[3])
    with fl.State(device=0) as st:
        p = fl.make_params(300, 200)
        one = st.process_png_pixels(data, p)
        assert np.array_equal(st.decode_png(data), img)
        src = fl.InflatePng(data) if device else data
        if device:
            assert np.array_equal(st.decode_png(data, device_inflate=True), img)
        for r in range(reps + 1):   # the first is the warm-up
            a = time.perf_counter()
            res = st.process_batch([src] * n, [p] * n)
            dt = time.perf_counter() - a
            assert all(np.array_equal(x, one) for x in res[:: max(1, n // 8)])
            out({"what": "flgpu_transform_batch, " + ("inflate on the device" if device else "host inflate serial on the calling thread"), "n": n, "rep": r, "wall_s": dt})
        out({"counters": dict(st.png_counters(), **({k: st.debug_get(k) for k in ("png_device_inflates", "png_inflate_retries")} if device else {}))})
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
            out(dict({"what": label, "callers": threads, "requests": threads * per, "wall_s": dt, "per_s": threads * per / dt, "usable_cpus": len(os.sched_getaffinity(0)),
                      "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}, **extra(st)))
    p = fl.make_params(300, 200)
    for rep in range(2):
        if device:
            run(lambda st: st.process_png_pixels(data, p, device_inflate=True), "PNG-file sources through flgpu_transform, inflate on the device (w=300&h=200, pixels out)",
                lambda st: dict(st.png_counters(), **{k: st.debug_get(k) for k in ("png_device_inflates", "png_inflate_retries")}))
            continue
        run(lambda st: st.process_png_pixels(data, p), "PNG-file sources through flgpu_transform (w=300&h=200, pixels out)", lambda st: st.png_counters())
        run(lambda st: st.process_pixels(img, p), "pixel sources through flgpu_transform, same request", lambda st: {})
    if device:
        sys.exit(0)
    from PIL import Image
    def pil():
        im = Image.open(io.BytesIO(data)); im.load()
    for rep in range(2):
        ts = [threading.Thread(target=lambda: [pil() for _ in range(8)]) for _ in range(16)]
        a = time.perf_counter()
        for t in ts: t.start()
        for t in ts: t.join()
        dt = time.perf_counter() - a
        out({"what": "Pillow decoding the same file, 16 threads", "files": 128, "wall_s": dt, "per_s": 128 / dt})
