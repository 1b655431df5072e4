"""Measurements of the GIF decode front end (profiles/pr_gif_source.txt) on two files: tests/golden/lenna.gif (512 x 512, one frame)
and a synthetic 64-frame 500 x 500 animation Pillow writes (a quantised photograph, a sprite moving over it: every frame behind
the first is a sub-rectangle).
  python tools/gif_source_probe.py host              the host half alone (container + LZW), one thread, beside Pillow decoding every frame of the same file
  python tools/gif_source_probe.py kernels <reps>    flgpu_decode_gif / flgpu_process_gif of the animation: compose kernel time by HIP events, alone and in
                                                     eight contexts side by side, bytes over PCIe, the share of the HBM peak
  python tools/gif_source_probe.py callers <k>       16 caller threads x k requests: flgpu_process_gif, then flgpu_transform_batch fed decoded frames"""
import ctypes as C, io, json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
import gif_model, synth
fl = g._load_package()
HBM_PEAK = 8.0e12   # bytes/s, MI355X

def animation(frames=64, side=500):
    from PIL import Image
    base = Image.fromarray(synth.photo(side, side, 3, index=5)).quantize(255)
    pal = base.getpalette()
    px = np.asarray(base)
    ims = []
    for f in range(frames):
        a = px.copy()
        x, y = 20 + 6 * f, 40 + 5 * f
        a[y:y + 90, x:x + 70] = (np.add.outer(np.arange(90), np.arange(70)) + 3 * f) % 255
        im = Image.fromarray(a, "P"); im.putpalette(pal)
        ims.append(im)
    b = io.BytesIO()
    ims[0].save(b, "GIF", save_all=True, append_images=ims[1:], duration=40, loop=0, optimize=False)
    return b.getvalue()

def pillow_frames(data):
    from PIL import Image, ImageSequence
    return [np.asarray(f.convert("RGBA")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))]

def out(d):
    print(json.dumps(d), flush=True)

FILES = {"lenna": open(os.path.join(ROOT, "tests", "golden", "lenna.gif"), "rb").read(), "animation": animation()}
mode = sys.argv[1]
if mode == "host":
    lib = fl.load_library()
    for name, data in FILES.items():
        info = fl.gif_info(data)
        blob = fl.debug_gif_blob(data)
        assert np.array_equal(gif_model.from_blob(blob)[..., :3], np.stack(pillow_frames(data))[..., :3])
        buf, used, t, z = np.empty(len(blob), np.uint8), C.c_uint64(), [], []
        for _ in range(8):
            a = time.perf_counter(); rc = lib.flgpu_debug_gif_blob(data, len(data), buf.ctypes.data, buf.nbytes, C.byref(used)); t.append(time.perf_counter() - a)
            assert rc == 0 and used.value == len(blob)
        for _ in range(8):
            a = time.perf_counter(); pillow_frames(data); z.append(time.perf_counter() - a)
        out({"what": "host half alone (container walk twice, LZW, palettes; flgpu_debug_gif_blob, which copies the blob once), one thread", "file": name,
             "file_bytes": len(data), "frames": info["frames"], "blob_bytes": len(blob), "decoded_bytes": info["decoded_bytes"],
             "ms_min": 1e3 * min(t), "ms_median": 1e3 * sorted(t)[4], "pillow_all_frames_rgba_ms_min": 1e3 * min(z), "pillow_all_frames_rgba_ms_median": 1e3 * sorted(z)[4]})
elif mode == "kernels":
    reps = int(sys.argv[2])
    data = FILES["animation"]
    info = fl.gif_info(data)
    want = gif_model.from_blob(fl.debug_gif_blob(data))
    def measure(st, label, n_ctx):
        for r in range(reps + 1):   # the first is the warm-up
            st.reset_stats()
            a = time.perf_counter(); got = st.decode_gif(data); dt = time.perf_counter() - a
            st.stats()   # (resolves the HIP events)
            ns = st.debug_get("gif_compose_ns")
            assert np.array_equal(got, want)
            out({"what": label, "contexts": n_ctx, "rep": r, "decode_wall_s": dt, "compose_kernel_us": ns / 1e3, "stored_bytes": info["decoded_bytes"],
                 "stored_bytes_per_s": info["decoded_bytes"] / (ns / 1e9) if ns else None, "share_of_hbm_peak": info["decoded_bytes"] / (ns / 1e9) / HBM_PEAK if ns else None,
                 "upload_bytes": st.debug_get("gif_upload_bytes"), "file_bytes": len(data), "old_path_upload_bytes": info["decoded_bytes"]})
    with fl.State(device=0, profile=True) as st:
        measure(st, "flgpu_decode_gif, 64-frame 500 x 500 animation, one context", 1)
        for r in range(reps + 1):
            st.reset_stats()
            a = time.perf_counter(); res = st.process_gif(data, "w=300&h=200"); dt = time.perf_counter() - a
            s = st.stats()
            out({"what": "flgpu_process_gif w=300&h=200, one context", "rep": r, "wall_s": dt, "compose_kernel_us": st.debug_get("gif_compose_ns") / 1e3, "resample_us": s["resample_ms"] * 1e3})
    states = [fl.State(device=0, profile=True) for _ in range(8)]
    try:
        ts = [threading.Thread(target=measure, args=(s, "flgpu_decode_gif, same animation, eight contexts side by side", 8)) for s in states]
        for t in ts: t.start()
        for t in ts: t.join()
    finally:
        for s in states: s.close()
elif mode == "callers":
    threads, per = 16, int(sys.argv[2])
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
            out(dict({"what": label, "callers": threads, "requests": threads * per, "wall_s": dt, "files_per_s": threads * per / dt, "usable_cpus": len(os.sched_getaffinity(0))}, **extra(st)))
    p = fl.make_params(300, 200, filter=fl.FILTER_NEAREST)
    for rep in range(2):
        for name, data in FILES.items():
            frames = [np.ascontiguousarray(f) for f in pillow_frames(data)]
            run(lambda st: st.process_gif(data, "w=300&h=200"), f"flgpu_process_gif ({name}), w=300&h=200", lambda st: st.gif_counters())
            run(lambda st: st.process_batch(frames, [p] * len(frames)), f"flgpu_transform_batch fed frames decoded beforehand ({name}), same request", lambda st: {})
            run(lambda st: st.process_batch([np.ascontiguousarray(f) for f in pillow_frames(data)], [p] * len(frames)),
                f"Pillow decode + flgpu_transform_batch ({name}), same request", lambda st: {})
