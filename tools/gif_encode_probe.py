"""Measurements of the GIF encoder (profiles/pr_gif_encode.txt) on the two files of tools/gif_source_probe.py: tests/golden/lenna.gif
with w=300&h=200&crop=true, and the 64-frame 500 x 500 Pillow animation with w=300&h=200.
  python tools/gif_encode_probe.py ratio            (no GPU) file size for segment lengths 1024 / 2048 / 3838 against one greedy stream per frame and
                                                    Pillow's file; the frames come from the CPU oracle's Nearest path
  python tools/gif_encode_probe.py calls <reps>     flgpu_process_gif with and without FLGPU_ENCODE_GIF: wall time, the encode kernels' HIP-event time, bytes over
                                                    PCIe; the call without the bit plus Pillow's GIF save of the frames it returns (a stand-in for the host's
                                                    GifEncoder, which cannot be built where this runs)
  python tools/gif_encode_probe.py kernels <reps>   the encoding call alone, to run under rocprofv3 --kernel-trace --stats
  python tools/gif_encode_probe.py callers <k>      16 caller threads x k requests on one context, with and without the bit"""
import io, json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as g
import gif_enc_model as em, gif_model, gif_write as gw
fl = g._load_package()

def animation(frames=64, side=500):
    """tools/gif_source_probe.py's animation"""
    from PIL import Image
    import synth
    base = Image.fromarray(synth.photo(side, side, 3, index=5)).quantize(255)
    pal, px, ims = base.getpalette(), np.asarray(base), []
    for f in range(frames):
        a = px.copy()
        x, y = 20 + 6 * f, 40 + 5 * f
        a[y:y + 90, x:x + 70] = (np.add.outer(np.arange(90), np.arange(70)) + 3 * f) % 255
        im = Image.fromarray(a, "P"); im.putpalette(pal)
        ims.append(im)
    b = io.BytesIO()
    ims[0].save(b, "GIF", save_all=True, append_images=ims[1:], duration=40, loop=0, optimize=False)
    return b.getvalue()

def pillow_save(frames):
    """Pillow's GIF of the frames (palette per frame, the whole canvas every time as far as its optimiser leaves it)"""
    from PIL import Image
    ims = [Image.fromarray(f if f.shape[-1] == 4 else np.concatenate([f[..., :1]] * 3 + [f[..., 1:]], -1), "RGBA") for f in frames]
    b = io.BytesIO()
    ims[0].save(b, "GIF", save_all=True, append_images=ims[1:], duration=0, loop=0)
    return b.getvalue()

def out(d):
    print(json.dumps(d), flush=True)

INPUTS = {"lenna": (open(os.path.join(ROOT, "tests", "golden", "lenna.gif"), "rb").read(), "w=300&h=200&crop=true"),
          "animation": (animation(), "w=300&h=200")}
mode = sys.argv[1]
GIF = fl.Format(fl.ENCODE_GIF)
if mode == "ratio":
    import oracle_lib
    oracle = oracle_lib.load()
    for name, (data, query) in INPUTS.items():
        canvases = gif_model.from_blob(fl.debug_gif_blob(data))[:8]     # (eight frames say what sixty-four would)
        frames = [oracle.process_pixels(np.ascontiguousarray(c), 300, 200, filter=oracle_lib.FILTER_NEAREST, crop="crop" in query) for c in canvases]
        colours = [em.colours_of(f) for f in frames]
        pals = [em.palette_of(f) for f in frames]
        single = sum(len(gw.lzw_greedy(p[2], max(2, p[1]))) for p in pals)
        row = {"what": "LZW data bytes of the frames (first eight), by segment length", "input": name, "frames": len(frames), "colours_max": max(colours),
               "one_greedy_stream_per_frame": single, "pillow_file_bytes": len(pillow_save(frames))}
        for seg in (512, 1024, 2048, 3838):
            d = sum(len(em.frame_data(p[2], max(2, p[1]), seg)) for p in pals)
            row["segments_of_%d" % seg] = d
            row["ratio_%d" % seg] = d / single
        row["model_file_bytes_2048"] = len(em.encode_file(frames))
        out(row)
elif mode in ("calls", "kernels"):
    reps = int(sys.argv[2])
    with fl.State(device=0, profile=True) as st:
        for name, (data, query) in INPUTS.items():
            for r in range(reps + 1):       # the first is the warm-up
                st.reset_stats()
                a = time.perf_counter(); mime, kind, body = st.process_gif(data, query, GIF); enc = time.perf_counter() - a
                st.stats()
                row = {"what": "flgpu_process_gif with FLGPU_ENCODE_GIF", "input": name, "query": query, "rep": r, "stream": kind == fl.RESULT_GIF_STREAM, "wall_ms": 1e3 * enc,
                       "encode_kernels_us": st.debug_get("gif_encode_ns") / 1e3, "upload_bytes": st.debug_get("gif_upload_bytes"),
                       "download_bytes": len(body) if isinstance(body, bytes) else sum(f.nbytes for f in body)}
                if mode == "calls":
                    st.reset_stats()
                    a = time.perf_counter(); mime, kind0, frames = st.process_gif(data, query); plain = time.perf_counter() - a
                    a = time.perf_counter(); pil = pillow_save(frames); save = time.perf_counter() - a
                    row.update({"without_bit_wall_ms": 1e3 * plain, "without_bit_download_bytes": sum(f.nbytes for f in frames), "pillow_save_ms": 1e3 * save,
                                "without_bit_plus_pillow_ms": 1e3 * (plain + save), "pillow_file_bytes": len(pil), "colours_max": max(em.colours_of(f) for f in frames),
                                "file_is_the_models": isinstance(body, bytes) and body == em.encode_file(frames) if r == 0 else None})
                out(row)
elif mode == "callers":
    threads, per = 16, int(sys.argv[2])
    def run(fn, label):
        with fl.State(device=0) as st:
            fn(st)  # warm-up
            def worker():
                for _ in range(per): fn(st)
            ts = [threading.Thread(target=worker) for _ in range(threads)]
            a = time.perf_counter()
            for t in ts: t.start()
            for t in ts: t.join()
            dt = time.perf_counter() - a
            out({"what": label, "callers": threads, "requests": threads * per, "wall_s": dt, "files_per_s": threads * per / dt, "usable_cpus": len(os.sched_getaffinity(0)),
                 "encoded": st.debug_get("gif_encoded"), "fallbacks": st.debug_get("gif_encode_fallbacks")})
    for rep in range(2):
        for name, (data, query) in INPUTS.items():
            run(lambda st: st.process_gif(data, query, GIF), f"flgpu_process_gif with FLGPU_ENCODE_GIF ({name}), {query}")
            run(lambda st: st.process_gif(data, query), f"flgpu_process_gif without the bit ({name}), {query}: frames back, no encoder behind it")
