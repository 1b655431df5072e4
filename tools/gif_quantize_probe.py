"""Measurements of the GIF quantiser (profiles/pr_gif_quantize.txt): flgpu_process_gif with FLGPU_ENCODE_GIF | FLGPU_ENCODE_GIF_QUANTIZE on
  lenna      tests/golden/lenna.gif with w=300&h=200: 256 colours letterboxed onto 32, 32, 32 -- 257 colours, the reference's sample request
  animation  64 frames on a 500 x 500 canvas (a photograph quantised to 256 colours; a 90 x 70 sprite with a local table of 255 other
             colours moving over it, disposal 1), w=300&h=200: every frame above 256 colours
  python tools/gif_quantize_probe.py calls <reps>     wall time with both bits, with FLGPU_ENCODE_GIF alone (the fallback to pixels), without any bit, and
                                                      the last plus Pillow's GIF save of the frames (a stand-in for the host's NeuQuant encoder)
  python tools/gif_quantize_probe.py kernels <reps>   the quantising call alone, to run under rocprofv3 --kernel-trace --stats"""
import io, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as g
import gif_enc_model as em, gif_quant_model as qm, gif_write as gw
fl = g._load_package()

def animation(frames=64, side=500):
    from PIL import Image
    import synth
    base = Image.fromarray(synth.photo(side, side, 3, index=5)).quantize(256)
    table = np.array(base.getpalette()[:768], np.uint8).reshape(256, 3)
    v = np.arange(256)
    local = np.stack([255 - v, (v * 7) % 256, v], 1).astype(np.uint8)           # the sprite's own colours
    out = [gw.Frame(0, 0, np.asarray(base), disposal=1)]
    for f in range(1, frames):
        sprite = ((np.add.outer(np.arange(90), np.arange(70)) + 3 * f) % 255).astype(np.uint8)
        out.append(gw.Frame(20 + 6 * f, 40 + 5 * f, sprite, table=local, disposal=1, delay=4))
    return gw.write_gif(side, side, out, table, head=gw.application_ext(0))

def pillow_save(frames):
    from PIL import Image
    ims = [Image.fromarray(f, "RGBA") for f in frames]
    b = io.BytesIO()
    ims[0].save(b, "GIF", save_all=True, append_images=ims[1:], duration=0, loop=0)
    return b.getvalue()

def out(d):
    print(json.dumps(d), flush=True)

INPUTS = {"lenna": (open(os.path.join(ROOT, "tests", "golden", "lenna.gif"), "rb").read(), "w=300&h=200"), "animation": (animation(), "w=300&h=200")}
mode, reps = sys.argv[1], int(sys.argv[2])
BOTH, GIF = fl.Format(fl.ENCODE_GIF | fl.ENCODE_GIF_QUANTIZE), fl.Format(fl.ENCODE_GIF)
with fl.State(device=0, profile=True) as st:
    for name, (data, query) in INPUTS.items():
        for r in range(reps + 1):       # the first is the warm-up
            st.reset_stats()
            a = time.perf_counter(); mime, kind, body = st.process_gif(data, query, BOTH); enc = time.perf_counter() - a
            st.stats()
            row = {"what": "flgpu_process_gif with FLGPU_ENCODE_GIF | FLGPU_ENCODE_GIF_QUANTIZE", "input": name, "query": query, "rep": r, "stream": kind == fl.RESULT_GIF_STREAM,
                   "wall_ms": 1e3 * enc, "encode_kernels_us": st.debug_get("gif_encode_ns") / 1e3, "quantized_frames": st.debug_get("gif_quantized_frames"),
                   "download_bytes": len(body) if isinstance(body, bytes) else sum(f.nbytes for f in body)}
            if mode == "calls":
                a = time.perf_counter(); mime, kind1, frames = st.process_gif(data, query, GIF); fallback = time.perf_counter() - a
                a = time.perf_counter(); mime, kind0, frames = st.process_gif(data, query); plain = time.perf_counter() - a
                a = time.perf_counter(); pil = pillow_save(frames); save = time.perf_counter() - a
                row.update({"encode_gif_alone_wall_ms": 1e3 * fallback, "encode_gif_alone_is_pixels": kind1 == fl.RESULT_PIXELS, "without_bits_wall_ms": 1e3 * plain,
                            "pillow_save_ms": 1e3 * save, "without_bits_plus_pillow_ms": 1e3 * (plain + save), "pillow_file_bytes": len(pil),
                            "without_bits_download_bytes": sum(f.nbytes for f in frames)})
                if r == 0:
                    # the file against the numpy model: lenna's as it is, the animation's on its first three frames (the model is slow)
                    check = data if name == "lenna" else animation(3)
                    got, px = st.process_gif(check, query, BOTH)[2], st.process_gif(check, query)[2]
                    marked = [qm.marked(f) for f in frames]
                    row.update({"frames": len(frames), "marked_frames": sum(marked), "colours_max": max(em.colours_of(f) for f in frames),
                                "file_is_the_models": isinstance(got, bytes) and got == qm.encode_file(px),
                                "model_mse": [round(qm.squared_error(f, qm.to_rgba(f)), 4) for f in px if qm.marked(f)]})
            out(row)
