"""Measurements of Adam7-interlaced PNG sources (profiles/pr_png_adam7.txt) on the 1920x1080 RGB8 photograph of tools/png_source_probe.py,
written both ways with Paeth on every row (of every pass), zlib level 6.
  python tools/png_adam7_probe.py host                       the host half alone on both files, one thread
  python tools/png_adam7_probe.py batch <n> <reps> <kind>    flgpu_transform_batch of n files, kind = adam7 | plain (run it under
                                                             rocprofv3 --kernel-trace --stats for kernel times); plain uses no new symbol,
                                                             so it also runs against an older library named by FLGPU_LIB"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
import png_adam7_write, png_write, synth
fl = g._load_package()

def out(d):
    print(json.dumps(d), flush=True)

img = synth.photo(1080, 1920, 3, index=3)
mode = sys.argv[1]
if mode == "host":
    files = {"plain": (png_write.write_png(img, 2, filters=4, level=6), False), "adam7": (png_adam7_write.write_png(img, 2, filters=4, level=6), True)}
    for kind, (data, adam7) in files.items():
        t = []
        for _ in range(8):
            a = time.perf_counter(); scan = fl.debug_png_scanlines(data, adam7=adam7); t.append(time.perf_counter() - a)
        out({"what": "host half alone (container walk with CRCs, inflate, Adler-32), 1920x1080 RGB8 Paeth level 6, one thread", "kind": kind,
             "file_bytes": len(data), "scanline_bytes": len(scan), "ms_min": 1e3 * min(t), "ms_median": 1e3 * sorted(t)[4]})
elif mode == "batch":
    n, reps, kind = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    adam7 = kind == "adam7"
    data = png_adam7_write.write_png(img, 2, filters=4, level=6) if adam7 else png_write.write_png(img, 2, filters=4, level=6)
    with fl.State(device=0) as st:
        p = fl.make_params(300, 200)
        one = st.process_png_pixels(data, p, adam7=True) if adam7 else st.process_png_pixels(data, p)
        assert np.array_equal(st.decode_png(data, adam7=True) if adam7 else st.decode_png(data), img)
        src = fl.Adam7Png(data) if adam7 else data
        for r in range(reps + 1):   # the first is the warm-up
            a = time.perf_counter()
            res = st.process_batch([src] * n, [p] * n)
            dt = time.perf_counter() - a
            assert all(np.array_equal(x, one) for x in res[:: max(1, n // 8)])
            out({"what": "flgpu_transform_batch, host inflate serial on the calling thread", "kind": kind, "n": n, "rep": r, "wall_s": dt})
        out({"counters": st.png_counters(), "library": fl.build_info()})
