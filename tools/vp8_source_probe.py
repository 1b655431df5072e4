"""Measurements of the lossy WebP decode front end on one MI355X (profiles/pr_webp_lossy_source.txt):
  host     the host half per 1080p photograph and thread beside libwebp's whole WebPDecodeRGB, and files/s for 64 callers
  device   HIP-event time of the decode kernels for one picture and for a batch of 64, beside the resample kernel's
  trace    (run under rocprofv3 --kernel-trace --stats) one picture four times (a warm-up and three timed), then a batch of 64 four
           times: per-kernel times
usage: python tools/vp8_source_probe.py host|device|trace"""
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import synth  # noqa: E402
import vp8_dec_lib  # noqa: E402

fl = conftest.load_package()


def photograph():
    img = synth.photo(1080, 1920, 3, index=7)
    return vp8_dec_lib.encode(np.dstack([img, np.full((1080, 1920), 255, np.uint8)]), 75)


def best(fn, n=5):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t), sorted(t)[len(t) // 2]


def host(data):
    info = fl.vp8_info(data)
    print("file bytes", len(data), "blob bytes", info["blob_bytes"], "decoded bytes", 1920 * 1080 * 3,
          {k: info[k] for k in ("macroblocks", "bpred_macroblocks", "skipped_macroblocks", "filter_level", "segmentation", "partitions")})
    lib = fl.load_library()
    import ctypes as C
    out = np.zeros(info["blob_bytes"], np.uint8)
    used = C.c_uint64()
    one = lambda: lib.flgpu_debug_vp8_blob(data, len(data), out.ctypes.data, out.nbytes, C.byref(used))  # noqa: E731
    print("host half per file and thread: best %.2f ms, median %.2f ms" % tuple(1e3 * v for v in best(one, 9)))
    print("libwebp WebPDecodeRGB:          best %.2f ms, median %.2f ms" % tuple(1e3 * v for v in best(lambda: vp8_dec_lib.decode_pixels(data, 3), 9)))
    for run in range(2):   # steady: every caller decodes until five seconds have passed
        outs = [np.zeros(info["blob_bytes"], np.uint8) for _ in range(64)]
        done = [0] * 64
        t0 = time.perf_counter()
        def worker(k):
            u = C.c_uint64()
            while time.perf_counter() - t0 < 5.0:
                lib.flgpu_debug_vp8_blob(data, len(data), outs[k].ctypes.data, outs[k].nbytes, C.byref(u))
                done[k] += 1
        th = [threading.Thread(target=worker, args=(k,)) for k in range(64)]
        [t.start() for t in th]
        [t.join() for t in th]
        dt = time.perf_counter() - t0
        print("host half, 64 callers for %.1f s, %d CPUs usable by this process: %d files, %.0f files/s" % (dt, len(os.sched_getaffinity(0)), sum(done), sum(done) / dt))


def device(data, rounds):
    p = fl.make_params(300, 200)
    with fl.State(device=0, profile=True) as st:
        for name, batch in (("one picture", 1), ("batch of 64", 64)):
            srcs = [fl.LossyWebp(data)] * batch
            st.process_batch(srcs, [p] * batch)   # warm: buffers, tables
            for _ in range(rounds):
                st.reset_stats()
                t0 = time.perf_counter()
                st.process_batch(srcs, [p] * batch)
                wall = time.perf_counter() - t0
                s = st.stats()
                print("%s: decode kernels %.3f ms, resample %.3f ms, wall %.1f ms (host halves on one thread included)"
                      % (name, st.debug_get("vp8_decode_ns") / 1e6, s["resample_ms"], wall * 1e3))


if __name__ == "__main__":
    what = sys.argv[1]
    data = photograph()
    if what == "host":
        host(data)
    elif what == "device":
        device(data, 2)
    else:
        device(data, 3)
