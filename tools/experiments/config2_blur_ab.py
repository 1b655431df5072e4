"""Blur of BASELINE config 2 (grey picture on a grey frame) on the window-tile matrix-pipe kernel as ONE channel (the default:
stage 1 leaves the unframed Luma8 picture) and as Rgba8 of the framed picture (the switch no_luma_mid), next to its colour twin.
   python tools/experiments/config2_blur_ab.py"""
import importlib, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
fl = importlib.import_module("fanlin-rs_amd")
n, H, W, C = 1024, 1080, 1920, 3
src = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
for no_luma_mid in (0, 1):
    for kw in (dict(w=300, h=200, blur_sigma=10.0, grayscale=True), dict(w=300, h=200, blur_sigma=10.0)):
        with fl.State(device=0, profile=True) as st:
            st.debug_set("no_luma_mid", no_luma_mid)
            p = fl.make_params(**kw)
            plan = fl.plan_output(p, W, H, C)
            stride = (int(plan.out_bytes) + 255) // 256 * 256
            dst = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
            run = st.prepared_batch([src.data_ptr() + i * H * W * C for i in range(n)], [(H, W, C)] * n, p, [dst.data_ptr() + i * stride for i in range(n)], [stride] * n)
            for _ in range(3): run(stream)
            torch.cuda.synchronize(); st.reset_stats()
            for _ in range(10): run(stream)
            torch.cuda.synchronize()
            s = st.stats()
            print(dict(no_luma_mid=no_luma_mid), kw, "resample %.3f blur %.3f ms; wtile launches %d" % (s["resample_ms"] / 10, s["blur_ms"] / 10, s["wtile_launches"]), flush=True)
