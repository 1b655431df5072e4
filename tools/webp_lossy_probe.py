"""Lossy WebP probe (FLGPU_FE_WEBP_LOSSY and, with --i4 / --probs / --filter, FLGPU_FE_WEBP_LOSSY_I4 / the adaptive-probability front ends / the
loop-filtered twin of each beside it): throughput of the device encoder beside the path it replaces -- the FLGPU_FE_WEBP420
planes from the device plus libwebp's WebPEncode per picture on the host's threads --, file sizes and Y-PSNR of both on the same
planes, and the bytes that cross PCIe.  Prints plain text; under `rocprofv3 --kernel-trace --stats` (a run of its own, with
--timing-only) the kernel statistics attribute device time to the four vp8_* kernels, the planes kernel and the resample kernel.

    python tools/webp_lossy_probe.py [--batch 1024] [--iters 5] [--host-threads 16] [--timing-only] [--i4] [--probs] [--filter] [--events]
                                     [--quality 75] [--alpha]
--filter: in the quality part, per loop-filtered front end the chosen level, the file against its twin's, the Y-PSNR gain and a
block-edge measure (mean absolute luma step across macroblock edges over the mean absolute step elsewhere) of the twin's file, the
filtered file and libwebp's own file on the same planes; in the timing part each loop-filtered family right after its twin, and the
histogram of the levels the batch's files carry.
--alpha: instead of the above, FLGPU_FEO_ALPHA_VP8L: the ALPH chunk bytes of a disc, a soft falloff and a ramp without and with the
option beside libwebp's own ALPH for the same plane; then, in interleaved rounds, the time per flagship batch (opaque) and per
translucent twin of it (a disc alpha plane over the same pictures) without and with the option, for FLGPU_FE_WEBP_LOSSY and
FLGPU_FE_WEBP_LOSSY_AP, with the mean file bytes.  With --timing-only as well: only the translucent FLGPU_FE_WEBP_LOSSY batch with the
option, 1 + --iters times (the run to put under `rocprofv3 --kernel-trace --stats`).
--segments: instead of the above, FLGPU_FEO_SEGMENTS: per quality the flagship request's file without and with the option beside
libwebp's on the same planes (bytes, Y-PSNR, Y-PSNR over the lower-activity and the upper-activity half of the macroblocks, the class
indices); then, in interleaved rounds, the time per flagship batch without and with the option, for FLGPU_FE_WEBP_LOSSY and
FLGPU_FE_WEBP_LOSSY_AP: the host's clock around synchronised batches and, with --events, the HIP events the library records around the
encoder's own launches (webp_lossy_ns: the segment kernel is inside, the resample and planes launches are not).  With --timing-only as well: only the FLGPU_FE_WEBP_LOSSY batch, 1 + --iters times, with
the option -- or with --no-option without it (the runs to put under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)


def _edge_measure(y):
    """Mean absolute step across macroblock edges over the mean absolute step elsewhere (both directions)."""
    y = y.astype(np.int64)
    dx, dy = np.abs(np.diff(y, axis=1)), np.abs(np.diff(y, axis=0))
    ex, ey = (np.arange(1, y.shape[1]) % 16) == 0, (np.arange(1, y.shape[0]) % 16) == 0
    edge = float(dx[:, ex].sum() + dy[ey].sum()) / (dx[:, ex].size + dy[ey].size)
    rest = float(dx[:, ~ex].sum() + dy[~ey].sum()) / (dx[:, ~ex].size + dy[~ey].size)
    return edge / rest if rest else 0.0


def _lf_kinds(fl, i4, probs):
    kinds = [("FE_WEBP_LOSSY_LF", fl.FE_WEBP_LOSSY_LF, fl.FE_WEBP_LOSSY)] + ([("FE_WEBP_LOSSY_I4_LF", fl.FE_WEBP_LOSSY_I4_LF, fl.FE_WEBP_LOSSY_I4)] if i4 else [])
    if probs:
        kinds += [("FE_WEBP_LOSSY_AP_LF", fl.FE_WEBP_LOSSY_AP_LF, fl.FE_WEBP_LOSSY_AP)]
        kinds += [("FE_WEBP_LOSSY_I4_AP_LF", fl.FE_WEBP_LOSSY_I4_AP_LF, fl.FE_WEBP_LOSSY_I4_AP)] if i4 else []
    return kinds


def quality(fl, st, i4=False, probs=False, filt=False):
    import synth
    import vp8_lib
    import webp_lib
    big = synth.photo(1080, 1920, 3, index=3)
    print("# 1080p photo -> w=300&h=200&webp=true: device file | libwebp WebPEncode on the same planes, same quality")
    for q in (1, 30, 75, 99):
        pl = st.process_pixels(big, fl.make_params(300, 200, quality=q, front_end=fl.FE_WEBP420))
        dev = st.process_pixels(big, fl.make_params(300, 200, quality=q, front_end=fl.FE_WEBP_LOSSY))
        ref = webp_lib.encode_planes(pl.y, pl.u, pl.v, q)
        dy, ry = vp8_lib.decode_yuv(dev)[0], vp8_lib.decode_yuv(ref)[0]
        print(f"quality {q}: device {len(dev)} bytes, Y-PSNR {_psnr(dy, pl.y):.2f} dB | libwebp {len(ref)} bytes, {_psnr(ry, pl.y):.2f} dB | "
              f"size ratio {len(dev) / len(ref):.3f}, planes {pl.y.nbytes * 2 + pl.u.nbytes * 2} bytes")
        if i4:
            dev4 = st.process_pixels(big, fl.make_params(300, 200, quality=q, front_end=fl.FE_WEBP_LOSSY_I4))
            info = fl.vp8_info(dev4)
            print(f"quality {q}: I4 file has {info['bpred_macroblocks']} B_PRED macroblocks of {13 * 19}, sub-block modes seen {info['bmodes_mask']:#05x}")
            print(f"quality {q}: I4 file {len(dev4)} bytes, Y-PSNR {_psnr(vp8_lib.decode_yuv(dev4)[0], pl.y):.2f} dB | {len(dev4) / len(dev):.3f} of the I16-only "
                  f"file, size ratio to libwebp {len(dev4) / len(ref):.3f}")
        if probs:
            for name, fe, old in [("FE_WEBP_LOSSY_AP", fl.FE_WEBP_LOSSY_AP, dev)] + ([("FE_WEBP_LOSSY_I4_AP", fl.FE_WEBP_LOSSY_I4_AP, dev4)] if i4 else []):
                new = st.process_pixels(big, fl.make_params(300, 200, quality=q, front_end=fe))
                same = all(np.array_equal(a, b) for a, b in zip(vp8_lib.decode_yuv(new), vp8_lib.decode_yuv(old)))
                print(f"quality {q}: {name} file {len(new)} bytes | {len(new) / len(old):.3f} of the non-adaptive file ({len(old)}), size ratio to libwebp "
                      f"{len(new) / len(ref):.3f}, decodes to the non-adaptive file's planes: {same}")
        if filt:
            print(f"quality {q}: libwebp's file: filter level {fl.vp8_info(ref)['filter_level']}, block-edge measure {_edge_measure(ry):.3f} (source planes {_edge_measure(pl.y):.3f})")
            for name, fe, twin_fe in _lf_kinds(fl, i4, probs):
                p = fl.make_params(300, 200, quality=q, front_end=fe)
                new, twin = st.process_pixels(big, p), st.process_pixels(big, fl.make_params(300, 200, quality=q, front_end=twin_fe))
                c = st.debug_vp8_filter_costs(big, p)
                ny, ty = vp8_lib.decode_yuv(new)[0], vp8_lib.decode_yuv(twin)[0]
                print(f"quality {q}: {name}: levels {c['levels']} D {c['D']} -> level {c['chosen']}; file {len(new)} bytes against the twin's {len(twin)}; "
                      f"Y-PSNR {_psnr(ny, pl.y):.2f} dB against {_psnr(ty, pl.y):.2f} ({_psnr(ny, pl.y) - _psnr(ty, pl.y):+.2f}); block-edge measure "
                      f"{_edge_measure(ny):.3f} against the twin's {_edge_measure(ty):.3f}")


def timing(fl, st, batch, iters, host_threads, i4=False, events=False, probs=False, filt=False, q=75):
    import torch
    import synth
    import webp_lib
    nsrc = 16
    srcs = [torch.from_numpy(synth.photo(1080, 1920, 3, index=40 + i)).cuda() for i in range(nsrc)]
    shapes = [(1080, 1920, 3)] * batch
    ptrs = [srcs[i % nsrc].data_ptr() for i in range(batch)]
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    kinds = [("FE_WEBP420", fl.FE_WEBP420), ("FE_WEBP_LOSSY", fl.FE_WEBP_LOSSY)] + ([("FE_WEBP_LOSSY_I4", fl.FE_WEBP_LOSSY_I4)] if i4 else [])
    if probs:
        kinds += [("FE_WEBP_LOSSY_AP", fl.FE_WEBP_LOSSY_AP)] + ([("FE_WEBP_LOSSY_I4_AP", fl.FE_WEBP_LOSSY_I4_AP)] if i4 else [])
    if filt:  # each loop-filtered family right after its twin
        twins = {twin_fe: (name, fe) for name, fe, twin_fe in _lf_kinds(fl, i4, probs)}
        kinds = [k for name, fe in kinds for k in ([(name, fe)] + ([twins[fe]] if fe in twins else []))]
    for name, fe in kinds:
        p = fl.make_params(300, 200, quality=q, front_end=fe)
        ns0 = (st.stats(), st.debug_get("webp_lossy_ns"))[1] if events else 0
        cap = (int(fl.plan_output(p, 1920, 1080, 3).max_out_bytes) + 255) // 256 * 256
        dst = torch.empty(batch * cap, dtype=torch.uint8, device="cuda")
        run = st.prepared_batch(ptrs, shapes, p, [dst.data_ptr() + i * cap for i in range(batch)], [cap] * batch)
        run(stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            run(stream)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
        res = st.batch_results()
        nbytes = [r[1] for r in res]
        out[name] = (dt, nbytes)
        print(f"{name}: {batch} x 1080p RGB8 -> w=300&h=200&webp=true&quality={q}: {dt * 1e3:.2f} ms per batch, {batch / dt:.0f} images/s on the device, "
              f"mean output {np.mean(nbytes):.0f} bytes")
        if fe == fl.FE_WEBP420:
            first = dst[:cap].cpu().numpy()
        if name.endswith("_LF"):
            hist = {}
            for i in range(batch):
                lv = fl.vp8_info(dst[i * cap:i * cap + nbytes[i]].cpu().numpy().tobytes())["filter_level"]
                hist[lv] = hist.get(lv, 0) + 1
            print(f"{name}: levels chosen over the batch {dict(sorted(hist.items()))}")
        if events and fe != fl.FE_WEBP420:
            st.stats()  # (resolves the pending events)
            ns = st.debug_get("webp_lossy_ns")
            print(f"{name}: webp_lossy_ns {(ns - ns0) / (iters + 1) / 1e6:.2f} ms per batch (HIP events around the encoder's launches)")
    # the host half of the path this replaces: WebPEncode of the planes, one picture per call, on the host's threads
    ny, nc = 300 * 200, 150 * 100
    y, u, v = first[:ny].reshape(200, 300), first[ny:ny + nc].reshape(100, 150), first[ny + nc:ny + 2 * nc].reshape(100, 150)
    webp_lib.load()
    n = 16 * host_threads
    with ThreadPoolExecutor(host_threads) as ex:
        t0 = time.perf_counter()
        files = list(ex.map(lambda _: webp_lib.encode_planes(y, u, v, q), range(n)))
        dth = (time.perf_counter() - t0) / n
    dt_p, nb_p = out["FE_WEBP420"]
    dt_l, nb_l = out["FE_WEBP_LOSSY"]
    host_rate = 1.0 / dth
    print(f"host WebPEncode of the planes on {host_threads} threads: {dth * 1e3:.3f} ms per picture, {host_rate:.0f} images/s ({len(files[0])} bytes)")
    print(f"planes + host encode: {min(batch / dt_p, host_rate):.0f} images/s (the slower of the two stages); device encoder: {batch / dt_l:.0f} images/s")
    print(f"encode adds {(dt_l - dt_p) * 1e3:.2f} ms per batch to the planes path")
    if i4:
        dt_4, nb_4 = out["FE_WEBP_LOSSY_I4"]
        print(f"I4 encode adds {(dt_4 - dt_p) * 1e3:.2f} ms per batch to the planes path: {batch / dt_4:.0f} images/s, mean file {np.mean(nb_4):.0f} bytes "
              f"({np.mean(nb_4) / np.mean(nb_l):.3f} of the I16-only file)")
    for name in ("FE_WEBP_LOSSY_LF", "FE_WEBP_LOSSY_I4_LF", "FE_WEBP_LOSSY_AP_LF", "FE_WEBP_LOSSY_I4_AP_LF"):
        if name in out:
            dt_a, nb_a = out[name]
            dt_o, nb_o = out[name[:-3]]
            print(f"{name}: {(dt_a - dt_o) * 1e3:+.2f} ms per batch against {name[:-3]}: {batch / dt_a:.0f} images/s, mean file {np.mean(nb_a):.0f} bytes "
                  f"({np.mean(nb_a) / np.mean(nb_o):.4f} of the twin's)")
    for name in ("FE_WEBP_LOSSY_AP", "FE_WEBP_LOSSY_I4_AP"):
        if name in out:
            dt_a, nb_a = out[name]
            dt_o, nb_o = out[name[:-3]]
            print(f"{name}: {(dt_a - dt_o) * 1e3:+.2f} ms per batch against {name[:-3]}: {batch / dt_a:.0f} images/s, mean file {np.mean(nb_a):.0f} bytes "
                  f"({np.mean(nb_a) / np.mean(nb_o):.3f} of the non-adaptive file)")
    print(f"PCIe per picture: up {1080 * 1920 * 3} bytes of source either way; down {int(np.mean(nb_p))} bytes of planes before, {np.mean(nb_l):.0f} bytes of file now "
          f"({np.mean(nb_l) / np.mean(nb_p):.3f} x)")


def alpha(fl, st, batch, iters, q=75, rounds=3, profile=False):
    import torch
    import synth
    import vp8_alpha_cases as ac
    import vp8_alpha_model as am
    import vp8_cases
    import webp_lib
    print("# ALPH chunk payload of a translucent 300 x 200 picture: raw | FLGPU_FEO_ALPHA_VP8L | libwebp's own (WebPEncode of the same planes)")
    rgb = synth.photo(200, 300, 3, index=61)
    for name, a in () if profile else (("disc", ac.disc()), ("falloff", ac.falloff()), ("alpha_ramp", vp8_cases.alpha_ramp(300, 200))):
        img = vp8_cases._rgba(rgb, a)
        pl = st.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_WEBP420))
        raw = st.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY))
        new = st.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY, alpha_vp8l=True))
        theirs = am.alph_of(webp_lib.encode_planes(pl.y, pl.u, pl.v, q, pl.a))
        ours = am.alph_of(new)
        print(f"{name}: ALPH {len(am.alph_of(raw))} | {len(ours)} (header byte {ours[0]}) | {len(theirs)} bytes ({len(ours) / len(theirs):.2f} x libwebp's); "
              f"file {len(raw)} -> {len(new)} bytes; equals the model: {new == am.with_alpha(raw, pl.a)}")
    nsrc = 16
    d = ac.disc(1920, 1080, 500.0)
    photos = [synth.photo(1080, 1920, 3, index=40 + i) for i in range(nsrc)]
    sets = {"opaque": ([torch.from_numpy(p).cuda() for p in photos], 3),
            "translucent": ([torch.from_numpy(vp8_cases._rgba(p, d)).cuda() for p in photos], 4)}
    stream = torch.cuda.current_stream().cuda_stream
    runs = {}
    if profile:  # a run under rocprofv3: the translucent batch with the option alone, so that the kernel statistics are its own
        sets, rounds = {"translucent": sets["translucent"]}, 1
    for kind, (srcs, c) in sets.items():
        for name, fe in (("FE_WEBP_LOSSY", fl.FE_WEBP_LOSSY), ("FE_WEBP_LOSSY_AP", fl.FE_WEBP_LOSSY_AP))[:1 if profile else 2]:
            for opt in (True,) if profile else (False, True):
                p = fl.make_params(300, 200, quality=q, front_end=fe, alpha_vp8l=opt)
                cap = (int(fl.plan_output(p, 1920, 1080, c).max_out_bytes) + 255) // 256 * 256
                dst = torch.empty(batch * cap, dtype=torch.uint8, device="cuda")
                run = st.prepared_batch([srcs[i % nsrc].data_ptr() for i in range(batch)], [(1080, 1920, c)] * batch, p,
                                        [dst.data_ptr() + i * cap for i in range(batch)], [cap] * batch)
                run(stream)
                torch.cuda.synchronize()
                runs[(kind, name, opt)] = (run, dst, [r[1] for r in st.batch_results()])
    times = {k: [] for k in runs}
    for _ in range(rounds):  # interleaved, so that a drift of the clocks falls on every variant alike
        for k, (run, dst, nbytes) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                run(stream)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters * 1e3)
    for (kind, name, opt), ts in times.items():
        nbytes = runs[(kind, name, opt)][2]
        print(f"{kind} {name} option {int(opt)}: {batch} x 1080p -> w=300&h=200&webp=true&quality={q}: ms per batch {' '.join(f'{t:.2f}' for t in ts)} "
              f"(median {float(np.median(ts)):.2f}), mean file {np.mean(nbytes):.0f} bytes")
    try:
        print("webp_alpha_vp8l:", st.debug_get("webp_alpha_vp8l"))
    except fl.FanlinError:  # (FLGPU_LIB points at a library from before the option: an A/B run)
        print("webp_alpha_vp8l: not in this library")


def segments(fl, st, batch, iters, q=75, rounds=3, profile=False, option=True, events=False):
    import torch
    import synth
    import vp8_lib
    import vp8_seg_model as sm
    import webp_lib
    big = synth.photo(1080, 1920, 3, index=3)
    for qq in () if profile else (1, 30, 75, 99):
        pl = st.process_pixels(big, fl.make_params(300, 200, quality=qq, front_end=fl.FE_WEBP420))
        act = sm.activity(pl.y)
        low = np.zeros(act.size, bool)
        low[np.argsort(act.reshape(-1), kind="stable")[:act.size // 2]] = True
        mask = np.repeat(np.repeat(low.reshape(act.shape), 16, axis=0), 16, axis=1)[:200, :300]
        files = {"twin": st.process_pixels(big, fl.make_params(300, 200, quality=qq, front_end=fl.FE_WEBP_LOSSY)),
                 "segments": st.process_pixels(big, fl.make_params(300, 200, quality=qq, front_end=fl.FE_WEBP_LOSSY, segments=True)),
                 "libwebp": webp_lib.encode_planes(pl.y, pl.u, pl.v, qq)}
        rule = sm.rule(pl.y, sm.vm.QUALITY_TO_INDEX[qq])
        for who, data in files.items():
            y = vp8_lib.decode_yuv(data)[0]
            print(f"quality {qq}: {who} {len(data)} bytes, Y-PSNR {_psnr(y, pl.y):.2f} dB (lower-activity half {_psnr(y[mask], pl.y[mask]):.2f}, upper {_psnr(y[~mask], pl.y[~mask]):.2f})")
        print(f"quality {qq}: classes {rule['qi']} around {sm.vm.QUALITY_TO_INDEX[qq]}, macroblocks per class {rule['counts']}, tree probabilities {rule['prob']}")
    nsrc = 16
    srcs = [torch.from_numpy(synth.photo(1080, 1920, 3, index=40 + i)).cuda() for i in range(nsrc)]
    stream = torch.cuda.current_stream().cuda_stream
    runs = {}
    kinds = (("FE_WEBP_LOSSY", fl.FE_WEBP_LOSSY, option),) if profile else tuple((n, fe, o) for n, fe in (("FE_WEBP_LOSSY", fl.FE_WEBP_LOSSY), ("FE_WEBP_LOSSY_AP", fl.FE_WEBP_LOSSY_AP)) for o in (False, True))
    for name, fe, opt in kinds:
        p = fl.make_params(300, 200, quality=q, front_end=fe, segments=opt)
        cap = (int(fl.plan_output(p, 1920, 1080, 3).max_out_bytes) + 255) // 256 * 256
        dst = torch.empty(batch * cap, dtype=torch.uint8, device="cuda")
        run = st.prepared_batch([srcs[i % nsrc].data_ptr() for i in range(batch)], [(1080, 1920, 3)] * batch, p,
                                [dst.data_ptr() + i * cap for i in range(batch)], [cap] * batch)
        run(stream)
        torch.cuda.synchronize()
        runs[(name, opt)] = (run, dst, [r[1] for r in st.batch_results()])
    times, dev = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(1 if profile else rounds):  # interleaved, so that a drift of the clocks falls on every variant alike
        for k, (run, dst, nbytes) in runs.items():
            torch.cuda.synchronize()
            ns0 = (st.stats(), st.debug_get("webp_lossy_ns"))[1] if events else 0  # (flgpu_get_stats resolves the pending events)
            t0 = time.perf_counter()
            for _ in range(iters):
                run(stream)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters * 1e3)
            if events:
                dev[k].append(((st.stats(), st.debug_get("webp_lossy_ns"))[1] - ns0) / iters / 1e6)
    for (name, opt), ts in times.items():
        print(f"{name} option {int(opt)}: {batch} x 1080p -> w=300&h=200&webp=true&quality={q}: ms per batch {' '.join(f'{t:.2f}' for t in ts)} "
              f"(median {float(np.median(ts)):.2f})" + (f", of which the encoder's launches by device events {' '.join(f'{t:.2f}' for t in dev[(name, opt)])} "
              f"(median {float(np.median(dev[(name, opt)])):.2f})" if events else "") + f", mean file {np.mean(runs[(name, opt)][2]):.0f} bytes")
    try:
        print("webp_lossy_segments:", st.debug_get("webp_lossy_segments"))
    except fl.FanlinError:  # (FLGPU_LIB points at a library from before the option: an A/B run)
        print("webp_lossy_segments: not in this library")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--events", action="store_true", help="a profiling context: also report webp_lossy_ns per batch")
    ap.add_argument("--i4", action="store_true", help="also FLGPU_FE_WEBP_LOSSY_I4")
    ap.add_argument("--probs", action="store_true", help="also FLGPU_FE_WEBP_LOSSY_AP (and, with --i4, FLGPU_FE_WEBP_LOSSY_I4_AP)")
    ap.add_argument("--filter", action="store_true", help="also the loop-filtered twin (FLGPU_FE_WEBP_LOSSY_LF, ...) of every front end selected")
    ap.add_argument("--quality", type=int, default=75, help="the timing part's quality")
    ap.add_argument("--alpha", action="store_true", help="FLGPU_FEO_ALPHA_VP8L: ALPH chunk bytes and batch times without and with the option (instead of the rest)")
    ap.add_argument("--segments", action="store_true", help="FLGPU_FEO_SEGMENTS: files and batch times without and with the option (instead of the rest)")
    ap.add_argument("--no-option", action="store_true", help="with --segments --timing-only: the batch without the option")
    a = ap.parse_args()
    import __graft_entry__ as g
    fl = g._load_package()
    with fl.State(device=0, profile=a.events) as st:
        if a.segments:
            segments(fl, st, a.batch, a.iters, a.quality, profile=a.timing_only, option=not a.no_option, events=a.events)
            return
        if a.alpha:
            alpha(fl, st, a.batch, a.iters, a.quality, profile=a.timing_only)
            return
        if not a.timing_only:
            quality(fl, st, a.i4, a.probs, a.filter)
        timing(fl, st, a.batch, a.iters, a.host_threads, a.i4, a.events, a.probs, a.filter, a.quality)


if __name__ == "__main__":
    main()
