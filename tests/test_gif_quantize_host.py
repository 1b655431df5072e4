"""The GIF quantiser (FLGPU_ENCODE_GIF_QUANTIZE) without a GPU: the constants, the model of the rule (tests/gif_quant_model.py) and its
invariants on every case, the model's files under Pillow and under the library's own host decoder, the host twin of the kernels'
arithmetic (tests/gif_quant_host.cpp over csrc/fl_gif_quant_core.h, plain and under ASan + UBSan), the routing of the size limit, and
the quality condition: on nine inputs, at K = 256 and K = 255, the model's squared error is no larger than that of Pillow's median cut
without dithering at the same colour count (Pillow stands in for the reference's NeuQuant, which cannot be run here)."""
import ctypes
import io
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gif_enc_model as em
import gif_quant_cases as qc
import gif_quant_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_the_constants_are_mirrored(fl):
    api = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert re.search(r"#define FLGPU_ENCODE_GIF_QUANTIZE 0x8000u", api) and re.search(r"#define FLGPU_ABI_VERSION 6\b", api)
    assert re.search(r"pub const ENCODE_GIF_QUANTIZE: u32 = 0x8000;", open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read())
    assert fl.ENCODE_GIF_QUANTIZE == 0x8000
    flags = [getattr(fl, n) for n in dir(fl) if n.startswith(("ENCODE_", "ACCEPT_")) and isinstance(getattr(fl, n), int)]
    assert len(flags) == len(set(flags)) and all(f & (f - 1) == 0 for f in flags)          # a bit of its own
    core = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_gif_quant_core.h")).read()
    assert int(re.search(r"kGifQuantHashCells = (\d+);", core).group(1)) == qm.MAX_CELLS
    assert re.search(r"kGifQuantMaxPixels = 1u << 22;", core) and qm.MAX_PIXELS == 1 << 22


def test_the_bit_leaves_every_plan_alone(fl):
    """the plan of a GIF request is FLGPU_ENCODE_GIF's, with or without the new bit; alone the bit does nothing"""
    lib = fl.load_library()
    data = qc.get("colours_257")[0]

    def plan_of(query, flags):
        plan, kind, frames = fl.flgpu_plan(), ctypes.c_int(), ctypes.c_uint32()
        rc = lib.flgpu_process_gif_plan(data, len(data), query.encode(), flags, ctypes.byref(plan), ctypes.byref(frames), ctypes.byref(kind))
        return rc, kind.value, frames.value, bytes(plan)
    for query in ("webp=true", "w=40&h=30", "grayscale=true", ""):
        assert plan_of(query, fl.ENCODE_GIF | fl.ENCODE_GIF_QUANTIZE) == plan_of(query, fl.ENCODE_GIF)
        assert plan_of(query, fl.ENCODE_GIF_QUANTIZE) == plan_of(query, 0)
    assert plan_of("webp=true", fl.ENCODE_GIF | fl.ENCODE_GIF_QUANTIZE)[1] == fl.RESULT_GIF_STREAM


def test_a_frame_above_the_limit_is_routed_back_to_pixels():
    """2 ** 22 pixels is the last size the 64-bit products are sized for: N Q and S S stay below 2 ** 60 there, and a larger frame
    above 256 colours makes the model (as the host does by clearing the job's quant word) return no file"""
    N, c = qm.MAX_PIXELS, 255
    assert N * (N * c * c) < 1 << 60 and (N * c) ** 2 < 1 << 60 and N * c < 1 << 30
    run = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_gifrun.cpp")).read()
    assert re.search(r"J\.quant = quantize && gif_quantizable\(J\.px, frames\) \? 1u : 0u;", run)
    head = open(os.path.join(ROOT, "fanlin-rs_amd", "csrc", "fl_gif.h")).read()
    assert re.search(r"gif_quantizable\(uint64_t pixels, uint64_t frames\) \{ return pixels <= kGifQuantMaxPixels && ", head)
    rng = np.random.default_rng(5)
    big = np.zeros((2049, 2048, 4), np.uint8)          # 2 ** 22 + 2,048 pixels
    big[..., 3] = 255
    big[0, :300, :3] = rng.integers(0, 256, (300, 3))
    assert qm.marked(big) and qm.encode_file([big]) is None
    big[0, :300, :3] = 0
    assert not qm.marked(big)                          # at most 256 colours: the exact branch has no such limit


# ---- the model on every case ----------------------------------------------------------------------------------------------------------

def test_the_cases_are_what_their_names_say():
    def last(name):
        return qm.quantize(qc.frames_of(name)[-1])
    for name, colours in (("colours_257", 257), ("colours_272", 272), ("colours_4096", 4096), ("colours_4097", 4097), ("pixels_285", 280)):
        f = qc.frames_of(name)[-1]
        assert em.colours_of(f) == colours and (f[..., 3] == 255).all(), name
    assert [em.colours_of(f) for f in qc.frames_of("fallback_in_the_middle")] == [256, 257, 4]
    assert [last(n)["s"] for n in ("colours_272", "colours_4096", "colours_4097", "dark_s1", "dark_s2", "noise_128", "noise_128_s3")] == [0, 0, 1, 1, 2, 3, 3]
    assert last("colours_4096")["cells"] == 4096 and last("noise_128")["cells"] > 4096 and last("noise_128_s3")["cells"] == 5000
    assert qc.frames_of("noise_128_s3").shape[1:3] == (128, 128)
    q = last("one_clear_pixel")
    assert (q["K"], q["boxes"], q["transparent"]) == (255, 255, 255) and (q["indices"] == 255).sum() == 1
    f = qc.frames_of("exact_with_clear_colours")[0]
    q = qm.quantize(f)
    assert em.colours_of(f) == 272 and (q["boxes"], q["transparent"]) == (200, 200) and qm.squared_error(f, qm.to_rgba(f)) == 0.0
    f = qc.frames_of("no_opaque_pixel")[0]
    q = qm.quantize(f)
    assert em.colours_of(f) == 260 and (q["boxes"], q["transparent"], len(q["table"])) == (0, 0, 1) and not q["indices"].any()
    f = qc.frames_of("luma_alpha_257")[0]
    assert f.shape[-1] == 2 and em.colours_of(f) == 257 and qm.quantize(f)["K"] == 255
    assert qc.frames_of("pixels_285").shape[1] * qc.frames_of("pixels_285").shape[2] % 4 == 1
    assert len(qc.frames_of("eight_frames_all_marked")) == 8 and all(qm.marked(f) for f in qc.frames_of("eight_frames_all_marked"))


def test_the_constructed_ties():
    # mirror halves: the two boxes of the first split have the same priority, and the lower number goes first
    trace = []
    f = qc.frames_of("ties_between_boxes")[0]
    q = qm.quantize(f, trace)
    assert (trace[0]["box"], trace[0]["cut"], trace[0]["low"], trace[0]["high"]) == (0, 127, 128, 128)
    assert trace[1]["priority"] == trace[2]["priority"] and (trace[1]["box"], trace[2]["box"]) == (0, 1)
    # 255 boxes for 256 colours: one entry stands for two neighbours x, x + 1 as x + 1, so x is as far from it as from x - 1's: the lower index
    table = q["table"][:255, 0].astype(int)
    x = next(v for v in range(256) if v not in table)
    assert q["boxes"] == 255 and x - 1 in table and x + 1 in table
    rgb, opaque = qm.rgb_of(f)
    at = int(np.flatnonzero(opaque & (rgb[:, 0] == x))[0])
    assert table[q["indices"][at]] == x - 1
    # the same V on r and g (g is a permutation of r): r is cut
    trace = []
    g = qc.frames_of("ties_between_axes")[0]
    qm.quantize(g, trace)
    n = np.ones(256, np.int64)
    c = np.unique(g.reshape(-1, 4)[g.reshape(-1, 4)[:, 3] != 0][:, :3].astype(np.int64), axis=0)
    N, S, Q = qm.box_stats(n, c, np.ones(256, bool))
    assert N * Q[0] - S[0] ** 2 == N * Q[1] - S[1] ** 2 > N * Q[2] - S[2] ** 2 and trace[0]["axis"] == 0


@pytest.mark.parametrize("name", qc.FRAMES)
def test_model_invariants(name):
    for f in qc.frames_of(name):
        if not qm.marked(f):
            assert qm.palette_of(f)[2].tolist() == em.palette_of(f)[2].tolist()           # the exact branch, untouched
            continue
        trace = []
        q = qm.quantize(f, trace)
        rgb, opaque = qm.rgb_of(f)
        assert q["boxes"] <= q["K"] and len(q["table"]) <= 256 and q["boxes"] == 1 + len(trace) - (0 if opaque.any() else 1)
        assert all(t["low"] > 0 and t["high"] > 0 and t["V"] > 0 for t in trace)           # both halves of every split
        assert (q["transparent"] is None) == bool(opaque.all())
        if q["transparent"] is not None:
            assert q["transparent"] == q["boxes"] and (q["indices"][~opaque] == q["transparent"]).all() and (q["indices"][opaque] < q["boxes"]).all()
        assert [tuple(e) for e in q["table"][:q["boxes"]]] == sorted(tuple(e) for e in q["table"][:q["boxes"]])
        if len(np.unique(rgb[opaque], axis=0)) <= q["K"]:
            assert qm.squared_error(f, qm.to_rgba(f)) == 0.0                                # few enough colours end in an exact palette


@pytest.mark.parametrize("name", qc.FRAMES)
def test_pillow_reads_the_model_files(name):
    """Pillow and the model's own to_rgba read the model's file to the same frames.  Frame by frame in files of one frame: a viewer's
    composition of disposal 1 over a transparent pixel is not the frame itself."""
    from PIL import Image
    for f in qc.frames_of(name):
        if f.shape[-1] == 2:
            f = np.concatenate([f[..., :1]] * 3 + [f[..., 1:]], -1)
        im = Image.open(io.BytesIO(qm.encode_file([f])))
        assert np.array_equal(np.asarray(im.convert("RGBA")), qm.to_rgba(f)), name


def test_the_library_decoder_reads_the_model_files(fl):
    """the library's own host half: the table and the indices of every frame as the model wrote them"""
    import gif_model as gm
    for name in ("fallback_in_the_middle", "one_clear_pixel", "colours_4097", "no_opaque_pixel", "luma_alpha_257"):
        frames = qc.frames_of(name)
        data = qm.encode_file(frames)
        info = fl.gif_info(data)
        assert (info["supported"], info["frames"]) == (1, len(frames)) and len(data) <= em.max_file_bytes(len(frames), frames.shape[1] * frames.shape[2], frames.shape[-1])
        blob = fl.debug_gif_blob(data)
        buf = np.frombuffer(blob, np.uint8)
        for r, f in zip(gm.blob_records(blob), frames):
            table, bits, idx, transparent = qm.palette_of(f)
            assert np.array_equal(buf[r["idx_off"]:r["idx_off"] + len(idx)], idx)
            assert np.array_equal(buf[r["pal_off"]:r["pal_off"] + 1024].reshape(256, 4), gm.palette_of(table, transparent))


# ---- the host twin ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitised", (False, True), ids=("plain", "asan_ubsan"))
def test_the_host_twin_reproduces_the_model(tmp_path, sanitised):
    """csrc/fl_gif_quant_core.h's functions in plain loops, as a program of its own; the second build runs them under ASan + UBSan"""
    exe = str(tmp_path / "gif_quant_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitised else []) +
                   [os.path.join(ROOT, "tests", "gif_quant_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    for name in qc.FRAMES:
        frames = qc.frames_of(name)
        src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("<4I", len(frames), frames.shape[1], frames.shape[2], frames.shape[3]) + np.ascontiguousarray(frames).tobytes())
        r = subprocess.run([exe, src, out], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        got = open(out, "rb").read()
        at = 0
        for f in frames:
            (mark,) = struct.unpack_from("<I", got, at)
            at += 4
            assert bool(mark) == qm.marked(f), name
            if not mark:
                continue
            q = qm.quantize(f)
            entries, transparent, s, cells = struct.unpack_from("<4I", got, at)
            at += 16
            assert (entries, transparent, s, cells) == (len(q["table"]), 0xffffffff if q["transparent"] is None else q["transparent"], q["s"], q["cells"]), name
            assert got[at:at + 3 * entries] == q["table"].tobytes(), name
            at += 3 * entries
            assert got[at:at + len(q["indices"])] == q["indices"].tobytes(), name
            at += len(q["indices"])
        assert at == len(got)


# ---- quality: no worse than Pillow's median cut -------------------------------------------------------------------------------------

def quality_inputs():
    from PIL import Image
    rng = np.random.default_rng(2024)
    lenna = Image.open(os.path.join(GOLDEN, "lenna_reference.jpg")).convert("RGB")
    out = {"lenna_512": np.asarray(lenna.resize((512, 512), Image.LANCZOS)) if lenna.size != (512, 512) else np.asarray(lenna),
           "lenna_300x200": np.asarray(lenna.resize((300, 200), Image.LANCZOS)), "lenna_48x32": np.asarray(lenna.resize((48, 32), Image.LANCZOS))}
    pal = Image.open(os.path.join(GOLDEN, "lenna.gif")).convert("RGB").resize((200, 200), Image.NEAREST)
    box = np.full((200, 300, 3), 32, np.uint8)
    box[:, 50:250] = np.asarray(pal)
    box[0, 0] = (255, 0, 255)                                                             # one colour more than the fill's 257
    out["lenna_gif_letterboxed"] = box
    y, x = np.mgrid[0:64, 0:96]
    out["gradient_96x64"] = np.stack([x * 255 // 95, y * 255 // 63, (x + y) * 255 // 158], -1).astype(np.uint8)
    v = rng.choice(1 << 24, 4096, replace=False)
    out["noise_64_4096_colours"] = np.stack([v >> 16, v >> 8 & 255, v & 255], -1).astype(np.uint8).reshape(64, 64, 3)
    out["noise_128"] = rng.integers(0, 256, (128, 128, 3)).astype(np.uint8)
    out["dark_noise_96"] = rng.integers(0, 24, (96, 96, 3)).astype(np.uint8)
    out["noise_17x16"] = rng.integers(0, 256, (16, 17, 3)).astype(np.uint8)
    return out


def model_and_pillow(rgb, K):
    """(the model's, Pillow's) mean squared error at K colours; at K = 255 the frame has one clear pixel more, which neither counts"""
    from PIL import Image
    f = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], -1)
    if K == 255:
        f = np.concatenate([f, np.zeros((1,) + f.shape[1:], np.uint8)], 0)                # a clear row: K = 255 for the rest
    ours = qm.squared_error(f, qm.to_rgba(f))
    pil = np.asarray(Image.fromarray(rgb, "RGB").quantize(K, method=Image.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB")).astype(np.int64)
    return ours, float(((rgb.astype(np.int64) - pil) ** 2).mean())


def test_no_worse_than_pillow_median_cut():
    rows, bad = [], []
    for name, rgb in quality_inputs().items():
        for K in (256, 255):
            ours, pil = model_and_pillow(rgb, K)
            rows.append("%-24s K=%d model %9.3f  Pillow %9.3f" % (name, K, ours, pil))
            if ours > pil:
                bad.append(rows[-1])
    print("\n".join(rows))
    assert not bad, bad
