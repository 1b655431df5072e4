"""FLGPU_FE_WEBP_LOSSY, the host half: routing and sizing of the new front end, the restated encoder (tests/vp8_model.py) judged by
libwebp's decoder -- every file decodes to exactly the model's reconstruction --, the host twin (tests/vp8_host.cpp: the kernels'
own functions in plain loops) byte for byte against the model, and the coder measured against libwebp's encoder on the same
planes.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import vp8_cases
import vp8_host_twin
import vp8_lib
import vp8_model as vm
import webp_lib

PLANES_300x200 = 2 * 300 * 200 + 2 * 150 * 100

# Measured on the four photo_300x200 pictures (q = 1, 30, 75, 99; a letterboxed synth.photo), this coder against libwebp's encoder
# on the same planes at the same q.  File size ratio 1.035 / 1.483 / 1.622 / 2.059: no B_PRED, no
# rate-distortion search, no per-picture probabilities.  Y-PSNR of each decode against the source planes, libwebp's minus this
# coder's: +1.30 / +0.09 / +0.46 / -0.28 dB.  The files are deterministic; the bars are the worst measured values rounded up to the
# next tenth / the next half dB: room for an intended change and nothing else.
MEASURED_SIZE_RATIO = (1.035, 1.483, 1.622, 2.059)
MEASURED_PSNR_DEFICIT_DB = (1.30, 0.09, 0.46, -0.28)
SIZE_RATIO_BAR = 2.1
PSNR_DEFICIT_BAR_DB = 1.5


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


# ------------------------------------------------------------------------------------------------------------- routing --

def test_the_bit_turns_the_lossy_webp_arm_into_the_stream(fl):
    webp = fl.Format.from_accept_header("image/webp").flags
    for fmt in (fl.IN_PNG, fl.IN_JPEG, fl.IN_OTHER, fl.IN_WEBP):
        for q in ("&quality=1", "&quality=75", "&quality=99", ""):
            query = f"w=300&h=200&webp=true{q}"
            rc, kind, plan = _plan(fl, query, webp | fl.ENCODE_WEBP_LOSSY, fmt)
            assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM, (fmt, q)
            assert (plan.out_w, plan.out_h, plan.out_c) == (300, 200, 4)
            assert plan.out_bytes == PLANES_300x200 and plan.max_out_bytes == vm.max_out_bytes(300, 200)
            # without the bit: the planes, exactly as before
            rc, kind, plan = _plan(fl, query, webp, fmt)
            assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES and plan.out_bytes == plan.max_out_bytes == PLANES_300x200
    # a WebP source that stays WebP: no negotiation needed
    for q in ("&quality=1", "&quality=99", ""):
        rc, kind, plan = _plan(fl, "w=300&h=200" + q, fl.ENCODE_WEBP_LOSSY, fl.IN_WEBP)
        assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == vm.max_out_bytes(300, 200)
        assert _plan(fl, "w=300&h=200" + q, 0, fl.IN_WEBP)[1] == fl.RESULT_WEBP_PLANES
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75) == fl.FE_WEBP_LOSSY
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 100) == fl.result_front_end(fl.RESULT_WEBP_STREAM, 255) == fl.FE_WEBP_LOSSLESS


def test_the_bit_leaves_every_other_outcome_alone(fl):
    for extra in (0, fl.ENCODE_WEBP_LOSSLESS):
        both = fl.Format.from_accept_header("image/webp,image/avif").flags | extra
        for flags in (both, both | fl.ENCODE_WEBP_LOSSY):
            q100 = fl.RESULT_WEBP_STREAM if extra else fl.RESULT_PIXELS
            assert _plan(fl, "w=300&h=200&webp=true&quality=100", flags, fl.IN_PNG)[1] == q100
            assert _plan(fl, "w=300&h=200&webp=true&quality=255", flags, fl.IN_JPEG)[1] == q100
            assert _plan(fl, "w=300&h=200&quality=100", flags, fl.IN_WEBP)[1] == q100
            assert _plan(fl, "w=300&h=200&avif=true&quality=75", flags, fl.IN_PNG)[1] == fl.RESULT_PIXELS
            assert _plan(fl, "w=300&h=200&webp=true&quality=75", flags, fl.IN_GIF_FRAME)[1] == fl.RESULT_PIXELS
            assert _plan(fl, "", flags, fl.IN_WEBP)[1] == fl.RESULT_AS_IS
            assert _plan(fl, "w=300&h=200", flags, fl.IN_JPEG)[1] == fl.RESULT_JPEG_STREAM
            assert _plan(fl, "w=300&h=200", flags, fl.IN_PNG)[1] == fl.RESULT_PIXELS
            assert _plan(fl, "w=300&h=200", flags | fl.ENCODE_PNG, fl.IN_PNG)[1] == fl.RESULT_PNG_STREAM
            assert _plan(fl, "w=9999&h=9999&webp=true", flags, fl.IN_PNG)[0] == fl.ERR_PARSE
    # a client that does not accept WebP: the arm is not taken
    assert _plan(fl, "w=300&h=200&webp=true&quality=75", fl.ENCODE_WEBP_LOSSY, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200&webp=true&quality=75", fl.ENCODE_WEBP_LOSSY, fl.IN_JPEG)[1] == fl.RESULT_JPEG_STREAM


def test_outputs_over_the_limits_keep_the_planes(fl):
    flags = fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY
    # a side above 14 bits; 250 x 250 macroblocks (a token partition's worst case would not fit its 24-bit size)
    for w, h in ((16384, 4), (4, 16384), (20000, 20), (4000, 4000)):
        assert not vm.fits(w, h)
        for f in (flags, fl.ACCEPT_WEBP):
            rc, kind, plan = _plan(fl, "webp=true&quality=75", f, fl.IN_PNG, w=w, h=h, c=3)
            assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES and (plan.out_w, plan.out_h) == (w, h)
            assert plan.out_bytes == plan.max_out_bytes == 2 * w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    for w, h in ((16383, 4), (4, 16383), (2048, 2048)):
        assert vm.fits(w, h)
        rc, kind, plan = _plan(fl, "webp=true&quality=75", flags, fl.IN_PNG, w=w, h=h, c=3)
        assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == vm.max_out_bytes(w, h)


def test_plan_output_admits_front_end_9_and_not_5_7_or_8(fl):
    lib = fl.load_library()
    for w, h, c in ((1, 1, 1), (300, 200, 4), (301, 7, 3), (5000, 1, 2), (1, 16383, 3), (1920, 1080, 3)):
        plan = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_WEBP_LOSSY), w, h, c)
        assert (plan.out_w, plan.out_h, plan.out_c) == (w, h, c)
        assert plan.out_bytes == 2 * w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        assert plan.max_out_bytes == vm.max_out_bytes(w, h) == fl.vp8_max_out_bytes(w, h)
    for fe in (5, 7, 8):
        p, plan = fl.make_params(front_end=fe), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), 64, 64, 3, C.byref(plan)) == fl.ERR_INVALID_ARG, fe
    for w, h in ((16384, 1), (1, 16384), (4000, 4000)):
        p, plan = fl.make_params(front_end=fl.FE_WEBP_LOSSY), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), w, h, 3, C.byref(plan)) == fl.ERR_UNSUPPORTED


def test_the_quality_table_is_the_recalled_curve():
    for q in range(101):
        x = min(max(vm.quality_index_formula(q), 0.0), 127.0)
        assert vm.QUALITY_TO_INDEX[q] in (int(x - 1e-9), int(x + 1e-9)), q
    assert [vm.QUALITY_TO_INDEX[q] for q in (1, 30, 75, 99)] == [103, 52, 26, 0]
    assert vm.quant_steps(0)["y2"] == (8, 8) and vm.quant_steps(127)["uv"][0] == 132 and vm.quant_steps(127)["y2"] == (314, 440)


# ---------------------------------------------------------------------------------------------------------- the model --

@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (y, u, v, a or None, quality, model file, model reconstruction, model stats)."""
    out = {}
    for name, img, q in vp8_cases.corpus():
        y, u, v, has_alpha = oracle.webp_yuv420(img)
        a = np.ascontiguousarray(img[..., 3]) if has_alpha else None
        assert has_alpha == name.endswith("_a")
        data, rec, stats = vp8_cases.model(name, y, u, v, q, a)
        out[name] = (y, u, v, a, q, data, rec, stats)
    return out


def test_libwebp_decodes_every_model_file_to_the_models_reconstruction(cases):
    assert vp8_lib.load() is not None, "libwebp is needed to judge the files"
    bad = []
    for name, (y, u, v, a, q, data, rec, stats) in cases.items():
        h, w = y.shape
        assert len(data) <= vm.max_out_bytes(w, h) and data[:4] == b"RIFF" and data[8:12] == b"WEBP", name
        assert int.from_bytes(data[4:8], "little") == len(data) - 8 and len(data) % 2 == 0, name
        got = vp8_lib.decode_yuv(data)
        if got is None or got[0].shape != (h, w) or not all(np.array_equal(g, r) for g, r in zip(got, rec)):
            bad.append(name)
        feat = vp8_lib.features(data)
        assert feat == (w, h, a is not None), name
        if a is None:
            assert data[12:16] == b"VP8 " and b"VP8X" not in data[:32], name
        else:
            assert data[12:16] == b"VP8X" and data[30:34] == b"ALPH", name
            rgba = vp8_lib.decode_rgba(data)
            assert rgba is not None and np.array_equal(rgba[..., 3], a), name
    assert not bad, bad


def test_the_corpus_reaches_the_paths_it_is_there_for(cases):
    stats = {name: c[7] for name, c in cases.items()}
    assert stats["flat_64x48_q75"]["skipped"] == 4 * 3, "every macroblock of the flat picture is skipped"
    assert stats["noise_64x48_q99"]["cat6"] and not stats["noise_64x48_q1"]["cat6"]
    ramps = [stats[n] for n in ("ramp_h_64x48_q75", "ramp_v_64x48_q75", "ramp_d_64x48_q30")]
    assert set().union(*(s["ymodes"] for s in ramps)) == {vm.DC, vm.V, vm.H, vm.TM}
    assert set().union(*(s["uvmodes"] for s in ramps)) == {vm.DC, vm.V, vm.H, vm.TM}
    assert stats["photo_16x144_q99"]["partitions"] == 8 and stats["photo_64x48_q75"]["partitions"] == 2
    assert stats["photo_128x16_q1"]["partitions"] == 1 and stats["photo_300x200_q75"]["partitions"] == 8
    assert 0 < stats["photo_300x200_q75"]["skipped"] < 13 * 19, "the letterbox bars are skipped, the photo is not"


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)


def test_measured_against_libwebps_encoder(cases):
    assert webp_lib.load() is not None
    sizes, psnrs = [], []
    for k, q in enumerate(vp8_cases.QUALITIES):
        y, u, v, a, _, data, rec, stats = cases[f"photo_300x200_q{q}"]
        ref = webp_lib.encode_planes(y, u, v, q)
        ref_y = vp8_lib.decode_yuv(ref)[0]
        ratio, deficit = len(data) / len(ref), _psnr(ref_y, y) - _psnr(rec[0], y)
        print(f"q={q}: {len(data)} bytes against libwebp's {len(ref)} (ratio {ratio:.3f}); Y-PSNR {_psnr(rec[0], y):.2f} dB against {_psnr(ref_y, y):.2f} dB (deficit {deficit:+.2f})")
        assert ratio <= SIZE_RATIO_BAR and deficit <= PSNR_DEFICIT_BAR_DB, q
        assert abs(ratio - MEASURED_SIZE_RATIO[k]) < 0.01 and abs(deficit - MEASURED_PSNR_DEFICIT_DB[k]) < 0.01, "the record above is stale"
        sizes.append(len(data))
        psnrs.append(_psnr(rec[0], y))
    # independently of libwebp: more quality, more bytes, less error
    assert sizes == sorted(sizes) and len(set(sizes)) == 4 and psnrs == sorted(psnrs) and len(set(psnrs)) == 4


# ------------------------------------------------------------------------------------------------------- the host twin --

def test_the_host_twin_writes_the_models_bytes(cases, tmp_path):
    exe = vp8_host_twin.build(tmp_path)
    bad = []
    for name, (y, u, v, a, q, data, rec, stats) in cases.items():
        got = vp8_host_twin.run(exe, tmp_path, y, u, v, a, q, files=("recon",))
        if got["file"] != data or got["recon"] != b"".join(p.tobytes() for p in rec):
            bad.append(name)
    assert not bad, bad
