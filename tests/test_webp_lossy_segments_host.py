"""FLGPU_FEO_SEGMENTS / FLGPU_ENCODE_WEBP_LOSSY_SEGMENTS, the host half: the constants and the unchanged struct, the mapping of the accept
bit, the larger worst case and the fall-back limits, the rule's known answers, the restated encoder (tests/vp8_seg_model.py) pinned
to the models it restates and judged by libwebp's decoder -- every corpus file decodes to exactly what the model says a decoder
shows, loop-filtered families with a level above 0 included --, what the corpus reaches, the host twin (tests/vp8_host.cpp --segments: the
kernels' own functions in plain loops) byte for byte against the model, plain and under ASan + UBSan, and the recorded measurement
against libwebp's encoder.  No GPU."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import synth
import vp8_ap_cases
import vp8_ap_model as ap
import vp8_cases
import vp8_host_twin
import vp8_i4_model as m4
import vp8_lf_cases
import vp8_lib
import vp8_model as vm
import vp8_seg_cases as cases_mod
import vp8_seg_model as sm
import webp_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
FAMILIES = cases_mod.FAMILIES
QUALITIES = (1, 30, 75, 99)

# Measured with the model (FE_WEBP_LOSSY with the option) on the planes this file uses, against libwebp's encoder on the same planes
# at the same quality (README.md): the letterboxed 300 x 200 photo, then the flagship planes (synth.photo 1080p
# through the oracle's resize to 300 x 200), each at quality 1 / 30 / 75 / 99.  File size ratio, and libwebp's Y-PSNR minus this
# coder's.  The bars are the worst measured values rounded up to the next tenth / the next half dB, as tests/test_webp_lossy_host.py
# sets its own; the records are checked for staleness at 0.01.
MEASURED_SIZE_RATIO = {"letterbox": (1.160, 1.562, 1.680, 2.034), "flagship": (1.033, 1.523, 1.440, 2.216)}
MEASURED_PSNR_DEFICIT_DB = {"letterbox": (1.28, 0.15, 0.42, -0.07), "flagship": (0.43, -0.10, -0.06, -0.04)}
SIZE_RATIO_BAR = 2.3
PSNR_DEFICIT_BAR_DB = 1.5


def _twin_max_out(w, h, i4, adapt):
    return ap.max_out_bytes(w, h, i4) if adapt else (m4.max_out_bytes(w, h) if i4 else vm.max_out_bytes(w, h))


# ----------------------------------------------------------------------------------------------------------- the ABI --

def test_the_constants_the_header_and_the_shim(fl, tmp_path):
    assert fl.ENCODE_WEBP_LOSSY_SEGMENTS == 0x40000 and fl.FEO_SEGMENTS == 2 and fl.FEO_ALPHA_VP8L == 1 and fl.load_library().flgpu_abi_version() == 6
    assert C.sizeof(fl.flgpu_params) == 28 and fl.flgpu_params.reserved.offset == 26 and fl.flgpu_params.reserved.size == 2
    assert not any(fl.ENCODE_WEBP_LOSSY_SEGMENTS & b for b in (fl.ACCEPT_WEBP, fl.ACCEPT_AVIF, fl.ENCODE_PNG, fl.DECODE_PNG_ADAM7, fl.ENCODE_WEBP_LOSSLESS,
                                                               fl.ENCODE_GIF, fl.ENCODE_GIF_QUANTIZE, fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4,
                                                               fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER, fl.ENCODE_WEBP_LOSSY_ALPHA))
    assert tuple(fl.make_params().reserved) == (0, 0) and tuple(fl.make_params(segments=True).reserved) == (2, 0)
    assert tuple(fl.make_params(segments=True, alpha_vp8l=True).reserved) == (3, 0) and tuple(fl.make_params(alpha_vp8l=True).reserved) == (1, 0)
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert "#define FLGPU_ENCODE_WEBP_LOSSY_SEGMENTS 0x40000u" in header and "#define FLGPU_FEO_SEGMENTS 2u" in header
    assert "#define FLGPU_ABI_VERSION 6" in header and "uint8_t options;" in header
    assert "encode_webp_lossy_segments()" in open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    shim = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    assert "ENCODE_WEBP_LOSSY_SEGMENTS: u32 = 0x40000" in shim and "FEO_SEGMENTS: u8 = 2" in shim
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fanlin_gpu.h"\nint main(void) { printf("%zu %zu %zu %u %u\\n", sizeof(flgpu_params), '
                   'offsetof(flgpu_params, options), offsetof(flgpu_params, reserved), FLGPU_FEO_SEGMENTS, FLGPU_ENCODE_WEBP_LOSSY_SEGMENTS); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["28", "26", "27", "2", str(0x40000)]
    # the rule's constants are stated once in the core header and restated in the model
    core = open(os.path.join(CSRC, "fl_vp8_seg_core.h")).read()
    assert "kVp8SegBinShift = 5" in core and "kVp8SegAmpNum = 3" in core and "kVp8SegSpan = 96" in core and "kVp8SegRounds = 6" in core
    assert (sm.BIN_SHIFT, sm.AMP_NUM, sm.SPAN, sm.ROUNDS) == (5, 3, 96, 6)


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, (plan.out_w, plan.out_h, plan.out_c, plan.out_bytes, plan.max_out_bytes)


def test_the_mapping_of_every_combination_of_the_lossy_bits(fl):
    """flgpu_params_from_query sets the option iff the WebP arm runs below quality 100 and both ENCODE_WEBP_LOSSY and the new bit are
    there; nothing else of the parameters moves.  Of a plan only max_out_bytes moves, and only where the stream is planned."""
    bits = (fl.ENCODE_WEBP_LOSSLESS, fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER, fl.ENCODE_WEBP_LOSSY_ALPHA)
    new = fl.ENCODE_WEBP_LOSSY_SEGMENTS

    def fields(p):
        return [getattr(p, n) for n, _ in fl.flgpu_params._fields_ if n != "reserved"]
    for query, lossy_arm in (("w=300&h=200&webp=true&quality=75", True), ("w=300&h=200&webp=true", True), ("w=300&h=200&webp=true&quality=100", False),
                             ("w=300&h=200&quality=75", False)):
        q = fl.Query.parse(query)
        for accept in (0, fl.ACCEPT_WEBP):
            for on in itertools.product((False, True), repeat=len(bits)):
                flags = accept | sum(b for b, o in zip(bits, on) if o)
                without, fmt0 = q.to_params(fl.Format(flags))
                with_bit, fmt1 = q.to_params(fl.Format(flags | new))
                want = bool(lossy_arm and accept and flags & fl.ENCODE_WEBP_LOSSY)
                assert without.reserved[0] & fl.FEO_SEGMENTS == 0 and bool(with_bit.reserved[0] & fl.FEO_SEGMENTS) == want, (query, hex(flags))
                assert with_bit.reserved[0] & ~fl.FEO_SEGMENTS == without.reserved[0] and with_bit.reserved[1] == 0, (query, hex(flags))
                assert fields(without) == fields(with_bit) and fmt0 == fmt1, (query, hex(flags))
                for fmt in (fl.IN_PNG, fl.IN_JPEG):
                    a, b = _plan(fl, query, flags, fmt), _plan(fl, query, flags | new, fmt)
                    assert a[:2] == b[:2] and a[2][:4] == b[2][:4], (query, hex(flags), fmt)
                    stream = a[1] == fl.RESULT_WEBP_STREAM and bool(flags & fl.ENCODE_WEBP_LOSSY) and lossy_arm
                    if stream:
                        i4, adapt = bool(flags & fl.ENCODE_WEBP_LOSSY_I4), bool(flags & fl.ENCODE_WEBP_LOSSY_PROBS)
                        assert a[2][4] == _twin_max_out(300, 200, i4, adapt) and b[2][4] == sm.max_out_bytes(300, 200, i4, adapt) > a[2][4]
                    else:
                        assert a[2][4] == b[2][4], (query, hex(flags), fmt)
    # the bit alone, and with every other lossy bit but ENCODE_WEBP_LOSSY: the planes, as without it
    for extra in (0, fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS | fl.ENCODE_WEBP_LOSSY_FILTER | fl.ENCODE_WEBP_LOSSY_ALPHA):
        rc, kind, plan = _plan(fl, "w=300&h=200&webp=true&quality=75", fl.ACCEPT_WEBP | new | extra, fl.IN_PNG)
        assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES
        assert tuple(fl.Query.parse("w=300&h=200&webp=true&quality=75").to_params(fl.Format(fl.ACCEPT_WEBP | new | extra))[0].reserved) == (0, 0)
    # a WebP source that stays WebP
    assert _plan(fl, "w=300&h=200&quality=75", fl.ENCODE_WEBP_LOSSY | new, fl.IN_WEBP)[2][4] == sm.max_out_bytes(300, 200)
    # front ends that do not know the option plan as without it
    for fe in (fl.FE_WEBP_LOSSLESS, fl.FE_JPEG, fl.FE_PNG, fl.FE_WEBP420, fl.FE_NONE):
        assert bytes(fl.plan_output(fl.make_params(quality=75, front_end=fe), 300, 200, 4)) == bytes(fl.plan_output(fl.make_params(quality=75, front_end=fe, segments=True), 300, 200, 4)), fe


def test_max_out_bytes_and_the_fall_back_limits(fl):
    lib = fl.load_library()
    assert sm.PART0_SEG_BOOLS == 98 and (sm.max_mbs(True, False), sm.max_mbs(True, True)) == (5024, 4953)
    core = open(os.path.join(CSRC, "fl_vp8_core.h")).read()
    assert ("vp8_max_mbs(true) == 5111 && vp8_max_mbs(true, true) == 5039 && vp8_max_mbs(true, false, true) == 5024 && vp8_max_mbs(true, true, true) == 4953" in core
            and "kVp8Part0SegBools == 98" in core)
    assert [fl.vp8_max_mbs(True, adapt, seg) for seg in (False, True) for adapt in (False, True)] == [5111, 5039, 5024, 4953]
    for fe in fl.FE_WEBP_LOSSY_ALL:
        i4, adapt, _ = fl.vp8_variant(fe)
        for w, h, c in ((1, 1, 1), (300, 200, 4), (301, 7, 3), (1, 16383, 3), (1104, 1136, 3)):
            plain = fl.plan_output(fl.make_params(quality=75, front_end=fe), w, h, c)
            seg = fl.plan_output(fl.make_params(quality=75, front_end=fe, segments=True), w, h, c)
            both = fl.plan_output(fl.make_params(quality=75, front_end=fe, segments=True, alpha_vp8l=True), w, h, c)
            mbs = ((w + 15) // 16) * ((h + 15) // 16)
            assert plain.max_out_bytes == _twin_max_out(w, h, i4, adapt)
            assert seg.max_out_bytes == both.max_out_bytes == sm.max_out_bytes(w, h, i4, adapt)
            # the header's 98 booleans and 2 per macroblock, at 7 bits each (to the rounding of two partition-0 terms)
            assert abs(seg.max_out_bytes - plain.max_out_bytes - 7 * (98 + 2 * mbs) / 8) < 1
            assert (seg.out_w, seg.out_h, seg.out_c, seg.out_bytes) == (plain.out_w, plain.out_h, plain.out_c, plain.out_bytes)
    # a picture within the front end's limits but over the segmented ones is planned (and coded) without the option:
    # 5040 = 72 x 70 and 5025 = 75 x 67 macroblocks for B_PRED (5111 / 5024), 5035 = 95 x 53 and 4958 = 74 x 67 with updates (5039 / 4953)
    for fe, (mw, mh) in ((fl.FE_WEBP_LOSSY_I4, (72, 70)), (fl.FE_WEBP_LOSSY_I4_LF, (75, 67)), (fl.FE_WEBP_LOSSY_I4_AP, (95, 53)), (fl.FE_WEBP_LOSSY_I4_AP_LF, (74, 67))):
        i4, adapt, _ = fl.vp8_variant(fe)
        w, h = 16 * mw, 16 * mh
        assert mw * mh > sm.max_mbs(i4, adapt) and not sm.fits(w, h, i4, adapt) and (ap.fits(w, h, True) if adapt else m4.fits(w, h))
        assert fl.plan_output(fl.make_params(front_end=fe, segments=True), w, h, 3).max_out_bytes == _twin_max_out(w, h, i4, adapt)
    # at the segmented limit itself the option holds: 5024 = 157 x 32, 4953 = 127 x 39
    assert fl.plan_output(fl.make_params(front_end=fl.FE_WEBP_LOSSY_I4, segments=True), 157 * 16, 32 * 16, 3).max_out_bytes == sm.max_out_bytes(157 * 16, 32 * 16, True, False)
    assert fl.plan_output(fl.make_params(front_end=fl.FE_WEBP_LOSSY_I4_AP, segments=True), 127 * 16, 39 * 16, 3).max_out_bytes == sm.max_out_bytes(127 * 16, 39 * 16, True, True)
    # the I16 families stay bound by the token partitions' 24-bit field: where they fit at all, the option fits too
    for w, h in ((2048, 2048), (16383, 4), (1920, 1080)):
        assert vm.fits(w, h) and sm.fits(w, h, False, True)
    # what does not fit the front end is refused as before, with or without the option
    for w, h in ((16384, 1), (4000, 4000), (2320, 2320)):
        for fe in (fl.FE_WEBP_LOSSY, fl.FE_WEBP_LOSSY_I4_AP_LF):
            a, b, plan = fl.make_params(front_end=fe), fl.make_params(front_end=fe, segments=True), fl.flgpu_plan()
            assert lib.flgpu_plan_output(C.byref(a), w, h, 3, C.byref(plan)) == lib.flgpu_plan_output(C.byref(b), w, h, 3, C.byref(plan)) != fl.OK


# ------------------------------------------------------------------------------------------------------------ the rule --

def _mbs(values):
    """A luma plane of one row of macroblocks, macroblock k alternating between 128 - values[k] and 128 + values[k] (act = 256 v)."""
    y = np.zeros((16, 16 * len(values)), np.uint8)
    for k, v in enumerate(values):
        y[:, 16 * k:16 * k + 16] = 128 - v
        y[::2, 16 * k:16 * k + 16:2] = 128 + v
        y[1::2, 16 * k + 1:16 * k + 16:2] = 128 + v
    return y


def test_the_rule_on_paper():
    # activity and bins: half the samples at m - v, half at m + v: act = 256 v, bin = 8 v
    y = _mbs([0, 1, 2, 31, 32, 127])
    assert sm.activity(y).tolist() == [[0, 256, 512, 7936, 8192, 32512]] and np.minimum(255, sm.activity(y) >> 5).tolist() == [[0, 8, 16, 248, 255, 255]]
    # edge replication: a 17 x 17 plane's right and bottom macroblocks repeat the last column / row
    e = np.zeros((17, 17), np.uint8)
    e[:, 16] = 200
    e[16, :] = 100
    assert sm.activity(e)[0, 1] == 0 and sm.activity(e)[1, 0] == 0 and sm.activity(e)[1, 1] == 0 and sm.activity(e)[0, 0] == 0
    # degenerate: one macroblock, only flat ones, one occupied bin (with flat ones beside it)
    for values in ([5], [0, 0, 0], [4, 4, 4], [0, 4, 0, 4]):
        r = sm.rule(_mbs(values), 52)
        assert not r["on"] and r["qi"] == [52] * 4 and r["prob"] == [255] * 3 and not r["map"].any(), values
    # two bins: classes 0 and 3, the lower below qi and the upper above; the flat macroblock is class 0 and stays out of the centres
    r = sm.rule(_mbs([0, 2, 2, 2, 20]), 52)
    assert r["on"] and r["map"].tolist() == [[0, 0, 0, 0, 3]] and r["centres"][0] == 16 and r["centres"][3] == 160 and r["counts"] == [4, 0, 0, 1]
    mid = (16 * 3 + 160 + 2) // 4
    assert mid == 52 and r["qi"][0] == 52 - (36 * 19) // 96 and r["qi"][3] == min(52 + 19, 52 + (108 * 19) // 96) and r["prob"] == [204, 255, 1]
    # ties go to the lowest class; offsets truncate towards zero; the clamps at 0 and 127
    assert sm._trunc_div(-7, 2) == -3 and sm._trunc_div(7, 2) == 3
    assert max(sm.rule(_mbs([1, 1, 1, 31]), 127)["qi"]) == 127 and min(sm.rule(_mbs([1, 31, 31, 31]), 2)["qi"]) >= 0
    r = sm.rule(_mbs([1, 1, 1, 31]), 0)   # amp = 1: (248 - 68) / 96 = 1 upwards, (8 - 68) / 96 = 0 downwards
    assert r["on"] and r["qi"] == [0, 0, 0, 1]
    assert not sm.rule(_mbs([1, 1, 11, 11]), 0)["on"], "amp = 1 and a spread below 96 bins: every offset is 0"
    # the tree's probabilities
    assert sm.tree_prob(5, 0) == 255 and sm.tree_prob(0, 5) == 1 and sm.tree_prob(1, 1) == 128 and sm.tree_prob(1000, 1) == 255 and sm.tree_prob(3, 1) == 191


# ---------------------------------------------------------------------------------------------------------- the model --

@pytest.fixture(scope="module")
def cases(oracle):
    """(family, name) -> (y, u, v, a or None, quality, file, reconstruction, what a decoder shows, stats, the twin's file)."""
    out = {}
    for name, img, q in cases_mod.corpus():
        y, u, v, has_alpha = oracle.webp_yuv420(img)
        a = np.ascontiguousarray(img[..., 3]) if has_alpha else None
        assert has_alpha == name.endswith("_a")
        for family, (i4, adapt, filt) in FAMILIES.items():
            data, rec, shown, stats = cases_mod.model(name, y, u, v, q, a, i4, adapt, filt)
            twin = cases_mod.model(name, y, u, v, q, a, i4, adapt, filt, segments=False)[0]
            out[(family, name)] = (y, u, v, a, q, data, rec, shown, stats, twin)
    return out


def test_with_segmentation_off_the_restatement_writes_the_existing_models_bytes(cases):
    """`analyse` and `write` restate vp8_ap_model's loop and vp8_lf_model's writer; this pins both, for the three families."""
    bad = []
    for (family, name), (y, u, v, a, q, data, rec, shown, stats, twin) in cases.items():
        i4, adapt, filt = FAMILIES[family]
        if filt:
            want = vp8_lf_cases.model("seg:" + name, y, u, v, q, a, i4, adapt, None)[0]
        else:
            want = vp8_ap_cases.model("seg:" + name, y, u, v, q, a, i4, adapt)[0]
        if twin != want:
            bad.append((family, name))
    assert not bad, bad
    y, u, v, a, q = cases[("FE_WEBP_LOSSY", "letterbox_300x200_q75")][:5]
    assert cases[("FE_WEBP_LOSSY", "letterbox_300x200_q75")][9] == vm.encode(y, u, v, q)[0]


def _sse(p, s):
    return int(((p.astype(np.int64) - s.astype(np.int64)) ** 2).sum())


def test_libwebp_decodes_every_corpus_file_to_what_the_model_shows(fl, cases):
    assert vp8_lib.load() is not None, "libwebp is needed to judge the files"
    bad, filtered_segmented = [], 0
    for (family, name), (y, u, v, a, q, data, rec, shown, stats, twin) in cases.items():
        i4, adapt, filt = FAMILIES[family]
        h, w = y.shape
        assert len(data) <= sm.max_out_bytes(w, h, i4, adapt) and data[:4] == b"RIFF" and data[8:12] == b"WEBP", name
        assert int.from_bytes(data[4:8], "little") == len(data) - 8 and len(data) % 2 == 0, name
        got = vp8_lib.decode_yuv(data)
        if got is None or got[0].shape != (h, w) or not all(np.array_equal(g, r) for g, r in zip(got, shown)):
            bad.append((family, name, "decode"))
            continue
        if not filt and not all(np.array_equal(g, r) for g, r in zip(got, rec)):
            bad.append((family, name, "unfiltered"))
        info = fl.vp8_info(data)
        if info["filter_level"] != stats["chosen"]:
            bad.append((family, name, "level", info["filter_level"], stats["chosen"]))
        filtered_segmented += bool(stats["seg"]["on"] and stats["chosen"] > 0)
        assert vp8_lib.features(data) == (w, h, a is not None), name
        if a is not None:
            rgba = vp8_lib.decode_rgba(data)
            assert rgba is not None and np.array_equal(rgba[..., 3], a), name
        # degenerate pictures, and only those: the twin's bytes
        if (data == twin) != (not stats["seg"]["on"]):
            bad.append((family, name, "twin bytes"))
    assert not bad, bad
    assert filtered_segmented >= 4, "segmented files with a chosen level above 0: the four filter strengths of the header are exercised"


def test_the_corpus_reaches_what_it_is_there_for(cases):
    st = {name: c[8] for (family, name), c in cases.items() if family == "FE_WEBP_LOSSY"}
    for name in cases_mod.DEGENERATE + ("gradnoise_192x64_q99",):
        assert not st[name]["seg"]["on"], name
        for family in FAMILIES:
            assert cases[(family, name)][5] == cases[(family, name)][9], (family, name)
    assert all(s["seg"]["on"] for n, s in st.items() if n not in cases_mod.DEGENERATE + ("gradnoise_192x64_q99",))
    assert {(s["w"], s["h"]) for s in st.values()} >= {(1, 1), (17, 17), (33, 15), (16, 144), (192, 64), (64, 64), (300, 200), (304, 272)}
    assert st["photo_304x272_q75"]["mbw"] * st["photo_304x272_q75"]["mbh"] == 323 and vm.partitions(st["photo_16x144_q30"]["mbh"]) == 8
    # exactly two used classes, the lower below qi and the upper above; quality 1 clamps at 127
    for q in (1, 30, 75):
        s = st[f"gradnoise_192x64_q{q}"]
        seg = s["seg"]
        assert [c > 0 for c in seg["counts"]] == [True, False, False, True] and seg["qi"][0] < s["qi"] < seg["qi"][3], q
        assert (seg["map"][:, :6] == 0).all() and (seg["map"][:, 6:] == 3).all()
    assert st["gradnoise_192x64_q1"]["seg"]["qi"][3] == 127 and st["gradnoise_192x64_q1"]["qi"] + (3 * st["gradnoise_192x64_q1"]["qi"] >> 3) > 127
    # quality 99: amp = 1, the lower offset clamps at index 0, and the picture is segmented all the same
    s = st["skew_256x32_q99"]
    assert s["qi"] == 0 and s["seg"]["on"] and s["seg"]["qi"] == [0, 0, 0, 1]
    # four used classes with strictly rising indices, one band each
    for q in (30, 75):
        seg = st[f"bands_64x64_q{q}"]["seg"]
        assert seg["counts"] == [4, 4, 4, 4] and seg["qi"] == sorted(set(seg["qi"])) and seg["map"].tolist() == [[k] * 4 for k in range(4)], q
    # the letterbox bars are flat, class 0, and do not pull the centres down: the lowest centre is a photo macroblock's bin
    seg = st["letterbox_300x200_q75"]["seg"]
    assert (seg["bins"][:2] == 0).all() and (seg["bins"][-2:] == 0).all() and (seg["map"][:2] == 0).all() and seg["centres"][0] >= seg["bins"][seg["bins"] > 0].min()
    # partial macroblocks take part, a flat macroblock beside non-flat ones
    assert st["photo_17x17_q75"]["seg"]["on"] and (st["photo_17x17_q75"]["seg"]["bins"] == 0).any()
    # a probability of 255 (no flag literal) and one below, unused classes written
    assert any(255 in s["seg"]["prob"] and min(s["seg"]["prob"]) < 255 for s in st.values() if s["seg"]["on"])
    assert any(0 in s["seg"]["counts"] for s in st.values() if s["seg"]["on"])
    # B_PRED and I16 macroblocks in one segmented picture; the penalty follows the class
    s4 = cases[("FE_WEBP_LOSSY_I4_AP", "letterbox_300x200_q75")][8]
    assert s4["seg"]["on"] and 0 < s4["is4"].sum() < 13 * 19


def test_the_gradient_half_improves_and_the_file_shrinks(cases):
    """On the two-class picture the gradient half (class 0, a finer step) has no more squared error than in the twin's file and the
    file is smaller.  Qualities 30 and 75, the three families."""
    for family in FAMILIES:
        for q in (30, 75):
            y, u, v, a, _, data, rec, shown, stats, twin = cases[(family, f"gradnoise_192x64_q{q}")]
            twin_y = vp8_lib.decode_yuv(twin)[0]
            e_new, e_twin = _sse(shown[0][:, :96], y[:, :96]), _sse(twin_y[:, :96], y[:, :96])
            n_new, n_twin = _sse(shown[0][:, 96:], y[:, 96:]), _sse(twin_y[:, 96:], y[:, 96:])
            print(f"{family} q={q}: {len(twin)} -> {len(data)} bytes; gradient half SSE {e_twin} -> {e_new}, noise half {n_twin} -> {n_new}")
            assert e_new <= e_twin and len(data) < len(twin), (family, q)


# ------------------------------------------------------------------------------------------------------- measurements --

def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)


def _halves(y, dec):
    """Luma PSNR over the lower-activity and the upper-activity half of the macroblocks (by act, ties by raster order)."""
    act = sm.activity(y)
    order = np.argsort(act.reshape(-1), kind="stable")
    low = np.zeros(act.size, bool)
    low[order[:act.size // 2]] = True
    mask = np.repeat(np.repeat(low.reshape(act.shape), 16, axis=0), 16, axis=1)[:y.shape[0], :y.shape[1]]
    return _psnr(dec[mask], y[mask]), _psnr(dec[~mask], y[~mask])


def measurement_planes(oracle):
    import oracle_lib
    flagship = oracle.process_pixels(synth.photo(1080, 1920, 3, index=3), 300, 200, arith=oracle_lib.ARITH_REF)
    return {"letterbox": oracle.webp_yuv420(vp8_cases.letterboxed_photo())[:3], "flagship": oracle.webp_yuv420(flagship)[:3]}


def measure(oracle):
    """-> rows (picture, quality, {coder: (bytes, psnr, psnr of the low half, psnr of the high half)}) for the segmented file, its
    twin and libwebp's."""
    rows = []
    for pic, (y, u, v) in measurement_planes(oracle).items():
        for q in QUALITIES:
            seg = cases_mod.model(f"measure:{pic}:{q}", y, u, v, q)
            twin = cases_mod.model(f"measure:{pic}:{q}", y, u, v, q, segments=False)
            ref = webp_lib.encode_planes(y, u, v, q)
            row = {}
            for who, data, dec in (("segments", seg[0], seg[2][0]), ("twin", twin[0], twin[2][0]), ("libwebp", ref, vp8_lib.decode_yuv(ref)[0])):
                row[who] = (len(data), _psnr(dec, y)) + _halves(y, dec)
            rows.append((pic, q, row))
    return rows


def test_measured_against_libwebps_encoder(oracle):
    assert webp_lib.load() is not None and vp8_lib.load() is not None
    for pic, q, row in measure(oracle):
        k = QUALITIES.index(q)
        ratio, deficit = row["segments"][0] / row["libwebp"][0], row["libwebp"][1] - row["segments"][1]
        print(f"{pic} q={q}: " + "; ".join(f"{who} {r[0]} bytes, Y-PSNR {r[1]:.2f} dB (low half {r[2]:.2f}, high half {r[3]:.2f})" for who, r in row.items())
              + f"; ratio {ratio:.3f}, deficit {deficit:+.2f}")
        assert ratio <= SIZE_RATIO_BAR and deficit <= PSNR_DEFICIT_BAR_DB, (pic, q)
        assert abs(ratio - MEASURED_SIZE_RATIO[pic][k]) < 0.01 and abs(deficit - MEASURED_PSNR_DEFICIT_DB[pic][k]) < 0.01, "the record above is stale"


# ------------------------------------------------------------------------------------------------------- the host twin --

@pytest.mark.parametrize("sanitised", (False, True), ids=("plain", "asan_ubsan"))
def test_the_host_twin_writes_the_models_bytes(cases, tmp_path, sanitised):
    """The kernels' own functions in plain loops, as a program of its own; the second build runs them under ASan + UBSan."""
    exe = vp8_host_twin.build(tmp_path, sanitised)
    bad = []
    for (family, name), (y, u, v, a, q, data, rec, shown, stats, twin) in cases.items():
        i4, adapt, filt = FAMILIES[family]
        for segments, want in ((True, data), (False, twin)):
            got = vp8_host_twin.run(exe, tmp_path, y, u, v, a, q, i4=i4, adaptive=adapt, filt=filt, segments=segments, files=("shown",))
            seg = stats["seg"]
            if got["file"] != want:
                bad.append((family, name, segments, "file"))
            if segments and (got["shown"] != b"".join(p.tobytes() for p in shown) or got["seg_on"] != int(seg["on"])
                             or got["seg_qi"] != seg["qi"] or got["seg_prob"] != seg["prob"] or got["chosen"] != stats["chosen"]):
                bad.append((family, name, got))
    assert not bad, bad
