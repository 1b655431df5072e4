"""FLGPU_FE_WEBP_LOSSY_LF / _I4_LF / _AP_LF / _I4_AP_LF, the host half: routing and sizing of the four front ends and their accept
bit, the rule's known answers, the restated encoder (tests/vp8_lf_model.py) pinned to the model it restates and judged by libwebp's
decoder -- every file decodes to exactly the model's FILTERED reconstruction, and never to a worse picture than the twin front
end's file --, what the corpus reaches, and the host twin (tests/vp8_host.cpp --filter: the kernels' own functions in plain loops) byte
for byte and cost word for cost word against the model, plain and under ASan + UBSan.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import vp8_ap_cases
import vp8_ap_model as ap
import vp8_host_twin
import vp8_i4_model as m4
import vp8_lf_cases as cases_mod
import vp8_lf_model as lf
import vp8_lib
import vp8_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
PLANES_300x200 = 2 * 300 * 200 + 2 * 150 * 100
VARIANTS = cases_mod.VARIANTS


def _fe(fl, i4, adapt):
    return fl.vp8_front_end(i4, adapt, lf=True)


def _twin(fl, i4, adapt):
    return fl.vp8_front_end(i4, adapt)


def _max_out(w, h, i4, adapt):
    return ap.max_out_bytes(w, h, i4) if adapt else (m4.max_out_bytes(w, h) if i4 else vm.max_out_bytes(w, h))


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


# ------------------------------------------------------------------------------------------------------------- routing --

def test_the_new_bit_selects_the_twin_and_alone_does_nothing(fl):
    assert (fl.FE_WEBP_LOSSY_LF, fl.FE_WEBP_LOSSY_I4_LF, fl.FE_WEBP_LOSSY_AP_LF, fl.FE_WEBP_LOSSY_I4_AP_LF) == (16, 17, 18, 19)
    assert fl.ENCODE_WEBP_LOSSY_FILTER == 0x4000 and fl.load_library().flgpu_abi_version() == 6
    assert (fl.FE_WEBP_LOSSY, fl.FE_WEBP_LOSSY_I4, fl.FE_WEBP_LOSSY_AP, fl.FE_WEBP_LOSSY_I4_AP) == (9, 10, 12, 13), "existing values stay"
    webp, lossy, i4b, probs, filt = fl.ACCEPT_WEBP, fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER
    for fmt in (fl.IN_PNG, fl.IN_JPEG, fl.IN_WEBP):
        for q in ("&quality=1", "&quality=75", "&quality=99", ""):
            query = f"w=300&h=200&webp=true{q}"
            for i4, adapt in VARIANTS:
                bits = lossy | filt | (i4b if i4 else 0) | (probs if adapt else 0)
                rc, kind, plan = _plan(fl, query, webp | bits, fmt)
                assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and (plan.out_w, plan.out_h, plan.out_c) == (300, 200, 4)
                # the twin's worst case: the bound is per boolean, the level's six literals were counted all along
                assert plan.out_bytes == PLANES_300x200 and plan.max_out_bytes == _max_out(300, 200, i4, adapt), (bits, q)
                assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, bits, 300, 200) == _fe(fl, i4, adapt)
                assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, bits & ~filt, 300, 200) == _twin(fl, i4, adapt)
            # the new bit alone, and with every other bit but _LOSSY: the planes, as without it
            for bits in (filt, filt | i4b, filt | probs, filt | i4b | probs):
                rc, kind, plan = _plan(fl, query, webp | bits, fmt)
                assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES and plan.out_bytes == plan.max_out_bytes == PLANES_300x200
    every = lossy | i4b | probs | filt
    assert _plan(fl, "w=300&h=200&webp=true&quality=100", webp | every, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200&webp=true&quality=75", every, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200", webp | every, fl.IN_JPEG)[1] == fl.RESULT_JPEG_STREAM
    # the fall-back from the B_PRED families' limits still applies: 120 x 68 macroblocks
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, every, 1920, 1088) == fl.FE_WEBP_LOSSY_AP_LF
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, lossy | i4b | filt, 1920, 1088) == fl.FE_WEBP_LOSSY_LF
    rc, kind, plan = _plan(fl, "webp=true&quality=75", webp | every, fl.IN_PNG, w=1920, h=1080, c=3)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == ap.max_out_bytes(1920, 1080)
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 100, every, 300, 200) == fl.FE_WEBP_LOSSLESS


def test_the_limits_are_the_twins(fl):
    lib = fl.load_library()
    for w, h, c in ((1, 1, 1), (300, 200, 4), (301, 7, 3), (1, 16383, 3), (1120, 1136, 3)):
        for i4, adapt in VARIANTS:
            plan = fl.plan_output(fl.make_params(quality=75, front_end=_fe(fl, i4, adapt)), w, h, c)
            twin = fl.plan_output(fl.make_params(quality=75, front_end=_twin(fl, i4, adapt)), w, h, c)
            assert (plan.out_w, plan.out_h, plan.out_c, plan.out_bytes, plan.max_out_bytes) == (w, h, c, twin.out_bytes, twin.max_out_bytes)
            assert plan.max_out_bytes == _max_out(w, h, i4, adapt)
    for w, h in ((1136, 1136), (1920, 1080), (2320, 2320), (16384, 1)):
        for i4, adapt in VARIANTS:
            p, t, plan = fl.make_params(front_end=_fe(fl, i4, adapt)), fl.make_params(front_end=_twin(fl, i4, adapt)), fl.flgpu_plan()
            assert lib.flgpu_plan_output(C.byref(p), w, h, 3, C.byref(plan)) == lib.flgpu_plan_output(C.byref(t), w, h, 3, C.byref(plan))
    for fe in (14, 15, 20):
        p, plan = fl.make_params(front_end=fe), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), 64, 64, 3, C.byref(plan)) == fl.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------------ the rule --

def test_the_rule_on_paper():
    # known answers from this repository's own tables
    assert [lf.base_level(qi) for qi in (0, 26, 38, 52, 103)] == [0, 8, 11, 16, 51]
    assert all(0 <= lf.base_level(qi) <= 63 and lf.base_level(qi) != 1 for qi in range(128))
    assert lf.base_level(vm.QUALITY_TO_INDEX[99]) == 0
    assert lf.candidates(0) == [0, 0, 0, 0] and lf.candidates(1) == [0, 1, 1, 2] and lf.candidates(15) == [0, 8, 15, 23]
    assert lf.candidates(27)[3] == 41 and lf.candidates(42) == [0, 21, 42, 63] and lf.candidates(63) == [0, 32, 63, 63]
    # ties go to the lowest level; 64-bit words
    assert lf.choose([0, 8, 16, 24], [5, 5, 5, 5]) == 0 and lf.choose([0, 8, 16, 24], [9, 5, 5, 7]) == 8
    assert lf.choose([0, 32, 63, 63], [1 << 40, (1 << 40) - 1, (1 << 40) - 2, (1 << 40) - 2]) == 63
    # the limits of section 15.2 at sharpness 0, and the three hev classes
    assert lf.limits(1) == (1, 0, 7, 3) and lf.limits(15)[1] == 1 and lf.limits(39)[1] == 1 and lf.limits(40)[1] == 2 and lf.limits(63) == (63, 2, 193, 189)
    # the decode front end's derivation is the shared one (not a second copy)
    src = open(os.path.join(CSRC, "fl_vp8src.cpp")).read()
    core = open(os.path.join(CSRC, "fl_vp8_lf_core.h")).read()
    assert "vp8_filter_strength(level, F.sharpness, o);" in src and "vp8_filter_strength((int)level, 0, fs);" in core
    assert "sharpness > 4" not in core and "level >= 40" not in core


# ---------------------------------------------------------------------------------------------------------- the model --

@pytest.fixture(scope="module")
def cases(oracle):
    """(b_pred, adaptive, name) -> (y, u, v, a or None, quality, base, file, reconstruction, filtered, stats, the twin's file)."""
    out = {}
    for name, img, q, base in cases_mod.corpus():
        y, u, v, has_alpha = oracle.webp_yuv420(img)
        a = np.ascontiguousarray(img[..., 3]) if has_alpha else None
        assert has_alpha == name.endswith("_a")
        key = cases_mod.analysis_key(name)
        for i4, adapt in VARIANTS:
            data, rec, shown, stats = cases_mod.model(key, y, u, v, q, a, i4, adapt, base)
            twin = cases_mod.model(key, y, u, v, q, a, i4, adapt, 0)[0]
            out[(i4, adapt, name)] = (y, u, v, a, q, base, data, rec, shown, stats, twin)
    return out


def test_with_every_candidate_forced_to_0_the_restatement_writes_vp8_ap_models_bytes(cases):
    """`analyse` runs vp8_ap_model's on padded planes and `write` restates its writer; this pins both."""
    bad = []
    for (i4, adapt, name), (y, u, v, a, q, base, data, rec, shown, stats, twin) in cases.items():
        if base is not None:
            continue
        want, want_rec, _ = vp8_ap_cases.model("lf:" + name, y, u, v, q, a, i4, adapt)
        if twin != want or not all(np.array_equal(g, r) for g, r in zip(rec, want_rec)):
            bad.append((i4, adapt, name))
    assert not bad, bad


def _sse(planes, y, u, v):
    return sum(int(((p.astype(np.int64) - s.astype(np.int64)) ** 2).sum()) for p, s in zip(planes, (y, u, v)))


def test_libwebp_decodes_every_file_to_the_filtered_reconstruction_and_no_worse_than_the_twin(fl, cases):
    assert vp8_lib.load() is not None, "libwebp is needed to judge the files"
    bad = []
    for (i4, adapt, name), (y, u, v, a, q, base, data, rec, shown, stats, twin) in cases.items():
        h, w = y.shape
        assert len(data) <= _max_out(w, h, i4, adapt) and data[:4] == b"RIFF" and data[8:12] == b"WEBP", name
        assert int.from_bytes(data[4:8], "little") == len(data) - 8 and len(data) % 2 == 0, name
        got, got_twin = vp8_lib.decode_yuv(data), vp8_lib.decode_yuv(twin)
        if got is None or got[0].shape != (h, w) or not all(np.array_equal(g, r) for g, r in zip(got, shown)):
            bad.append((i4, adapt, name, "decode"))
            continue
        assert all(np.array_equal(g, r) for g, r in zip(got_twin, rec)), name
        info = fl.vp8_info(data)
        if (info["filter_level"], info["filter_type"], info["sharpness"]) != (stats["chosen"], 0, 0):
            bad.append((i4, adapt, name, "header", info["filter_level"], stats["chosen"]))
        # exact, no margin: level 0 is a candidate
        d_new, d_twin = _sse(got, y, u, v), _sse(got_twin, y, u, v)
        if d_new > d_twin or (stats["base"] and (d_new != min(stats["D"]) or d_twin != stats["D"][0])):
            bad.append((i4, adapt, name, "sse", d_new, d_twin, stats["D"]))
        if (stats["chosen"] == 0) != (data == twin) or (stats["base"] == 0 and data != twin):
            bad.append((i4, adapt, name, "twin bytes"))
        assert vp8_lib.features(data) == (w, h, a is not None), name
        if a is not None:
            rgba = vp8_lib.decode_rgba(data)
            assert data[12:16] == b"VP8X" and rgba is not None and np.array_equal(rgba[..., 3], a), name
    assert not bad, bad


def test_the_corpus_reaches_what_it_is_there_for(cases):
    """The conditions tests/vp8_lf_cases.py names, on the I16 / default-probability family and on the B_PRED one."""
    for i4 in (False, True):
        st = {name: c[9] for (v4, adapt, name), c in cases.items() if v4 == i4 and not adapt}
        assert {(s["w"], s["h"]) for s in st.values()} >= {(1, 1), (17, 17), (16, 144), (128, 16), (33, 15), (15, 33), (64, 48), (300, 200)}
        assert sum((s["w"], s["h"]) == (300, 200) for s in st.values()) == 2
        assert {s["base"] for s in st.values()} >= set(cases_mod.FORCED) | {0, 8, 11, 16, 51}
        assert st["photo_64x48_q50_b1"]["levels"] == [0, 1, 1, 2] and st["photo_64x48_q50_b15"]["levels"] == [0, 8, 15, 23]
        assert st["photo_64x48_q50_b27"]["levels"][3] == 41 and st["photo_64x48_q50_b42"]["levels"][3] == 63 == st["photo_17x17_q30_b42"]["levels"][3]
        # each of the four candidate positions is chosen at least twice (the first position that holds the chosen level)
        chosen_at = [s["levels"].index(s["chosen"]) for s in st.values() if s["base"]]
        print("B_PRED" if i4 else "I16", "chosen positions:", [chosen_at.count(k) for k in range(4)])
        assert all(chosen_at.count(k) >= 2 for k in range(4)), chosen_at
        # level 0 wins with L0 > 0 although the filter changed the picture
        assert any(s["base"] and s["chosen"] == 0 and len(set(s["D"])) > 1 for s in st.values())
        # exact ties between distinct levels at the minimum, resolved downwards; one of them is not a flat picture
        ties = [n for n, s in st.items() if s["base"] and len({lv for lv, d in zip(s["levels"], s["D"]) if d == min(s["D"])}) > 1]
        assert all(st[n]["chosen"] == min(lv for lv, d in zip(st[n]["levels"], st[n]["D"]) if d == min(st[n]["D"])) for n in ties)
        assert "flat_64x48_q75" in ties and any(len(set(st[n]["D"])) > 1 for n in ties), ties
        # the runner-up's D within 1 % of the winner's and different from it: at least three
        near = [n for n, s in st.items() if s["base"] and len(set(s["D"])) > 1 and (sorted(set(s["D"]))[1] - min(s["D"])) * 100 <= min(s["D"])]
        print("near misses:", near)
        assert len(near) >= 3, near
        # no macroblock with Y2 levels alone and sixteen zero DCs: it cannot be constructed (tests/vp8_lf_cases.py says why)
        assert not any(s["y2_only"].any() for s in st.values())
        # macroblocks with and without filtered inner edges, in one picture too
        assert any(s["inner"].any() and not s["inner"].all() for s in st.values())
    # with B_PRED allowed the diagonal wave has skipped B_PRED macroblocks, and their inner edges are filtered all the same
    s = cases[(True, False, "wave32_64x48_q30")][9]
    assert (s["skip"] & s["is4"]).any() and s["inner"][s["skip"] & s["is4"]].all() and s["chosen"] > 0
    # an I16 macroblock that is skipped keeps its inner edges
    s = cases[(False, False, "edges0_48x48_q1")][9]
    assert s["skip"].any() and not s["inner"][s["skip"]].any()
    # quality 99: base level 0, nothing evaluated
    s = cases[(False, False, "photo_64x48_q99")][9]
    assert s["base"] == 0 and s["D"] == [0, 0, 0, 0] and s["chosen"] == 0


# ------------------------------------------------------------------------------------------------------- the host twin --

@pytest.mark.parametrize("sanitised", (False, True), ids=("plain", "asan_ubsan"))
def test_the_host_twin_writes_the_models_bytes_and_prints_its_costs(cases, tmp_path, sanitised):
    """The kernels' own functions in plain loops, as a program of its own; the second build runs them under ASan + UBSan."""
    exe = vp8_host_twin.build(tmp_path, sanitised)
    bad = []
    for (i4, adapt, name), (y, u, v, a, q, base, data, rec, shown, stats, twin) in cases.items():
        got = vp8_host_twin.run(exe, tmp_path, y, u, v, a, q, i4=i4, adaptive=adapt, filt=True, filter_base=base, files=("shown",))
        if (got["file"] != data or got["shown"] != b"".join(p.tobytes() for p in shown)
                or got["levels"] != stats["levels"] or got["D"] != stats["D"] or got["chosen"] != stats["chosen"]):
            bad.append((i4, adapt, name, got["levels"], got["D"], got["chosen"]))
    assert not bad, bad
