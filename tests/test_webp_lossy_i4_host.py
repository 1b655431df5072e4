"""FLGPU_FE_WEBP_LOSSY_I4, the host half: routing and sizing of the front end and its accept bit, the restated encoder
(tests/vp8_i4_model.py) judged by libwebp's decoder -- every file decodes to exactly the model's reconstruction --, what the corpus
reaches, read from the model's mode map, and the host twin (tests/vp8_host.cpp --i4: the kernels' own functions in plain loops) byte
for byte against the model, plain and under ASan + UBSan.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import vp8_host_twin
import vp8_i4_cases
import vp8_i4_model as m4
import vp8_lib
import vp8_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
PLANES_300x200 = 2 * 300 * 200 + 2 * 150 * 100


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


# ------------------------------------------------------------------------------------------------------------- routing --

def test_both_bits_choose_the_i4_front_end_and_the_new_bit_alone_does_nothing(fl):
    assert fl.FE_WEBP_LOSSY_I4 == 10 and fl.ENCODE_WEBP_LOSSY_I4 == 0x1000
    webp = fl.ACCEPT_WEBP
    for fmt in (fl.IN_PNG, fl.IN_JPEG, fl.IN_OTHER, fl.IN_WEBP):
        for q in ("&quality=1", "&quality=75", "&quality=99", ""):
            query = f"w=300&h=200&webp=true{q}"
            rc, kind, plan = _plan(fl, query, webp | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4, fmt)
            assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and (plan.out_w, plan.out_h, plan.out_c) == (300, 200, 4)
            assert plan.out_bytes == PLANES_300x200 and plan.max_out_bytes == m4.max_out_bytes(300, 200) > vm.max_out_bytes(300, 200)
            rc, kind, plan = _plan(fl, query, webp | fl.ENCODE_WEBP_LOSSY, fmt)
            assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == vm.max_out_bytes(300, 200)
            rc, kind, plan = _plan(fl, query, webp | fl.ENCODE_WEBP_LOSSY_I4, fmt)
            assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES and plan.out_bytes == plan.max_out_bytes == PLANES_300x200
    # quality 100, other arms and clients that do not accept WebP: as without the bit
    both = fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4
    assert _plan(fl, "w=300&h=200&webp=true&quality=100", webp | both, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200&webp=true&quality=100", webp | both | fl.ENCODE_WEBP_LOSSLESS, fl.IN_PNG)[1] == fl.RESULT_WEBP_STREAM
    assert _plan(fl, "w=300&h=200&webp=true&quality=75", both, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200", webp | both, fl.IN_JPEG)[1] == fl.RESULT_JPEG_STREAM
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, both, 300, 200) == fl.FE_WEBP_LOSSY_I4
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, fl.ENCODE_WEBP_LOSSY, 300, 200) == fl.FE_WEBP_LOSSY
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, both, 1920, 1088) == fl.FE_WEBP_LOSSY
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 100, both, 300, 200) == fl.FE_WEBP_LOSSLESS


def test_the_limits_are_the_derived_ones(fl):
    lib = fl.load_library()
    # 117 booleans of at most 7 bits per macroblock in a first partition of at most 2^19 - 1 bytes
    assert m4.PART0_MB_BOOLS == 117 and m4.MAX_MBS == fl.vp8_max_mbs(i4=True) == 5111
    assert (7 * (1126 + 117 * 5111) + 7) // 8 < (1 << 19) <= (7 * (1126 + 117 * 5112) + 7) // 8
    for w, h, c in ((1, 1, 1), (300, 200, 4), (301, 7, 3), (5000, 1, 2), (1, 16383, 3), (1136, 1136, 3)):
        assert m4.fits(w, h)
        plan = fl.plan_output(fl.make_params(quality=75, front_end=fl.FE_WEBP_LOSSY_I4), w, h, c)
        assert (plan.out_w, plan.out_h, plan.out_c) == (w, h, c)
        assert plan.out_bytes == 2 * w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        assert plan.max_out_bytes == m4.max_out_bytes(w, h) == fl.vp8_max_out_bytes(w, h, i4=True)
        mbs = ((w + 15) // 16) * ((h + 15) // 16)
        assert plan.max_out_bytes - vm.max_out_bytes(w, h) in ((7 * 110 * mbs) // 8, (7 * 110 * mbs + 7) // 8)
    # over the limit: the front end is refused, and the accept bits fall back to FE_WEBP_LOSSY
    for w, h in ((1920, 1080), (1152, 1152), (16384, 1)):
        assert not m4.fits(w, h)
        p, plan = fl.make_params(front_end=fl.FE_WEBP_LOSSY_I4), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), w, h, 3, C.byref(plan)) == fl.ERR_UNSUPPORTED
    flags = fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4
    rc, kind, plan = _plan(fl, "webp=true&quality=75", flags, fl.IN_PNG, w=1920, h=1080, c=3)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == vm.max_out_bytes(1920, 1080)
    p, plan = fl.make_params(front_end=11), fl.flgpu_plan()
    assert lib.flgpu_plan_output(C.byref(p), 64, 64, 3, C.byref(plan)) == fl.ERR_INVALID_ARG


def test_the_penalty_is_the_headers(fl):
    src = open(os.path.join(CSRC, "fl_vp8_core.h")).read()
    assert f"kVp8I4PenaltyShift = {m4.PENALTY_SHIFT};" in src and "kVp8Part0MbBoolsI4 = 1 + 1 + 16 * 7 + 3;" in src
    assert [m4.penalty(s) for s in (4, 30, 56, 177)] == [1, 1582, 19208, 1917004]
    assert all(m4.penalty(vm.AC_STEP[qi]) >= 1 for qi in range(128)) and m4.penalty(max(vm.AC_STEP)) < 1 << 27


# ---------------------------------------------------------------------------------------------------------- the model --

@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (y, u, v, a or None, quality, model file, model reconstruction, model stats)."""
    out = {}
    for name, img, q in vp8_i4_cases.corpus():
        y, u, v, has_alpha = oracle.webp_yuv420(img)
        a = np.ascontiguousarray(img[..., 3]) if has_alpha else None
        assert has_alpha == name.endswith("_a")
        data, rec, stats = vp8_i4_cases.model(name, y, u, v, q, a)
        out[name] = (y, u, v, a, q, data, rec, stats)
    return out


def test_libwebp_decodes_every_model_file_to_the_models_reconstruction(cases):
    assert vp8_lib.load() is not None, "libwebp is needed to judge the files"
    bad = []
    for name, (y, u, v, a, q, data, rec, stats) in cases.items():
        h, w = y.shape
        assert len(data) <= m4.max_out_bytes(w, h) and data[:4] == b"RIFF" and data[8:12] == b"WEBP", name
        assert int.from_bytes(data[4:8], "little") == len(data) - 8 and len(data) % 2 == 0, name
        got = vp8_lib.decode_yuv(data)
        if got is None or got[0].shape != (h, w) or not all(np.array_equal(g, r) for g, r in zip(got, rec)):
            bad.append(name)
        assert vp8_lib.features(data) == (w, h, a is not None), name
        if a is None:
            assert data[12:16] == b"VP8 " and b"VP8X" not in data[:32], name
        else:
            assert data[12:16] == b"VP8X" and data[30:34] == b"ALPH", name
            rgba = vp8_lib.decode_rgba(data)
            assert rgba is not None and np.array_equal(rgba[..., 3], a), name
    assert not bad, bad


def _neighbours(stats):
    """[(kind, (y, x) of the first macroblock, (y, x) of the second)] for every pair of adjacent macroblocks of which exactly one is
    B_PRED; kind: 'B|I', 'I|B' (side by side, left first), 'B/I', 'I/B' (the first above the second)."""
    i4 = stats["i4"]
    out = []
    for y in range(i4.shape[0]):
        for x in range(i4.shape[1]):
            for y2, x2, sep in ((y, x + 1, "|"), (y + 1, x, "/")):
                if y2 < i4.shape[0] and x2 < i4.shape[1] and i4[y, x] != i4[y2, x2]:
                    out.append(("BI"[not i4[y, x]] + sep + "BI"[not i4[y2, x2]], (y, x), (y2, x2)))
    return out


def test_the_corpus_reaches_the_paths_it_is_there_for(cases):
    stats = {name: c[7] for name, c in cases.items()}
    sizes = {tuple(c[0].shape[::-1]) for c in cases.values()}
    assert sizes >= set(vp8_i4_cases.SIZES) | {(300, 200)}
    # every one of the ten sub-block modes is chosen
    chosen = set()
    for s in stats.values():
        chosen |= set(s["bmodes"][s["bmodes"] >= 0].tolist())
    assert chosen == set(range(10))
    # every I16 mode beside a B_PRED macroblock; a skipped macroblock beside one; all four adjacencies in one picture
    beside, skipped_beside, all_four = set(), False, []
    for name, s in stats.items():
        pairs = _neighbours(s)
        for kind, first, second in pairs:
            i16 = second if kind[0] == "B" else first
            beside.add(int(s["ymode"][i16]))
            skipped_beside |= bool(s["skip"][i16])
        if {k for k, _, _ in pairs} == {"B|I", "I|B", "B/I", "I/B"}:
            all_four.append(name)
    assert beside == {vm.DC, vm.V, vm.H, vm.TM} and skipped_beside and all_four
    # a flat picture has no B_PRED macroblock and is skipped whole
    assert not stats["flat_48x48_q75"]["i4"].any() and stats["flat_48x48_q75"]["skip"].all()
    assert not stats["flat_17x17_q1_a"]["i4"].any()
    # both ends of the quality range code B_PRED macroblocks somewhere
    for q in (1, 99):
        assert any(s["i4"].any() for n, s in stats.items() if f"_q{q}" in n), q
    # partitions 1, 2, 4, 8; an interior macroblock with eight neighbours that is B_PRED
    assert [stats[n]["partitions"] for n in ("noise_128x16_q30", "photo_17x17_q99", "photo_64x48_q99", "photo_16x64_q75", "photo_16x144_q30")] == [1, 2, 2, 4, 8]
    assert stats["photo_300x200_q75"]["partitions"] == 8 and stats["photo_48x48_q75"]["i4"][1, 1]
    assert 0 < stats["photo_300x200_q75"]["i4"].sum() < 13 * 19 and 0 < stats["photo_300x200_q75"]["skipped"] < 13 * 19


# ------------------------------------------------------------------------------------------------------- the host twin --

@pytest.mark.parametrize("sanitised", (False, True), ids=("plain", "asan_ubsan"))
def test_the_host_twin_writes_the_models_bytes(cases, tmp_path, sanitised):
    """The kernels' own functions in plain loops, as a program of its own; the second build runs them under ASan + UBSan."""
    exe = vp8_host_twin.build(tmp_path, sanitised)
    bad = []
    for name, (y, u, v, a, q, data, rec, stats) in cases.items():
        twin = vp8_host_twin.run(exe, tmp_path, y, u, v, a, q, i4=True, files=("recon", "modes"))
        got = np.frombuffer(twin["modes"], np.uint8).reshape(stats["i4"].shape + (17,))
        want = np.where(stats["i4"][..., None], np.array(m4.RFC_TO_TABLE)[np.maximum(stats["bmodes"], 0)], 0)
        if (twin["file"] != data or twin["recon"] != b"".join(p.tobytes() for p in rec)
                or not np.array_equal(got[..., 0], stats["i4"]) or not np.array_equal(got[..., 1:], want)):
            bad.append(name)
    assert not bad, bad
