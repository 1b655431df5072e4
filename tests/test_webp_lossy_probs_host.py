"""FLGPU_FE_WEBP_LOSSY_AP / FLGPU_FE_WEBP_LOSSY_I4_AP, the host half: routing and sizing of the two front ends and their accept bit,
the cost table against its formula, the restated encoder (tests/vp8_ap_model.py) pinned to the two models it restates and judged by
libwebp's decoder -- every file decodes to exactly the reconstruction of the non-adaptive front end --, what the corpus reaches,
the sizes, and the host twin (tests/vp8_host.cpp --adaptive: the kernels' own functions in plain loops) byte for byte against the model,
plain and under ASan + UBSan.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import vp8_ap_cases
import vp8_ap_model as ap
import vp8_cases
import vp8_host_twin
import vp8_i4_cases
import vp8_i4_model as m4
import vp8_lib
import vp8_model as vm
import webp_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
PLANES_300x200 = 2 * 300 * 200 + 2 * 150 * 100
VARIANTS = (False, True)  # B_PRED macroblocks allowed?

# Measured with the model on the oracle's planes of the letterboxed 300 x 200 photo, quality 1 / 30 / 75 / 99: the adaptive file's
# bytes over the non-adaptive front end's, and over libwebp's (webp_lib.encode_planes, same planes, same quality), per variant.
# The files are deterministic; a change of these figures is a change of the rule or of the coder.
MEASURED_VS_NON_ADAPTIVE = {False: (0.906, 0.792, 0.732, 0.559), True: (0.906, 0.939, 0.940, 0.727)}
MEASURED_VS_LIBWEBP = {False: (0.937, 1.174, 1.187, 1.152), True: (0.937, 1.254, 1.137, 1.094)}
# (The non-adaptive files are 1.035 / 1.483 / 1.622 / 2.059 and 1.035 / 1.335 / 1.210 / 1.505 of libwebp's.  At quality 30 the B_PRED
# variant's adaptive file, 2172 bytes, is larger than the I16-only one's, 2034: its mode decision sees prediction error, not rate.)


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, plan


# ------------------------------------------------------------------------------------------------------------- routing --

def test_the_new_bit_selects_the_adaptive_front_ends_and_alone_does_nothing(fl):
    assert (fl.FE_WEBP_LOSSY_AP, fl.FE_WEBP_LOSSY_I4_AP, fl.ENCODE_WEBP_LOSSY_PROBS) == (12, 13, 0x2000)
    assert fl.load_library().flgpu_abi_version() == 6
    webp, lossy, i4, probs = fl.ACCEPT_WEBP, fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS
    for fmt in (fl.IN_PNG, fl.IN_JPEG, fl.IN_OTHER, fl.IN_WEBP):
        for q in ("&quality=1", "&quality=75", "&quality=99", ""):
            query = f"w=300&h=200&webp=true{q}"
            for flags, want in ((lossy | probs, ap.max_out_bytes(300, 200)), (lossy | i4 | probs, ap.max_out_bytes(300, 200, True)),
                                (lossy, vm.max_out_bytes(300, 200)), (lossy | i4, m4.max_out_bytes(300, 200))):
                rc, kind, plan = _plan(fl, query, webp | flags, fmt)
                assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and (plan.out_w, plan.out_h, plan.out_c) == (300, 200, 4)
                assert plan.out_bytes == PLANES_300x200 and plan.max_out_bytes == want, (flags, q)
            # the new bit alone, and with only _I4: the planes, as without it
            for flags in (probs, probs | i4):
                rc, kind, plan = _plan(fl, query, webp | flags, fmt)
                assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES and plan.out_bytes == plan.max_out_bytes == PLANES_300x200
    # quality 100, other arms and clients that do not accept WebP: as without the bit
    every = lossy | i4 | probs
    assert _plan(fl, "w=300&h=200&webp=true&quality=100", webp | every, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200&webp=true&quality=100", webp | every | fl.ENCODE_WEBP_LOSSLESS, fl.IN_PNG)[1] == fl.RESULT_WEBP_STREAM
    assert _plan(fl, "w=300&h=200&webp=true&quality=75", every, fl.IN_PNG)[1] == fl.RESULT_PIXELS
    assert _plan(fl, "w=300&h=200", webp | every, fl.IN_JPEG)[1] == fl.RESULT_JPEG_STREAM
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, lossy | probs, 300, 200) == fl.FE_WEBP_LOSSY_AP
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, every, 300, 200) == fl.FE_WEBP_LOSSY_I4_AP
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, every, 1920, 1088) == fl.FE_WEBP_LOSSY_AP
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 75, lossy | i4, 300, 200) == fl.FE_WEBP_LOSSY_I4
    assert fl.result_front_end(fl.RESULT_WEBP_STREAM, 100, every, 300, 200) == fl.FE_WEBP_LOSSLESS


def test_the_limits_are_the_derived_ones_and_the_fall_backs_work(fl):
    lib = fl.load_library()
    # 9574 booleans in the fixed part of a first partition of at most 2^19 - 1 bytes
    assert ap.PART0_BOOLS == 9574 and ap.I4_MAX_MBS == fl.vp8_max_mbs(i4=True, ap=True) == 5039 == (599185 - 9574) // 117
    assert (7 * (9574 + 117 * 5039) + 7) // 8 < (1 << 19) <= (7 * (9574 + 117 * 5040) + 7) // 8
    src = open(os.path.join(CSRC, "fl_vp8_core.h")).read()
    assert "kVp8Part0BoolsAp = 29 + 1056 * 9 + 9 + 32;" in src
    for w, h, c in ((1, 1, 1), (300, 200, 4), (301, 7, 3), (5000, 1, 2), (1, 16383, 3), (1120, 1136, 3)):
        for i4, fe in ((False, fl.FE_WEBP_LOSSY_AP), (True, fl.FE_WEBP_LOSSY_I4_AP)):
            assert ap.fits(w, h, i4)
            plan = fl.plan_output(fl.make_params(quality=75, front_end=fe), w, h, c)
            assert (plan.out_w, plan.out_h, plan.out_c) == (w, h, c)
            assert plan.out_bytes == 2 * w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
            assert plan.max_out_bytes == ap.max_out_bytes(w, h, i4) == fl.vp8_max_out_bytes(w, h, i4, ap=True)
            assert plan.max_out_bytes - (m4.max_out_bytes(w, h) if i4 else vm.max_out_bytes(w, h)) == (7 * 8448 + 7) // 8 == 7392
    # the I16-only variant stays bound by the token partitions' 24-bit field: exactly the pictures FE_WEBP_LOSSY takes
    for w, h in ((1920, 1080), (2304, 2304), (2320, 2320), (16383, 16), (16384, 1), (16383, 16383)):
        assert ap.fits(w, h) == vm.fits(w, h)
        p, plan = fl.make_params(front_end=fl.FE_WEBP_LOSSY_AP), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), w, h, 3, C.byref(plan)) == (fl.OK if vm.fits(w, h) else fl.ERR_UNSUPPORTED)
    # 71 x 71 = 5041 macroblocks: over 13's limit, within 10's and 12's
    assert m4.fits(1136, 1136) and ap.fits(1136, 1136) and not ap.fits(1136, 1136, True)
    for w, h in ((1136, 1136), (1920, 1080), (16384, 1)):
        p, plan = fl.make_params(front_end=fl.FE_WEBP_LOSSY_I4_AP), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), w, h, 3, C.byref(plan)) == fl.ERR_UNSUPPORTED
    every = fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS
    # 13 -> 12, and never 13 -> 10 (FE_WEBP_LOSSY_I4's worst case differs from FE_WEBP_LOSSY_AP's, so max_out_bytes tells them apart)
    rc, kind, plan = _plan(fl, "webp=true&quality=75", every, fl.IN_PNG, w=1136, h=1136, c=3)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == ap.max_out_bytes(1136, 1136) != m4.max_out_bytes(1136, 1136)
    rc, kind, plan = _plan(fl, "webp=true&quality=75", every, fl.IN_PNG, w=1120, h=1136, c=3)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == ap.max_out_bytes(1120, 1136, True)
    rc, kind, plan = _plan(fl, "webp=true&quality=75", every, fl.IN_PNG, w=1920, h=1080, c=3)
    assert rc == fl.OK and kind == fl.RESULT_WEBP_STREAM and plan.max_out_bytes == ap.max_out_bytes(1920, 1080)
    # 12 -> planes: an output no lossy WebP front end takes
    assert not vm.fits(2320, 2320)
    for flags in (every, fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_PROBS):
        rc, kind, plan = _plan(fl, "webp=true&quality=75", flags, fl.IN_PNG, w=2320, h=2320, c=3)
        assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES and plan.out_bytes == plan.max_out_bytes
    # 11 and 14 are not front ends
    for fe in (11, 14):
        p, plan = fl.make_params(front_end=fe), fl.flgpu_plan()
        assert lib.flgpu_plan_output(C.byref(p), 64, 64, 3, C.byref(plan)) == fl.ERR_INVALID_ARG


def test_the_cost_table_is_its_formula():
    assert len(ap.BIT_COST) == 256
    for p in range(1, 256):
        exact = -256.0 * math.log2(p / 256.0)
        assert abs(ap.BIT_COST[p] - exact) <= 0.5 + 1e-9 and ap.BIT_COST[p] == math.floor(exact + 0.5), p
    assert ap.BIT_COST[128] == 256 and ap.BIT_COST[1] == 2048 and ap.BIT_COST[255] == 1
    # the rule on paper: never visited -> kept; only zeros -> 255; only ones -> 1; the candidate rounds to nearest
    assert ap.candidate(0, 0) == 255 and ap.candidate(7, 0) == 255 and ap.candidate(0, 7) == 1 and ap.candidate(1, 1) == 128
    assert ap.candidate(1, 1000) == 1 and ap.candidate(1000, 1) == 255 and ap.candidate(3, 1) == 191
    assert all(ap.decide(i, 0, 0) == ap.DEFAULT[i] for i in range(ap.N))
    # a picture at the macroblock limit: millions of visits at up to 2048 each need 64-bit sums; the decision still pays
    assert ap.decide(0, 8_000_000, 8_000_000) == ap.DEFAULT[0] == 128 and ap.decide(0, 8_000_000, 1_000_000) == 227


# ---------------------------------------------------------------------------------------------------------- the model --

@pytest.fixture(scope="module")
def cases(oracle):
    """(b_pred, name) -> (y, u, v, a or None, quality, adaptive file, reconstruction, stats, non-adaptive file)."""
    out = {}
    for i4 in VARIANTS:
        for name, img, q in vp8_ap_cases.corpus(i4):
            y, u, v, has_alpha = oracle.webp_yuv420(img)
            a = np.ascontiguousarray(img[..., 3]) if has_alpha else None
            assert has_alpha == name.endswith("_a")
            data, rec, stats = vp8_ap_cases.model(name, y, u, v, q, a, i4)
            plain = vp8_ap_cases.model(name, y, u, v, q, a, i4, adapt=False)[0]
            out[(i4, name)] = (y, u, v, a, q, data, rec, stats, plain)
    return out


def test_without_updates_the_restatement_writes_the_two_models_bytes(cases):
    """The macroblock loop and the partition writers are restated in vp8_ap_model; this pins them to vp8_model / vp8_i4_model."""
    bad = []
    for (i4, name), (y, u, v, a, q, data, rec, stats, plain) in cases.items():
        want, want_rec, _ = (vp8_i4_cases.model if i4 else vp8_cases.model)("ap:" + name, y, u, v, q, a)
        if plain != want or not all(np.array_equal(g, r) for g, r in zip(rec, want_rec)):
            bad.append((i4, name))
    assert not bad, bad


def test_libwebp_decodes_every_file_to_the_non_adaptive_reconstruction(cases):
    assert vp8_lib.load() is not None, "libwebp is needed to judge the files"
    bad = []
    for (i4, name), (y, u, v, a, q, data, rec, stats, plain) in cases.items():
        h, w = y.shape
        assert len(data) <= ap.max_out_bytes(w, h, i4) and data[:4] == b"RIFF" and data[8:12] == b"WEBP", name
        assert int.from_bytes(data[4:8], "little") == len(data) - 8 and len(data) % 2 == 0, name
        got, got_plain = vp8_lib.decode_yuv(data), vp8_lib.decode_yuv(plain)
        if got is None or got[0].shape != (h, w) or not all(np.array_equal(g, r) for g, r in zip(got, rec)):
            bad.append((i4, name))
        elif not all(np.array_equal(g, r) for g, r in zip(got, got_plain)):
            bad.append((i4, name, "differs from the non-adaptive file's decode"))
        assert vp8_lib.features(data) == (w, h, a is not None), name
        if a is not None:
            rgba = vp8_lib.decode_rgba(data)
            assert data[12:16] == b"VP8X" and rgba is not None and np.array_equal(rgba[..., 3], a), name
    assert not bad, bad


def _y2_context_through_b_pred(stats):
    """Is there a coded I16 macroblock whose Y2 block takes a context of 1 that a B_PRED neighbour passed on from beyond it?"""
    is4, skip, nz = stats["is4"], stats["skip"], stats["nz"]
    mbh, mbw = is4.shape
    top = [0] * mbw
    for y in range(mbh):
        left = 0
        for x in range(mbw):
            if is4[y, x]:
                continue  # passes `left` and top[x] on untouched
            through_left = x > 0 and bool(is4[y, x - 1]) and left == 1
            through_top = y > 0 and bool(is4[y - 1, x]) and top[x] == 1
            if not skip[y, x] and (through_left or through_top):
                return True
            left = top[x] = 0 if skip[y, x] else int(nz[y, x, 24])
    return False


def test_the_corpus_reaches_the_paths_it_is_there_for(cases):
    stats = {k: c[7] for k, c in cases.items()}
    assert {tuple(c[0].shape[::-1]) for (i4, _), c in cases.items() if not i4} >= set(vp8_cases.SIZES) | {(300, 200)}
    assert {tuple(c[0].shape[::-1]) for (i4, _), c in cases.items() if i4} >= set(vp8_i4_cases.SIZES) | {(300, 200)}
    # updates in all four block types (type 3 only where a macroblock is B_PRED), and in one picture at once
    types = {i4: set() for i4 in VARIANTS}
    for (i4, name), s in stats.items():
        types[i4] |= {i // (8 * 3 * 11) for i in s["updated"]}
    assert types[False] == {0, 1, 2} and types[True] == {0, 1, 2, 3}
    assert {i // 264 for i in stats[(True, "noise_16x64_q99")]["updated"]} == {0, 1, 2, 3}
    # a node that only saw zeros goes to 255, one that (nearly) only saw ones to 1
    to255 = [(k, i) for k, s in stats.items() for i in s["updated"] if s["probs"][i] == 255]
    to1 = [(k, i) for k, s in stats.items() for i in s["updated"] if s["probs"][i] == 1]
    assert to255 and to1
    assert any(stats[k]["o"][i] == 0 and stats[k]["z"][i] > 0 for k, i in to255) and any(stats[k]["z"][i] == 0 for k, i in to1)
    # pictures without any update: byte-identical to the non-adaptive front end's; one of them has coded macroblocks
    for key in ((False, "flat_64x48_q75"), (True, "flat_48x48_q75"), (False, "photo_1x1_q1"), (True, "edges0_48x48_q1")):
        assert not stats[key]["updated"] and cases[key][5] == cases[key][8], key
    assert not stats[(True, "edges0_48x48_q1")]["skip"].all() and sum(stats[(True, "edges0_48x48_q1")]["z"]) > 0
    # every other picture has an update, and its file differs
    assert all((c[5] == c[8]) == (not c[7]["updated"]) for c in cases.values())
    # cat-6 nodes are visited (noise at quality 99), 1 / 2 / 4 / 8 partitions, mixed B_PRED / I16 with the Y2 context carried through
    node10 = [i for i in range(ap.N) if i % 11 == 10]
    assert sum(stats[(False, "noise_64x48_q99")]["o"][i] for i in node10) > 0
    assert {vm.partitions(s["mbh"]) for s in stats.values()} == {1, 2, 4, 8}
    assert any(_y2_context_through_b_pred(s) for (i4, _), s in stats.items() if i4)
    assert 0 < stats[(True, "photo_300x200_q75")]["is4"].sum() < 13 * 19


def test_the_sizes(cases):
    """No file grows by more than the rounding of its partitions; the flagship output shrinks at every quality."""
    worst = []
    for (i4, name), (y, u, v, a, q, data, rec, stats, plain) in cases.items():
        nparts = vm.partitions(stats["mbh"])
        print(f"{'I4 ' if i4 else 'I16'} {name}: {len(plain)} -> {len(data)} bytes ({len(data) / len(plain):.3f}), {len(stats['updated'])} updates")
        if len(data) > len(plain) + 1 + nparts:
            worst.append((i4, name, len(plain), len(data)))
    assert not worst, worst
    assert webp_lib.load() is not None
    for i4 in VARIANTS:
        for k, q in enumerate(vp8_cases.QUALITIES):
            y, u, v, a, _, data, rec, stats, plain = cases[(i4, f"photo_300x200_q{q}")]
            ref = webp_lib.encode_planes(y, u, v, q)
            print(f"{'I4 ' if i4 else 'I16'} q={q}: {len(data)} bytes, {len(data) / len(plain):.3f} of the non-adaptive {len(plain)}, {len(data) / len(ref):.3f} of libwebp's {len(ref)}")
            assert len(data) < len(plain), (i4, q)
            assert abs(len(data) / len(plain) - MEASURED_VS_NON_ADAPTIVE[i4][k]) < 0.001, "the record above is stale"
            assert abs(len(data) / len(ref) - MEASURED_VS_LIBWEBP[i4][k]) < 0.001, "the record above is stale"


# ------------------------------------------------------------------------------------------------------- the host twin --

@pytest.mark.parametrize("sanitised", (False, True), ids=("plain", "asan_ubsan"))
def test_the_host_twin_writes_the_models_bytes(cases, tmp_path, sanitised):
    """The kernels' own functions in plain loops, as a program of its own; the second build runs them under ASan + UBSan."""
    exe = vp8_host_twin.build(tmp_path, sanitised)
    bad = []
    for (i4, name), (y, u, v, a, q, data, rec, stats, plain) in cases.items():
        twin = vp8_host_twin.run(exe, tmp_path, y, u, v, a, q, i4=i4, adaptive=True, files=("recon", "stats"))
        blob = twin["stats"]
        counts = np.frombuffer(blob[:8 * ap.N], "<u4")
        if (twin["file"] != data or twin["recon"] != b"".join(p.tobytes() for p in rec)
                or counts[:ap.N].tolist() != stats["z"] or counts[ap.N:].tolist() != stats["o"] or list(blob[8 * ap.N:]) != stats["probs"]):
            bad.append((i4, name))
    assert not bad, bad
