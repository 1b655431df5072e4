"""FLGPU_FEO_ALPHA_VP8L / FLGPU_ENCODE_WEBP_LOSSY_ALPHA, the host half: the constants and the unchanged struct, the mapping of the accept
bit, and the restated ALPH chunk (tests/vp8_alpha_model.py) judged by libwebp's decoder on the alpha corpus
(tests/vp8_alpha_cases.py): every file decodes to exactly the plane and to the Y, U, V of its raw-alpha twin, the payload begins
with 0x01 exactly where the rule says, no file is longer than its twin, and every branch of the rule occurs.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import vp8_alpha_cases as cases_mod
import vp8_alpha_model as am
import vp8_cases
import vp8_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (30, 75)


# ----------------------------------------------------------------------------------------------------------- the ABI --

def test_the_constants_and_the_unchanged_struct(fl, tmp_path):
    assert fl.ENCODE_WEBP_LOSSY_ALPHA == 0x20000 and fl.FEO_ALPHA_VP8L == 1 and fl.load_library().flgpu_abi_version() == 6
    assert C.sizeof(fl.flgpu_params) == 28 and fl.flgpu_params.reserved.offset == 26 and fl.flgpu_params.reserved.size == 2
    assert not any(fl.ENCODE_WEBP_LOSSY_ALPHA & b for b in (fl.ACCEPT_WEBP, fl.ACCEPT_AVIF, fl.ENCODE_PNG, fl.DECODE_PNG_ADAM7, fl.ENCODE_WEBP_LOSSLESS,
                                                            fl.ENCODE_GIF, fl.ENCODE_GIF_QUANTIZE, fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4,
                                                            fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER))
    p = fl.make_params(quality=75, front_end=fl.FE_WEBP_LOSSY)
    assert tuple(p.reserved) == (0, 0) and tuple(fl.make_params(alpha_vp8l=True).reserved) == (1, 0)
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert "#define FLGPU_ENCODE_WEBP_LOSSY_ALPHA 0x20000u" in header and "#define FLGPU_FEO_ALPHA_VP8L 1u" in header
    assert "#define FLGPU_ABI_VERSION 6" in header and "uint8_t options;" in header
    assert "encode_webp_lossy_alpha()" in open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    shim = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    assert "ENCODE_WEBP_LOSSY_ALPHA: u32 = 0x20000" in shim and "FEO_ALPHA_VP8L: u8 = 1" in shim
    # the C compiler's view of the struct: the options byte is the first of the two that were reserved
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fanlin_gpu.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(flgpu_params), '
                   'offsetof(flgpu_params, filter), offsetof(flgpu_params, options), offsetof(flgpu_params, reserved)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["28", "25", "26", "27"]


def _plan(fl, query, flags, fmt, w=1920, h=1080, c=4):
    lib = fl.load_library()
    img = fl.flgpu_image(None, w * h * c, w, h, c, 0)
    plan, k = fl.flgpu_plan(), C.c_int(-1)
    rc = lib.flgpu_process_image_plan(C.byref(img), 1, query.encode(), flags, fmt, C.byref(plan), C.byref(k))
    return rc, k.value, (plan.out_w, plan.out_h, plan.out_c, plan.out_bytes, plan.max_out_bytes)


def test_the_mapping_of_every_combination_of_the_lossy_bits(fl):
    """flgpu_params_from_query sets the option iff the WebP arm runs below quality 100 and both ENCODE_WEBP_LOSSY and the new bit are
    there; nothing else of the parameters moves, and neither does any plan: the option changes no size, no bound and no kind."""
    bits = (fl.ENCODE_WEBP_LOSSLESS, fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_I4, fl.ENCODE_WEBP_LOSSY_PROBS, fl.ENCODE_WEBP_LOSSY_FILTER)
    new = fl.ENCODE_WEBP_LOSSY_ALPHA

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
                want = 1 if lossy_arm and accept and flags & fl.ENCODE_WEBP_LOSSY else 0
                assert tuple(without.reserved) == (0, 0) and tuple(with_bit.reserved) == (want, 0), (query, hex(flags))
                assert fields(without) == fields(with_bit) and fmt0 == fmt1, (query, hex(flags))
                if want:
                    assert with_bit.front_end == fl.FE_WEBP420  # (the caller, or flgpu_process_*, puts the lossy front end in its place)
                for fmt in (fl.IN_PNG, fl.IN_JPEG, fl.IN_WEBP):
                    assert _plan(fl, query, flags, fmt) == _plan(fl, query, flags | new, fmt), (query, hex(flags), fmt)
    # the bit alone, and with every other lossy bit but ENCODE_WEBP_LOSSY: the planes, as without it
    for extra in (0, fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS | fl.ENCODE_WEBP_LOSSY_FILTER):
        rc, kind, plan = _plan(fl, "w=300&h=200&webp=true&quality=75", fl.ACCEPT_WEBP | new | extra, fl.IN_PNG)
        assert rc == fl.OK and kind == fl.RESULT_WEBP_PLANES
        assert tuple(fl.Query.parse("w=300&h=200&webp=true&quality=75").to_params(fl.Format(fl.ACCEPT_WEBP | new | extra))[0].reserved) == (0, 0)
    assert _plan(fl, "w=300&h=200&webp=true&quality=75", fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | new, fl.IN_PNG)[1] == fl.RESULT_WEBP_STREAM
    # the option changes no plan of any front end: the file is never larger than with the raw plane
    for fe in fl.FE_WEBP_LOSSY_ALL + (fl.FE_WEBP_LOSSLESS, fl.FE_JPEG, fl.FE_PNG, fl.FE_WEBP420, fl.FE_NONE):
        a = fl.plan_output(fl.make_params(quality=75, front_end=fe), 300, 200, 4)
        b = fl.plan_output(fl.make_params(quality=75, front_end=fe, alpha_vp8l=True), 300, 200, 4)
        assert bytes(a) == bytes(b), fe


# ---------------------------------------------------------------------------------------------------------- the model --

def test_the_stream_on_paper():
    import vp8l_model as ll
    # one literal and one run: the headers, a two-symbol green code, 0-bit red, blue, alpha and distance codes
    st = {}
    s = am.alpha_stream(np.zeros((17, 17), np.uint8), st)
    assert st == dict(literals=1, refs=1, longest=288, header_bits=396, green_symbols=2) and len(s) == 51
    # the first 37 bits: predictor transform with 2^9 blocks, its sub-image (no cache; green 2 as an 8-bit simple code, four 1-bit ones), no
    # further transform, no colour cache, no meta codes -- and no VP8L signature in front
    br = ll.BitReader(s)
    assert (br.get(1), br.get(2), br.get(3), br.get(1)) == (1, 0, 7, 0)
    assert (br.get(1), br.get(1), br.get(1), br.get(8)) == (1, 0, 1, 2)
    assert [br.get(4) for _ in range(4)] == [0b0001] * 4 and br.get(3) == 0 and s[0] != 0x2F
    # runs longer than 4096 are cut by a literal; a run crosses the row edge (T on column 0) and the tile edge
    st = {}
    am.alpha_stream(dict((n, a) for n, a, _ in cases_mod.planes())["runs_4097x2"], st)
    assert st["literals"] == 4 and st["refs"] == 3 and st["longest"] == 4096
    # the rule: strictly smaller, a tie goes to raw
    planes = dict((n, a) for n, a, _ in cases_mod.planes())
    under, tie = planes["under_64x48"], planes["tie_64x48"]
    assert len(am.alpha_stream(under)) == under.size - 1 and am.alph_payload(under)[0] == 1 and len(am.alph_payload(under)) == under.size
    assert len(am.alpha_stream(tie)) == tie.size and am.alph_payload(tie) == b"\0" + tie.tobytes()
    assert am.alph_payload(np.full((1, 1), 7, np.uint8)) == b"\0\x07"


@pytest.fixture(scope="module")
def files(oracle):
    """(name, quality) -> (plane or None, branch, the vp8_model file, the file with the option)"""
    out = {}
    for name, img, _, branch in cases_mod.corpus():
        y, u, v, has_alpha = oracle.webp_yuv420(img)
        assert has_alpha == (branch != "opaque"), name
        a = np.ascontiguousarray(img[..., 3]) if has_alpha else None
        for q in QUALITIES:
            twin = vp8_cases.model(f"alpha:{name}:{q}", y, u, v, q, a)[0]
            out[(name, q)] = (a, branch, twin, am.with_alpha(twin, a) if has_alpha else am.with_alpha(twin, img[..., 3]))
    return out


def test_the_rule_takes_the_branch_and_the_size_the_corpus_names(files):
    seen = set()
    for (name, q), (a, branch, twin, data) in files.items():
        payload = am.alph_of(data)
        assert len(data) <= len(twin) and len(data) % 2 == 0 and int.from_bytes(data[4:8], "little") == len(data) - 8, name
        assert [t for t, _ in am.chunks(data)] == [t for t, _ in am.chunks(twin)], name
        assert [c for c in am.chunks(data) if c[0] != b"ALPH"] == [c for c in am.chunks(twin) if c[0] != b"ALPH"], name
        if branch == "opaque":
            assert payload is None and data == twin and data[12:16] == b"VP8 ", name
        else:
            stream = am.alpha_stream(a)
            compressed = 1 + len(stream) < 1 + a.size
            assert branch == ("compressed" if compressed else "raw"), (name, len(stream), a.size)
            assert payload == (b"\x01" + stream if compressed else b"\x00" + a.tobytes()) and (payload[0] == 1) == compressed, name
            assert (data == twin) == (not compressed) and (len(data) < len(twin)) == compressed, name
            if name in cases_mod.MEASURED:
                assert len(payload) == cases_mod.MEASURED[name], (name, len(payload))
        seen.add(branch)
    assert seen == {"compressed", "raw", "opaque"}
    assert {n for n, _, _, _ in cases_mod.corpus()} >= {f"ramp_{w}x{h}" for w, h in vp8_cases.SIZES}


def test_libwebp_decodes_every_file_to_the_plane_and_to_the_twins_planes(files):
    if vp8_lib.load() is None:
        pytest.skip("libwebp is needed to judge the files")
    bad = []
    for (name, q), (a, branch, twin, data) in files.items():
        got, want = vp8_lib.decode_yuv(data), vp8_lib.decode_yuv(twin)
        if got is None or not all(np.array_equal(g, r) for g, r in zip(got, want)):
            bad.append((name, q, "yuv"))
            continue
        rgba = vp8_lib.decode_rgba(data)
        h, w = want[0].shape
        assert vp8_lib.features(data) == (w, h, a is not None), name
        if rgba is None or not np.array_equal(rgba[..., 3], a if a is not None else np.full((h, w), 255, np.uint8)):
            bad.append((name, q, "alpha"))
        if not np.array_equal(rgba, vp8_lib.decode_rgba(twin)):
            bad.append((name, q, "rgba"))
    assert not bad, bad
