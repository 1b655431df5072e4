"""Host half of the lossy WebP decode front end (csrc/fl_vp8src.cpp) and the host twin of its device half (tests/vp8_src_host.cpp:
the functions of csrc/fl_vp8dec_core.h in plain loops).  No GPU.  Host half plus twin must give exactly the planes and the pixels
libwebp decodes -- the model's own reconstruction for the model's files -- for the whole corpus of tests/vp8_src_cases.py; the
corpus itself is held to the coverage the decoder's tests rely on, read from flgpu_vp8_info_of's fields: every branch of the
arithmetic, and every size at which the device's scheduling (csrc/fl_vp8dec.hip) starts a second chunk, round or band."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import vp8_dec_lib
import vp8_src_cases as cases
import vp8l_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
needs_libwebp = pytest.mark.skipif(not cases.have_libwebp(), reason="libwebp cannot be loaded")
CASES = [pytest.param(n, marks=needs_libwebp) if n in cases.LIBWEBP else n for n in cases.names()]


def status_of(fl, fn, *args):
    try:
        fn(*args)
    except fl.FanlinError as e:
        return e.status
    return fl.OK


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vp8twin") / "vp8_src_host")
    subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "vp8_src_host.cpp"),
                    os.path.join(CSRC, "fl_vp8src.cpp"), os.path.join(CSRC, "fl_webpsrc.cpp"), "-o", exe], check=True)

    def run(data, tmp_path, green=None):
        src, out = str(tmp_path / "in.webp"), str(tmp_path / "out.bin")
        open(src, "wb").write(data)
        extra = []
        if green is not None:
            extra = [str(tmp_path / "green.bin")]
            green.tofile(extra[0])
        r = subprocess.run([exe, src, out] + extra, capture_output=True, text=True)
        if r.returncode:
            return r.returncode, None
        w, h, c, mbw, mbh, blob_bytes = map(int, r.stdout.split())
        raw = np.fromfile(out, np.uint8)
        n = mbw * mbh * 384

        def planes(b):
            return (b[:mbw * mbh * 256].reshape(mbh * 16, mbw * 16)[:h, :w], b[mbw * mbh * 256:mbw * mbh * 320].reshape(mbh * 8, mbw * 8)[:(h + 1) // 2, :(w + 1) // 2],
                    b[mbw * mbh * 320:n].reshape(mbh * 8, mbw * 8)[:(h + 1) // 2, :(w + 1) // 2])
        return 0, dict(unfiltered=planes(raw[:n]), filtered=planes(raw[n:2 * n]), pixels=raw[2 * n:].reshape(h, w, c), blob_bytes=blob_bytes)
    return run


# ---- the host half and the twin are exact -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_host_half_and_twin_give_the_expected_planes_and_pixels(fl, twin, tmp_path, name):
    c = cases.get(name)
    info = fl.vp8_info(c["data"])
    h, w = c["yuv"][0].shape
    assert (info["width"], info["height"], info["channels"], info["supported"], info["animated"]) == (w, h, c["channels"], 1, 0)
    blob = fl.debug_vp8_blob(c["data"])
    green = None
    if info["alpha_compression"] == 1:   # the lossless blob behind the levels: its numpy inverse stands in for the lossless decoder's kernels
        at = int.from_bytes(blob[44:48], "little")
        lossless = blob[at:at + vp8l_write.blob_header(blob[at:])["total_bytes"]]
        assert int.from_bytes(blob[28:32], "little") == 2 and len(blob) - at - len(lossless) < 16
        green = np.ascontiguousarray(vp8l_write.inverse(lossless)[..., 1])
    rc, got = twin(c["data"], tmp_path, green)
    assert rc == 0
    assert got["blob_bytes"] == info["blob_bytes"] == len(blob) == int.from_bytes(blob[48:52], "little")
    assert blob[:4] == b"VP81" and int.from_bytes(blob[4:8], "little") == w and int.from_bytes(blob[12:16], "little") == c["channels"]
    for k, plane in enumerate("YUV"):
        assert np.array_equal(got["filtered"][k], c["yuv"][k]), f"{plane} plane differs"
        if info["filter_level"] == 0:
            assert np.array_equal(got["unfiltered"][k], c["yuv"][k]), f"{plane} plane differs before the loop filter"
    if info["filter_level"] >= 14 and info["macroblocks"] > 1:   # (at the low levels the filter finds nothing to do in the noisy pictures)
        assert any(not np.array_equal(a, b) for a, b in zip(got["filtered"], got["unfiltered"])), "the loop filter changed nothing"
    if c["pixels"] is not None:
        assert np.array_equal(got["pixels"], c["pixels"]), "pixels differ from WebPDecodeRGB / WebPDecodeRGBA"
    if c["channels"] == 4 and name in cases.MODEL:
        assert np.array_equal(got["pixels"][..., 3], c["alpha"]), "the alpha plane is not the one the file was written from"
    if name in cases.MODEL and cases.have_libwebp():   # the model's files are valid for libwebp too, and it agrees with the model
        for a, b in zip(vp8_dec_lib.decode_yuv(c["data"]), c["yuv"]):
            assert np.array_equal(a, b)


# ---- flgpu_vp8_info_of ------------------------------------------------------------------------------------------------------------------

def test_info_fields_of_the_model_files(fl):
    for n, parts in ((16, 1), (32, 2), (64, 4), (128, 8)):
        info = fl.vp8_info(cases.get(f"model_partitions{parts}")["data"])
        assert (info["partitions"], info["macroblocks"], info["version"], info["filter_level"], info["segmentation"]) == (parts, n // 16, 0, 0, 0)
        assert info["bpred_macroblocks"] == 0 and info["coef_prob_updates"] == 0 and info["extended"] == 0
    for name in cases.MODEL:
        c = cases.get(name)
        info = fl.vp8_info(c["data"])
        assert info["ymodes_mask"] == sum(1 << m for m in c["stats"]["ymodes"]) and info["uvmodes_mask"] == sum(1 << m for m in c["stats"]["uvmodes"]), name
        assert info["skipped_macroblocks"] == c["stats"]["skipped"] and (info["cat6_tokens"] > 0) == c["stats"]["cat6"], name
        assert info["has_alpha"] == info["extended"] == int(c["channels"] == 4), name
    for m in (1, 2, 3):
        info = fl.vp8_info(cases.get(f"model_alpha_filter{m}")["data"])
        assert (info["alpha_compression"], info["alpha_filter"], info["channels"]) == (0, m, 4)
    data = cases.extended(cases.get("model_48x32")["data"], 6)
    info = fl.vp8_info(data)
    assert (info["extended"], info["exif_orientation"], info["has_alpha"], info["channels"], info["supported"]) == (1, 6, 0, 3, 1)
    assert fl.vp8_info(cases.extended(cases.get("model_48x32")["data"]))["exif_orientation"] == 0


@needs_libwebp
def test_info_fields_of_libwebp_files(fl):
    info = {n: fl.vp8_info(cases.get(n)["data"]) for n in cases.LIBWEBP}
    d = info["lib_default"]
    assert (d["segmentation"], d["update_map"], d["filter_type"], d["sharpness"], d["version"]) == (1, 1, 0, 0, 0) and 0 < d["filter_level"] < 15
    assert 15 <= info["lib_quality20"]["filter_level"] < 40 <= info["lib_quality5"]["filter_level"]
    assert info["lib_skips"]["skipped_macroblocks"] and not info["lib_skips"]["skipped_bpred_macroblocks"] and info["lib_skips_bpred"]["skipped_bpred_macroblocks"]
    assert (info["lib_simple_filter"]["filter_type"], info["lib_simple_filter"]["version"]) == (1, 1)
    assert info["lib_sharpness5"]["sharpness"] == 5
    assert (info["lib_strength0"]["filter_level"], info["lib_strength0"]["version"]) == (0, 2)
    assert info["lib_segments1"]["segmentation"] == 0 and info["lib_segments1"]["segment_quantizers"] == 1
    assert (info["lib_alpha_raw"]["alpha_compression"], info["lib_alpha_raw"]["channels"], info["lib_alpha_raw"]["has_alpha"]) == (0, 4, 1)
    c = info["lib_alpha_compressed"]
    assert (c["alpha_compression"], c["supported"], c["channels"], c["has_alpha"]) == (1, 1, 4, 1) and c["macroblocks"] == 12
    assert all(len(cases.get(n)["data"]) < 4096 for n in cases.LIBWEBP if "x" not in n and "bars" not in n and "skips" not in n)


@needs_libwebp
def test_the_corpus_covers_what_the_decoder_has(fl):
    """A condition on the corpus, not a measurement: every branch of the decoder is reached by a file whose decode is checked."""
    infos = {n: fl.vp8_info(cases.get(n)["data"]) for n in cases.names()}
    union = lambda k: sum(1 << b for b in range(16) if any(i[k] >> b & 1 for i in infos.values()))  # noqa: E731
    assert union("bmodes_mask") == 0x3ff and union("ymodes_mask") == 15 and union("uvmodes_mask") == 15
    assert any(0 < i["bpred_macroblocks"] < i["macroblocks"] for i in infos.values()), "B_PRED and one-mode macroblocks in one file"
    assert any(i["skipped_bpred_macroblocks"] and i["filter_level"] for i in infos.values()), "a skipped macroblock with filtered inner edges"
    assert any(i["skipped_macroblocks"] > i["skipped_bpred_macroblocks"] and i["filter_level"] for i in infos.values()), "... and without"
    assert any(i["segment_quantizers"] > 1 and i["segment_filter_levels"] > 1 for i in infos.values())
    assert {0, 1} <= {i["filter_type"] for i in infos.values() if i["filter_level"]}
    assert any(i["sharpness"] == 0 and i["filter_level"] for i in infos.values()) and any(i["sharpness"] > 0 and i["filter_level"] for i in infos.values())
    levels = {i["filter_level"] for i in infos.values()}
    assert any(0 < l < 15 for l in levels) and any(15 <= l < 40 for l in levels) and any(l >= 40 for l in levels), levels
    assert any(i["coef_prob_updates"] for i in infos.values()) and any(i["cat6_tokens"] for i in infos.values())
    assert {i["partitions"] for i in infos.values()} == {1, 2, 4, 8}
    assert {(i["alpha_compression"], i["alpha_filter"]) for i in infos.values() if i["channels"] == 4} >= {(0, 0), (0, 1), (0, 2), (0, 3)}
    assert {i["alpha_compression"] for i in infos.values() if i["channels"] == 4} == {0, 1}   # both decoded, both checked against WebPDecodeRGBA


def fullest_diagonal(mbw, mbh):
    """the most macroblocks on one anti-diagonal d = x + 2 y (diagonal() of csrc/fl_vp8dec.hip)"""
    def count(d):
        lo = (d - mbw + 2) >> 1 if d >= mbw else 0
        return max(min(mbh - 1, d >> 1) - lo + 1, 0)
    return max(count(d) for d in range(mbw + 2 * (mbh - 1)))


@needs_libwebp
def test_the_corpus_reaches_every_seam_of_the_device_schedule(fl):
    """A condition on the corpus, like the one above, for what only csrc/fl_vp8dec.hip knows: how lanes, waves, rounds and bands
    share a picture.  Every place where that scheduling has a second iteration is reached by a file whose decode is checked.  The
    sizes are restated here and compared with the headers: whoever retunes the kernels moves the corpus with them."""
    WAVES, LANES, THREADS, FILTER_SLOTS = 16, 64, 1024, 32
    h_text, core_text = open(os.path.join(CSRC, "fl_vp8dec.h")).read(), open(os.path.join(CSRC, "fl_vp8dec_core.h")).read()
    waves, per_wave = map(int, re.search(r"constexpr uint32_t kVp8dWaves = (\d+), kVp8dThreads = kVp8dWaves \* (\d+)u;", h_text).groups())
    lanes = int(re.search(r"\bkVp8dLanes = (\d+)\b", core_text).group(1))
    filter_lanes = int(re.search(r"\bkVp8dFilterLanes = (\d+)\b", core_text).group(1))
    assert (waves, lanes, per_wave, waves * per_wave, waves * per_wave // filter_lanes) == (WAVES, LANES, LANES, THREADS, FILTER_SLOTS), \
        "the kernels' shape changed: move the sizes of cases.SCHEDULING with it"
    assert fullest_diagonal(35, 18) == 18 and fullest_diagonal(65, 33) == 33 and fullest_diagonal(1, 1) == 1

    infos = {n: fl.vp8_info(cases.get(n)["data"]) for n in cases.names()}
    assert set(cases.SCHEDULING) <= set(infos) and len(cases.SCHEDULING) == 26

    # -- rounds of vp8dec_recon_kernel (WAVES macroblocks each) and vp8dec_filter_kernel (FILTER_SLOTS each)
    def rounds(i):
        mbw, mbh = (i["width"] + 15) // 16, (i["height"] + 15) // 16
        assert mbw * mbh == i["macroblocks"]
        return fullest_diagonal(mbw, mbh)
    mixed = {n: (rounds(i), i["filter_type"]) for n, i in infos.items() if i["filter_level"] and 0 < i["bpred_macroblocks"] < i["macroblocks"]}
    for filter_type, what in ((0, "normal"), (1, "simple")):
        fullest = {f for f, t in mixed.values() if t == filter_type}
        assert any(f > 2 * WAVES for f in fullest), f"no third reconstruction round under the {what} filter"
        assert any(f % FILTER_SLOTS == 1 and f > FILTER_SLOTS for f in fullest), f"no second filter round with one slot active under the {what} filter"
    assert any(f == FILTER_SLOTS and f % WAVES == 0 for f, t in mixed.values()), "no file whose fullest diagonal is whole rounds only"
    for n in ("lib_rounds_1040x528", "lib_rounds_simple_1040x528", "lib_rounds_1040x512"):
        assert n in mixed, f"{n}: B_PRED and one-mode macroblocks together behind a loop filter"
        # ... and together in every round of the fullest diagonals but a one-wave one (Vp8MbRecord::ymode: csrc/fl_vp8src.h), so
        # the rounds behind the first take the sixteen sub-steps with one-step waves waiting beside sixteen-step ones
        blob = fl.debug_vp8_blob(cases.get(n)["data"])
        mbw, mbh, rec_off = (int.from_bytes(blob[k:k + 4], "little") for k in (16, 20, 36))
        ymode = np.frombuffer(blob, np.uint8, mbw * mbh * 48, rec_off).reshape(mbh, mbw, 48)[..., 4]
        for d in range(mbw + 2 * (mbh - 1)):
            ys = [y for y in range(mbh) if 0 <= d - 2 * y < mbw]
            if len(ys) == mixed[n][0]:
                for base in range(0, len(ys), WAVES):
                    kinds = {int(ymode[y, d - 2 * y]) == 4 for y in ys[base:base + WAVES]}
                    assert kinds == {False, True} or len(ys) - base == 1, (n, d, base)
    assert infos["lib_rounds_1040x528"]["segmentation"] == 1 and infos["lib_rounds_1040x528"]["update_map"] == 1

    # -- vp8dec_alpha_kernel: (compression, filter) -> the sizes it is decoded at; compression 0 is read at stride 1, 1 at stride 4
    sizes = {}
    for i in infos.values():
        if i["channels"] == 4:
            sizes.setdefault((i["alpha_compression"], i["alpha_filter"]), set()).add((i["width"], i["height"]))

    def reached(compression, method, seam, what):
        assert any(seam(w, h) for w, h in sizes.get((compression, method), ())), f"ALPH compression {compression}, filter {method}: {what}"
    for m in (1, 2, 3):   # stride 1: each filter at every seam
        reached(0, m, lambda w, h: w == LANES and h > 1, "a row of exactly one chunk")
        reached(0, m, lambda w, h: w == LANES + 1 and h > 1, "a row one sample into the second chunk")
        reached(0, m, lambda w, h: w > 2 * LANES and w % LANES and h > WAVES, "three chunks with a ragged end, more rows than waves")
        reached(0, m, lambda w, h: h > THREADS + 1 and w > 1, "a second gradient band behind a row; 17 passes of the column sum; columns longer than a band")
        reached(0, m, lambda w, h: w > THREADS and h > 1, "columns beyond the last thread; more chunks than waves")
    reached(0, 0, lambda w, h: w * h > THREADS, "a second pass of the copy loop")
    for m in (0, 1, 2, 3):   # stride 4: every filter past a chunk and past the waves
        reached(1, m, lambda w, h: w > LANES and w % LANES and h > WAVES, "several chunks a row, more rows than waves")
    reached(1, 3, lambda w, h: h > THREADS + 1 and w > LANES, "a second gradient band")
    for m in (1, 2):
        reached(1, m, lambda w, h: w > THREADS and h > 1, "columns beyond the last thread; more chunks than waves")


# ---- damaged and refused files ---------------------------------------------------------------------------------------------------------

def resized(data):
    """RIFF and VP8 chunk sizes repaired after bytes were cut from the end of a simple-format file"""
    data = data + (b"\0" if len(data) & 1 else b"")
    return data[:4] + (len(data) - 8).to_bytes(4, "little") + data[8:16] + (len(data) - 20).to_bytes(4, "little") + data[20:]


def damaged():
    import vp8l_model
    good = cases.get("model_48x32")["data"]
    multi = cases.get("model_partitions4")["data"]
    tag = int.from_bytes(good[20:23], "little")
    part0 = tag >> 5
    table = 20 + 10 + (int.from_bytes(multi[20:23], "little") >> 5)
    ext = cases.extended(good)
    translucent = cases.get("model_alpha_raw")["data"]
    at = translucent.index(b"ALPH")

    def alph(bits, cut=False):
        """the ALPH chunk's first byte with `bits` set; cut: the chunk announces one byte fewer (its last byte becomes the padding)"""
        d = translucent[:at + 8] + bytes([translucent[at + 8] | bits]) + translucent[at + 9:]
        size = int.from_bytes(d[at + 4:at + 8], "little")
        return d[:at + 4] + (size - 1).to_bytes(4, "little") + d[at + 8:] if cut else d
    return {
        "first partition cut short": good[:20] + ((tag & 31) | 40 << 5).to_bytes(3, "little") + good[23:],
        "first partition longer than the file": good[:20] + ((tag & 31) | 0x7ffff << 5).to_bytes(3, "little") + good[23:],
        "file ends inside the first partition": resized(good[:30 + part0 // 2]),
        "file ends inside the token partition": resized(good[:30 + part0 + 4]),
        "file ends inside the last token partition": resized(multi[:len(multi) - 40]),
        "partition table points outside the file": multi[:table] + b"\xff\xff\xff" + multi[table + 3:],
        "inter frame": good[:20] + bytes([good[20] | 1]) + good[21:],
        "hidden frame": good[:20] + bytes([good[20] & ~16]) + good[21:],
        "start code": good[:23] + b"\x9d\x01\x2b" + good[26:],
        "width 0": good[:26] + b"\0\0" + good[28:],
        "height 0": good[:28] + b"\0\0" + good[30:],
        "canvas disagrees with the frame": ext[:24] + (99).to_bytes(3, "little") + ext[27:],   # VP8X canvas 100 wide, the frame 48
        "ALPH pre-processing 2": alph(0x20),
        "ALPH reserved field 2": alph(0x80),
        "ALPH compression 2": alph(0x02),
        "ALPH raw plane one byte short": alph(0, cut=True),
        "RIFF size": good[:4] + (len(good) - 6).to_bytes(4, "little") + good[8:],
        "a lossless file": vp8l_model.encode(np.zeros((4, 4, 4), np.uint8)),
    }


def test_damaged_files_are_parse_errors_and_the_thread_goes_on(fl, twin, tmp_path):
    good = cases.get("model_48x32")
    for what, data in damaged().items():
        assert status_of(fl, fl.vp8_info, data) == fl.ERR_PARSE, what
        assert twin(data, tmp_path)[0] == 3, what
        if cases.have_libwebp() and what != "a lossless file":
            assert vp8_dec_lib.decode_pixels(data, 4 if b"ALPH" in data[:64] else 3) is None, f"libwebp decodes the file with: {what}"
        assert fl.vp8_info(good["data"])["supported"] == 1   # the next call is served


def test_animated_and_refused_files_are_unsupported(fl, twin, tmp_path):
    good = cases.extended(cases.get("model_48x32")["data"])
    animated = good[:20] + bytes([good[20] | 2]) + good[21:]
    info = fl.vp8_info(animated)
    assert (info["animated"], info["supported"], info["channels"]) == (1, 0, 0)
    assert twin(animated, tmp_path)[0] == 4
    # the frame-header features no corpus file vouches for, each set alone by a test-side writer: refused, whatever follows the header
    for feature in cases.REFUSED_FEATURES:
        data = cases.refused_file(feature)
        info = fl.vp8_info(data)
        assert (info["width"], info["height"], info["supported"], info["channels"], info["macroblocks"]) == (16, 16, 0, 0, 0), feature
        assert twin(data, tmp_path)[0] == 4, feature
        plan, kind = fl.flgpu_plan(), ctypes.c_int()
        assert fl.load_library().flgpu_process_webp_plan(data, len(data), b"w=30&h=20", 0, ctypes.byref(plan), ctypes.byref(kind)) == fl.ERR_UNSUPPORTED, feature


# ---- robustness ----------------------------------------------------------------------------------------------------------------------------

def test_mutated_files_under_address_and_ub_sanitizers(fl, tmp_path):
    """tests/vp8_src_fuzz.cpp + csrc/fl_vp8src.cpp as one program with -fsanitize=address,undefined, run as a child process:
    2,000 seeded mutants per corpus file.  Never through Python's process."""
    exe = str(tmp_path / "vp8_src_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "vp8_src_fuzz.cpp"), os.path.join(CSRC, "fl_vp8src.cpp"), os.path.join(CSRC, "fl_webpsrc.cpp"), "-o", exe], check=True)
    paths = []
    for name in cases.names(libwebp_too=cases.have_libwebp()):
        if name in ("lib_560x288", "lib_300x200") or name in cases.SCHEDULING:
            continue   # (the large ones, and the sizes chosen for the device's scheduling: the same code paths, ten times the time)
        p = str(tmp_path / (name + ".webp"))
        open(p, "wb").write(cases.get(name)["data"])
        paths.append(p)
    r = subprocess.run([exe, "2000"] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("intact=ok") == len(paths)
    assert sum(int(m) for m in re.findall(r"refused=(\d+)", r.stdout)) > 0


def test_host_half_compiles_as_plain_cpp():
    for flags in (["-std=c++17"], ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"]):
        subprocess.run(["g++", *flags, "-fsyntax-only", os.path.join(CSRC, "fl_vp8src.cpp"), os.path.join(CSRC, "fl_webpsrc.cpp")], check=True)
    text = open(os.path.join(CSRC, "fl_vp8src.cpp")).read() + open(os.path.join(CSRC, "fl_vp8src.h")).read()
    assert "#include <hip" not in text and "__global__" not in text
    assert "malloc" not in text and "std::vector" not in text and " new " not in text   # nothing is allocated while decoding


# ---- bindings ------------------------------------------------------------------------------------------------------------------------------

def test_bindings_know_the_new_names(fl, tmp_path):
    header = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    shim = open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    assert int(re.search(r"#define FLGPU_IMG_VP8_SOURCE\s+(\d+)u", header).group(1)) == fl.IMG_VP8_SOURCE == 128
    assert int(re.search(r"const IMG_VP8_SOURCE: u32 = (\d+);", shim).group(1)) == 128
    flags = {int(v) for v in re.findall(r"#define FLGPU_IMG_\w+\s+(\d+)u", header)}
    assert len(flags) == len(re.findall(r"#define FLGPU_IMG_\w+\s+(\d+)u", header)), "the bit was not free"
    fields = re.search(r"typedef struct flgpu_vp8_info \{(.*?)\} flgpu_vp8_info;", header, re.S).group(1)
    names = re.findall(r"uint32_t (\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", fields, flags=re.S).replace("width, height", "width; uint32_t height"))
    assert names == [n for n, _ in fl.flgpu_vp8_info._fields_]
    assert ctypes.sizeof(fl.flgpu_vp8_info) == 128
    block = re.search(r"pub struct FlVp8Info \{(.*?)\}", shim, re.S).group(1)
    assert re.findall(r"pub (\w+): ", block) == names
    assert {"flgpu_vp8_info_of"} <= set(re.findall(r"fn (flgpu_\w+)\(", shim)) and "pub fn vp8_info(" in shim
    assert "flgpu_vp8_info_of" in hpp and "decode_webp_lossy(" in hpp
    lib = fl.load_library()
    for sym in ("flgpu_vp8_info_of", "flgpu_decode_webp_lossy", "flgpu_debug_vp8_planes", "flgpu_debug_vp8_blob"):
        assert hasattr(lib, sym) and sym in fl.EXPORTED_SYMBOLS
    assert lib.flgpu_abi_version() == 6
    src = tmp_path / "size.cpp"
    src.write_text('#include "fanlin_gpu.hpp"\nstatic_assert(sizeof(flgpu_vp8_info) == 128, "flgpu_vp8_info is 32 u32");\n'
                   'static_assert(FLGPU_IMG_VP8_SOURCE == 128u, "flag value");\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_process_webp_plan_takes_a_lossy_file_without_a_device(fl):
    C = ctypes
    lib = fl.load_library()
    data = cases.extended(cases.get("model_48x32")["data"], 6)
    plan, kind = fl.flgpu_plan(), C.c_int()
    assert lib.flgpu_process_webp_plan(data, len(data), b"w=30&h=20", 0, C.byref(plan), C.byref(kind)) == fl.OK
    assert kind.value != fl.RESULT_AS_IS and plan.max_out_bytes > 0
    assert lib.flgpu_process_webp_plan(data, len(data), b"", 0, C.byref(plan), C.byref(kind)) == fl.OK and kind.value == fl.RESULT_AS_IS
    assert lib.flgpu_process_webp_plan(data[:30], 30, b"w=30&h=20", 0, C.byref(plan), C.byref(kind)) == fl.ERR_PARSE
    animated = data[:20] + bytes([data[20] | 2]) + data[21:]
    assert lib.flgpu_process_webp_plan(animated, len(animated), b"w=30&h=20", 0, C.byref(plan), C.byref(kind)) == fl.ERR_UNSUPPORTED
