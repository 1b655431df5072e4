"""The host twin of the PNG inflate kernel (flgpu_debug_png_inflate_model: csrc/fl_inflate_core.h in plain loops over arrays of the
kernel's LDS sizes) against zlib.decompress, on streams zlib writes in every mode and on hand-written ones; broken streams are each a
"no"; constants and ABI; and the twin under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import subprocess
import zlib

import pytest

import png_inflate_cases as pc
import png_write as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")


@pytest.fixture(scope="module")
def results(fl):
    """name -> (scanlines, stats) of the model for the whole valid corpus, computed once"""
    return {name: fl.debug_png_inflate_model(data) for name, data, _ in pc.valid()}


@pytest.mark.parametrize("k", range(len(pc.valid())), ids=[c[0] for c in pc.valid()])
def test_model_equals_zlib(fl, results, k):
    name, data, raw = pc.valid()[k]
    assert zlib.decompress(pw.idat_payload(data)) == raw
    got, stats = results[name]
    assert got == raw, (name, stats)
    assert got == fl.debug_png_scanlines(data)
    assert stats["blocks"] >= 1


def test_the_corpus_reaches_the_synchronisation_and_resolution_loops(results):
    stats = {n: s for n, (_, s) in results.items()}
    assert max(s["max_sync_rounds"] for s in stats.values()) > 1, stats
    assert max(s["max_resolve_rounds"] for s in stats.values()) > 1, stats
    # what the cases were built for
    assert stats["chain-of-3-3-matches"]["max_resolve_rounds"] > 100                       # a chain of dependent matches: one per round
    assert stats["sync-flush-every-100"]["blocks"] > stats["sync-flush-every-100"]["strips"] > 0      # many blocks inside one strip's bits
    assert stats["stored-65535"]["strips"] == 0 and stats["stored-level0-spanning"]["blocks"] == 2
    assert stats["fewer-bits-than-a-subsequence"]["strips"] == 1
    assert stats["eob-in-the-last-subsequence"]["strips"] == 1 and stats["eob-in-the-first-of-the-next-strip"]["strips"] == 2
    assert stats["exactly-one-strip"]["strips"] == 1 and stats["one-strip-minus-a-token"]["strips"] == 1 and stats["one-strip-plus-a-token"]["strips"] == 2
    assert stats["level6-long"]["tokens_again"] > 0                                          # speculation was wrong somewhere and was repaired


@pytest.mark.parametrize("k", range(len(pc.broken())), ids=[c[0] for c in pc.broken()])
def test_broken_streams_are_each_a_no(fl, k):
    name, data = pc.broken()[k]
    assert fl.png_info(data)["supported"] == 1          # the container is intact: the stream is what is wrong
    with pytest.raises(fl.FanlinError) as e:
        fl.debug_png_inflate_model(data)
    assert e.value.status == fl.ERR_PARSE, name
    with pytest.raises(fl.FanlinError):                 # and the host inflate, whose verdict is final, refuses it too
        fl.debug_png_scanlines(data)


def test_pictures_of_every_kind_and_interlaced_ones(fl):
    for k, (ct, depth) in enumerate([(0, 1), (0, 8), (2, 8), (3, 2), (3, 8), (4, 8), (6, 8)]):
        for interlace in (0, 1):
            data, _ = pc.picture(ct, depth, 11, 5, 40 + k, interlace=interlace)
            got, _ = fl.debug_png_inflate_model(data)
            assert got == fl.debug_png_scanlines(data, adam7=bool(interlace)), (ct, depth, interlace)


def test_constants_abi_and_header_text(fl):
    assert fl.IMG_PNG_INFLATE == 512 and fl.DECODE_PNG_INFLATE == 0x100000
    assert fl.load_library().flgpu_abi_version() == 6
    text = open(os.path.join(ROOT, "include", "fanlin_gpu.h")).read()
    assert "#define FLGPU_IMG_PNG_INFLATE     512u" in text and "#define FLGPU_DECODE_PNG_INFLATE 0x100000u" in text
    assert "flgpu_debug_png_inflate_device(flgpu_ctx *ctx, const uint8_t *png, uint64_t n, uint32_t src_flags, uint8_t *out, uint64_t capacity, uint64_t *used)" in text
    assert "flgpu_debug_png_inflate_model(const uint8_t *png, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *used, uint32_t stats[8])" in text
    assert pc.SUB_BITS >= 64 and pc.SUBS == 256
    hpp = open(os.path.join(ROOT, "include", "fanlin_gpu.hpp")).read()
    assert "FLGPU_DECODE_PNG_INFLATE" in hpp
    assert "IMG_PNG_INFLATE: u32 = 512" in open(os.path.join(ROOT, "shim", "handler_gpu.rs")).read()
    assert fl.png_info(pc.valid()[0][1], device_inflate=True) == fl.png_info(pc.valid()[0][1])


def test_mutated_streams_under_address_and_ub_sanitizers(tmp_path):
    """tests/png_inflate_fuzz.cpp + csrc/fl_pngsrc.cpp as one program with -fsanitize=address,undefined, run as a child process: 2,000
    seeded mutations of each file's IDAT payload through the twin; whenever it says yes, the host inflate says yes with the same bytes."""
    exe = str(tmp_path / "png_inflate_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "png_inflate_fuzz.cpp"), os.path.join(CSRC, "fl_pngsrc.cpp"), "-o", exe], check=True)
    files = []
    picks = ["z-fixed", "z-rle", "sync-flush-every-100", "single-distance-code", "15-bit-codes", "blocks-of-every-kind", "empty-stored-from-sync-flush"]
    cases = {n: d for n, d, _ in pc.valid()}
    for k, name in enumerate(picks):
        path = tmp_path / f"f{k}.png"
        path.write_bytes(cases[name])
        files.append(str(path))
    data, _ = pc.picture(2, 8, 37, 19, 7, interlace=1)
    (tmp_path / "a7.png").write_bytes(data)
    files.append(str(tmp_path / "a7.png"))
    r = subprocess.run([exe, "2000"] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("file ")]
    assert len(lines) == len(files) and all("intact=ok" in l for l in lines), r.stdout
    accepted = sum(int(l.split("accepted=")[1].split()[0]) for l in lines)
    refused = sum(int(l.split("refused=")[1].split()[0]) for l in lines)
    assert refused > 1000 and accepted > 0, r.stdout      # the mutants were really looked at: most are refused, some survive
