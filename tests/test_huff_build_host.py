"""csrc/fl_huff_build.h -- the length-limited Huffman builder of the PNG deflate and the lossless WebP encoder -- run on the CPU
under AddressSanitizer and UBSan (no GPU).  On the device its fold to 15 or 7 bits is next to unreachable: a symbol frequent enough
to make the tree that deep becomes matches in the LZ77 stage.  tests/huff_build_host.cpp includes the header unchanged and feeds it
Fibonacci, power-of-two, flat, two-symbol, full-alphabet and 20,000 seeded random histograms for every (limit, alphabet, scratch
size) the two encoders use, and checks lengths, Kraft sum, order, canonical bit-reversed codes, prefix freedom and the cost against
an unlimited heap-built tree or its repaired form; it says how many cases needed the fold, and every pair must have had some."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")

# (limit, alphabet, words of `num` scratch): read from the huff_build calls of fl_png.hip and fl_webpll.hip
PAIRS = {(15, 286, 96), (15, 30, 96), (7, 19, 96), (15, 280, 64), (15, 256, 64), (7, 19, 64)}
RANDOMS = 20000


def test_the_pairs_are_the_ones_the_encoders_use():
    """A new caller, alphabet or scratch size in the kernels must show up in PAIRS (and in the program's table)."""
    png = open(os.path.join(CSRC, "fl_png.hip")).read()
    wll = open(os.path.join(CSRC, "fl_webpll.hip")).read()
    assert png.count("huff_build(") == 2 and wll.count("huff_build(") == 2
    assert "286u : 30u" in png and "15u, n, " in png and "7u, 19u, " in png
    assert "kMiscBuild0 = 64, kMiscBuild1 = 160" in png            # 96 words between them
    assert "{280u, 256u, 256u, 256u}" in wll and "s_num[4][64]" in wll and "15u, n, " in wll and "7u, 19u, " in wll
    host = open(os.path.join(ROOT, "tests", "huff_build_host.cpp")).read()
    for limit, nsyms, words in PAIRS:
        assert "{%d, %d, %d, " % (limit, nsyms, words) in host


def test_huff_build_under_address_sanitizer(tmp_path):
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "huff_build_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "huff_build_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, str(RANDOMS)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    print("limit alphabet scratch cases folded:", rows)
    assert {row[:3] for row in rows} == PAIRS and len(rows) == len(PAIRS)
    for limit, nsyms, words, cases, folded in rows:
        assert cases >= RANDOMS + 2 * nsyms, (limit, nsyms, cases)
        assert folded > 0, f"no case of ({limit}, {nsyms}) needed the fold"
        assert folded < cases, f"every case of ({limit}, {nsyms}) needed the fold: the optimum branch never ran"
