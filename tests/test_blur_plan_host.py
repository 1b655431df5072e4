"""blur_tile_kernel's table block against the kernel's own sizing rules, on the host (no GPU).

csrc/fl_tables.cpp build_blur_plan writes the block, csrc/fl_blur.h says how many lanes a workgroup has and how much LDS it is
given, csrc/fl_blur.hip indexes both without a bounds check.  tests/tools/asan_blur_plan.cpp builds the plan of every (sigma,
width, height) of a sweep that crosses each lane-count threshold and holds it against what the kernel relies on: tiles and windows
within the lanes and the hand-off row, bands within the picture, the three LDS areas within blur_lds_bytes(), and the dense
vertical and deduplicated horizontal weights equal, bit for bit, to the axis tables they were made from."""
import os
import shutil
import subprocess

import pytest


def test_blur_plan_fits_the_kernels_lanes_and_lds_under_address_sanitizer(tmp_path):
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "fanlin-rs_amd", "csrc")
    exe = str(tmp_path / "asan_blur_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + csrc, os.path.join(root, "tests", "tools", "asan_blur_plan.cpp"),
                    os.path.join(csrc, "fl_tables.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    plans, refused, at256, at384, at512 = (int(x) for x in r.stdout.split())
    assert plans + refused == 14 * 27 * 8 and plans > 600
    assert at256 + at384 + at512 == plans
    assert at256 > 0 and at384 > 0 and at512 > 0, "the sweep is meant to reach every instantiation of the kernel"
