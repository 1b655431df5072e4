"""The C++ mirror (include/fanlin_gpu.hpp) serving a PNG request: tests/png_host.cpp is compiled the way the existing C/C++
clients are, runs one request through handler::State::process_image with the opt-in bit, and the body it wrote is checked
here against the library's own FE_NONE pixels."""
import os
import subprocess

import numpy as np
import pytest

from test_png_encode import check_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fanlin-rs_amd")


def build(tmp_path):
    exe = str(tmp_path / "png_host")
    subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", os.path.join(ROOT, "tests", "png_host.cpp"), "-I", os.path.join(ROOT, "include"),
                    "-L", LIBDIR, "-lfanlin_gpu", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_png_host_compiles(fl, tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
def test_png_host_serves_the_png_body(fl, gpu_state, tmp_path):
    out = str(tmp_path / "body.png")
    r = subprocess.run([build(tmp_path), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "png ok" in r.stdout, r.stderr
    y, x = np.mgrid[0:360, 0:640]
    px = np.stack([(x * (c + 1) + y * (3 - c)) // 3 for c in range(3)], axis=2).astype(np.uint8)
    want = gpu_state.process_pixels(px, fl.make_params(300, 200))
    data = open(out, "rb").read()
    check_stream(data, want, 75)
    assert data == gpu_state.process_pixels(px, fl.make_params(300, 200, quality=75, front_end=fl.FE_PNG))
