"""The C++ mirror (include/fanlin_gpu.hpp) serving a lossless WebP request: tests/webp_host.cpp is compiled the way the existing
C/C++ clients are, runs one request through handler::State::process_image with the opt-in bit, and the body it wrote is checked
here against the library's own FE_NONE pixels and the restated encoder (tests/vp8l_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import vp8l_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fanlin-rs_amd")


def build(tmp_path):
    exe = str(tmp_path / "webp_host")
    subprocess.run(["g++", "-O1", "-Wall", "-Wextra", "-Werror", "-std=c++17", os.path.join(ROOT, "tests", "webp_host.cpp"), "-I", os.path.join(ROOT, "include"),
                    "-L", LIBDIR, "-lfanlin_gpu", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_webp_host_compiles(fl, tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
def test_webp_host_serves_the_webp_body(fl, gpu_state, tmp_path):
    out = str(tmp_path / "body.webp")
    r = subprocess.run([build(tmp_path), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "webp ok" in r.stdout, r.stderr
    y, x = np.mgrid[0:360, 0:640]
    px = np.stack([(x * (c + 1) + y * (3 - c)) // 3 for c in range(3)], axis=2).astype(np.uint8)
    want = gpu_state.process_pixels(px, fl.make_params(300, 200))
    data = open(out, "rb").read()
    assert np.array_equal(vm.decode_rgba(data), vm.into_rgba8(want))
    assert data == vm.encode(want)
    assert data == gpu_state.process_pixels(px, fl.make_params(300, 200, quality=100, front_end=fl.FE_WEBP_LOSSLESS))
