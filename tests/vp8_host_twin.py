"""The lossy WebP encoder's host twin (tests/vp8_host.cpp: the kernels' own functions in plain loops, a program of its own) for the
test_webp_lossy*_host.py files: one way to build it, plain or under ASan + UBSan, and one way to run it and read what it says."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fanlin-rs_amd", "csrc")
_LINE = re.compile(r"vp8 ok (\d+) bytes, (\d+) of (\d+) macroblocks skipped, (\d+) B_PRED, (\d+) of 1056 probabilities updated, "
                   r"levels (\d+) (\d+) (\d+) (\d+) D (\d+) (\d+) (\d+) (\d+) chosen (\d+), segments on ([01]) qi (\d+) (\d+) (\d+) (\d+) prob (\d+) (\d+) (\d+)\n")


def build(tmp_path, sanitised=False):
    exe = str(tmp_path / "vp8_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitised else []
    subprocess.run(["g++", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-std=c++17", *extra, os.path.join(ROOT, "tests", "vp8_host.cpp"), "-I", CSRC, "-o", exe],
                   check=True)
    return exe


def run(exe, tmp_path, y, u, v, a, q, i4=False, adaptive=False, filt=False, filter_base=None, segments=False, files=()):
    """One picture (planes y, u, v and the alpha plane or None, quality q) through the twin.  -> dict: `file` (the bytes it wrote), the
    fields of the line it printed (bytes, skipped, mbs, b_pred, updated, levels, D, chosen, seg_on, seg_qi, seg_prob) and, for every
    name in `files` ("recon", "shown", "modes", "stats"), the bytes of that optional output."""
    h, w = y.shape
    planes, out = str(tmp_path / "planes.bin"), str(tmp_path / "out.webp")
    with open(planes, "wb") as f:
        f.write(y.tobytes() + u.tobytes() + v.tobytes() + (a if a is not None else np.full((h, w), 255, np.uint8)).tobytes())
    args = [exe, str(w), str(h), str(q), planes, out]
    args += [flag for flag, on in (("--translucent", a is not None), ("--i4", i4), ("--adaptive", adaptive), ("--filter", filt), ("--segments", segments)) if on]
    if filter_base is not None:
        args += ["--filter-base", str(filter_base)]
    for name in files:
        args += ["--" + name, str(tmp_path / (name + ".bin"))]
    r = subprocess.run(args, capture_output=True, text=True)
    m = _LINE.fullmatch(r.stdout)
    assert r.returncode == 0 and m and not r.stderr, (args[1:4], args[6:], r.returncode, r.stdout, r.stderr)
    n = [int(x) for x in m.groups()]
    got = {"file": open(out, "rb").read(), "bytes": n[0], "skipped": n[1], "mbs": n[2], "b_pred": n[3], "updated": n[4], "levels": n[5:9], "D": n[9:13],
           "chosen": n[13], "seg_on": n[14], "seg_qi": n[15:19], "seg_prob": n[19:22]}
    assert got["bytes"] == len(got["file"])
    for name in files:
        got[name] = open(str(tmp_path / (name + ".bin")), "rb").read()
    return got
