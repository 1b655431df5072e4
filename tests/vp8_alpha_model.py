"""A numpy restatement of the ALPH chunk FLGPU_FEO_ALPHA_VP8L makes the lossy WebP front ends write (fanlin-rs_amd/csrc/fl_webpll.hip
in alpha mode, fl_vp8.hip vp8_frame_kernel), built from the pieces of tests/vp8l_model.py.  Test infrastructure only.

The pixels are ARGB (255, 0, a, 0).  The stream is the lossless coder's minus its 40 header bits and minus subtract-green (which
would turn the zero red and blue into -g): the predictor transform with 2^9 blocks and a one-symbol sub-image of mode 2 (T; L on
row 0, black 0xff000000 for the first pixel), no colour cache, no meta codes, a real green + length code, one-symbol red, blue,
alpha and distance codes of 0 bits, runs of the previous residual of at most 4096.

    alpha_stream(a)      the byte-aligned VP8L stream of the plane a (h, w)
    alph_payload(a)      the chunk's payload by the rule: b"\\x01" + stream iff that is strictly smaller than b"\\x00" + plane
    with_alpha(file, a)  a file of any of the lossy models (vp8_model and the _i4, _ap, _lf models) with its ALPH payload replaced
                         by alph_payload(a), the RIFF size and the pad byte fixed, every other chunk untouched; an opaque file (no
                         ALPH chunk) comes back as it is
    chunks(file)         [(tag, payload)] of a RIFF / WEBP file"""
import struct

import numpy as np

import vp8l_model as ll


def residuals(a):
    """(h * w, 4) uint8 residuals (a, r, g, b) of the plane read as ARGB (255, 0, a, 0), after the predictor transform alone."""
    a = np.asarray(a, np.uint8)
    h, w = a.shape
    argb = np.zeros((h, w, 4), np.int32)
    argb[..., 0] = 255
    argb[..., 2] = a
    pred = np.zeros_like(argb)
    pred[1:] = argb[:-1]                  # T for every later row, column 0 included
    pred[0, 1:] = argb[0, :-1]            # L on row 0
    pred[0, 0] = (255, 0, 0, 0)           # ARGB black for the first pixel
    return ((argb - pred) & 255).astype(np.uint8).reshape(h * w, 4)


def header(hists):
    """The stream up to the pixel data (from the transform bits on), and the four codes."""
    bw = ll.BitWriter()
    bw.put(0b111001, 6)                    # predictor, 2^9 blocks
    bw.put(0, 1)                           # sub-image: no colour cache
    ll.write_simple(bw, 2)                 # mode T
    for _ in range(4):
        ll.write_simple(bw, 0)
    bw.put(0, 1); bw.put(0, 1); bw.put(0, 1)  # no more transforms, no colour cache, no meta prefix codes
    codes = [ll.write_code(bw, hists[k], ll.ALPHABETS[k]) for k in range(4)]
    ll.write_simple(bw, 1)                 # distance: plane code 2, the left pixel
    return bw, codes


def alpha_stream(a, stats=None):
    res = residuals(a)
    lit, ref, m = ll.tokens(res)
    hists = ll.histograms(res, lit, ref, m)
    bw, codes = header(hists)
    # red, blue and alpha residuals are all zero: one-symbol codes, 0 bits per literal
    assert all(sum(1 for f in hists[k] if f) == 1 and hists[k][0] for k in (1, 2, 3))
    n = len(res)
    vals = np.zeros((n, 2), np.uint64)
    lens = np.zeros((n, 2), np.int64)
    cl = np.asarray(codes[0][0], np.int64)
    cc = np.asarray(codes[0][1], np.uint64)
    sym = res[lit, 2].astype(np.int64)
    vals[lit, 0] = cc[sym]
    lens[lit, 0] = cl[sym]
    if ref.any():
        pc = [ll.prefix_code(int(v)) for v in m[ref]]
        sym = np.array([256 + p[0] for p in pc], np.int64)
        vals[ref, 0] = cc[sym]
        lens[ref, 0] = cl[sym]
        vals[ref, 1] = np.array([p[2] for p in pc], np.uint64)
        lens[ref, 1] = np.array([p[1] for p in pc], np.int64)
    data, _ = ll.pack(np.concatenate([np.asarray(bw.vals, np.uint64), vals.ravel()]),
                      np.concatenate([np.asarray(bw.lens, np.int64), lens.ravel()]))
    if stats is not None:
        stats.update(literals=int(lit.sum()), refs=int(ref.sum()), longest=int(m[ref].max()) if ref.any() else 0,
                     header_bits=bw.bits(), green_symbols=sum(1 for f in hists[0] if f))
    return data


def alph_payload(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    stream = alpha_stream(a)
    return b"\x01" + stream if 1 + len(stream) < 1 + a.size else b"\x00" + a.tobytes()


def chunks(data):
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP" and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out, o = [], 12
    while o < len(data):
        n, = struct.unpack("<I", data[o + 4:o + 8])
        out.append((bytes(data[o:o + 4]), bytes(data[o + 8:o + 8 + n])))
        o += 8 + n + (n & 1)
    assert o == len(data)
    return out


def with_alpha(data, a):
    parts = chunks(data)
    if not any(tag == b"ALPH" for tag, _ in parts):
        return data
    h, w = np.asarray(a).shape
    body = b""
    for tag, payload in parts:
        if tag == b"ALPH":
            assert payload == b"\x00" + np.ascontiguousarray(a, dtype=np.uint8).tobytes(), "the file's raw plane is not `a`"
            payload = alph_payload(a)
        body += tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


def alph_of(data):
    """The ALPH payload of a file, or None."""
    return dict(chunks(data)).get(b"ALPH")
