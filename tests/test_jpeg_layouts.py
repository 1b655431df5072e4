"""JPEG decode on the layouts, tables and sizes that Pillow's default files never show (companion of test_jpeg_decode.py).

The files are written by Pillow at run time and, where Pillow cannot be asked for a layout, rewritten by tests/jpeg_surgery.py:
  * a width sweep -- every width 1 .. 64 at 4:2:0 and at 4:2:2, a few at 4:4:4, heights from a short cycle, uniform noise -- for the
    row ends, narrow chroma planes and one-row tails of jpeg_color_kernel's fast form (csrc/fl_jpegdec.hip color_group);
  * 4:4:0, three-component RGB files (Adobe transform 0, planes sub-sampled or not), a one-component file that announces 2 x 2
    sampling, 16-bit quantiser tables: the pixel-wise form (color_pixel / chroma_at), a new MCU shape for the device entropy decoder;
  * optimised Huffman tables (optimize=True): single-code DC tables, 13 .. 16-bit code words past the 12-bit lookahead, end-of-block
    codes longer than the 7 bits the device fuses;
  * pictures that saturate: sat17 of the IDCT and clamp8 of the colour transform.
Bars as in test_jpeg_decode.py: host coefficients == the oracle's; oracle vs libjpeg-turbo inside the pinned bound (max <= 4, <= 2
for one component, mean < 1); device pixels bit-identical to the oracle, through the host entropy decoder and through the device's."""
import io
import types

import numpy as np
import pytest
from PIL import Image

import jpeg_surgery as js
import synth
from test_jpeg_decode import CASES

SAMPLING = {0: ((1, 1), "4:4:4"), 1: ((2, 1), "4:2:2"), 2: ((2, 2), "4:2:0")}     # Pillow's subsampling -> (hmax, vmax)
HEIGHTS = (1, 2, 3, 5, 8, 9, 16, 17)


def save(img, **kw):
    b = io.BytesIO()
    if img.shape[2] == 1:
        kw.pop("subsampling", None)
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(b, "JPEG", **kw)
    return b.getvalue()


def entry(name, data, h, w, nc, hv, content, rgb=False, same_as=None, twin=None):
    """One file of a case list.  h, w, nc, hv = (hmax, vmax) and rgb are what the file was BUILT to be; same_as: a file that must
    decode to the very same coefficients and pixels; twin: the optimize=False file of the same picture."""
    return types.SimpleNamespace(name=name, data=data, h=h, w=w, nc=nc, hv=hv, content=content, rgb=rgb, same_as=same_as, twin=twin)


def sweep_height(w):
    # the cycle advances one extra step every eight widths: widths of one w % 4 class meet all eight heights, not two of them
    return HEIGHTS[((w - 1) + (w - 1) // 8) % 8]


def sweep_files():
    out = []
    for sub, widths in ((2, range(1, 65)), (1, range(1, 65)), (0, (1, 2, 3, 5, 6, 7, 63))):
        for w in widths:
            h = sweep_height(w)
            # noise: neighbouring chroma samples differ strongly, so a wrong replicate at a row's end cannot decode to the right byte
            data = save(synth.uniform(h, w, 3, index=w + 100 * sub), quality=90, subsampling=sub)
            out.append(entry(f"sweep {SAMPLING[sub][1]} {h}x{w}", data, h, w, 3, SAMPLING[sub][0], "noise"))
    return out


def layout_files():
    out = []
    for h, w in ((40, 56), (37, 53), (16, 17), (1, 1), (9, 300)):                  # sizes before the swap
        data = js.to_440(save(synth.photo(h, w, 3, index=h + w), quality=85, subsampling=1))
        out.append(entry(f"4:4:0 {w}x{h}", data, w, h, 3, (1, 2), "photo"))
    for h, w in ((37, 53), (64, 96)):
        for sub in (0, 1, 2):
            data = js.to_rgb(save(synth.photo(h, w, 3, index=h + w + sub), quality=85, subsampling=sub))
            out.append(entry(f"rgb {SAMPLING[sub][1]} {h}x{w}", data, h, w, 3, SAMPLING[sub][0], "photo", rgb=True))
    base = save(synth.photo(33, 47, 1, index=5), quality=80)
    out.append(entry("gray 2x2 33x47", js.gray_2x2(base), 33, 47, 1, (1, 1), "photo", same_as=base))
    base = save(synth.photo(40, 56, 3, index=6), quality=85, subsampling=2)
    out.append(entry("dqt16 4:2:0 40x56", js.dqt16(base), 40, 56, 3, (2, 2), "photo", same_as=base))
    return out


def optimised_files():
    cases = [(h, w, c, q, sub, "photo") for h, w, c, q, sub, rst in CASES if not rst]
    cases += [(200, 301, 3, 95, 2, "photo"), (360, 640, 3, 92, 2, "photo"), (120, 160, 3, 98, 0, "uniform"), (120, 160, 3, 100, 2, "uniform")]
    out = []
    for h, w, c, q, sub, dist in cases:
        img = getattr(synth, dist)(h, w, c, index=h + w)
        data, twin = save(img, quality=q, subsampling=sub, optimize=True), save(img, quality=q, subsampling=sub)
        hv = SAMPLING[sub][0] if c == 3 else (1, 1)
        out.append(entry(f"optimised {dist} {SAMPLING[sub][1] if c == 3 else 'gray'} {h}x{w} q{q}", data, h, w, c, hv,
                         "photo" if dist == "photo" else "noise", twin=twin))
    return out


def saturating_pictures():
    yy, xx = np.mgrid[0:24, 0:40]
    stripes = lambda shift: ((((xx + yy // 5 + shift) // 3) & 1) * 255).astype(np.uint8)   # 0 / 255, three wide, stepped every five rows
    gray = stripes(0)[:, :, None]
    colour = np.stack([stripes(0)] * 3, axis=2)
    k = ((yy // 5) * 3 + xx // 6) % 8                                                        # 5 x 6 patches, the RGB cube's corners
    corners = np.stack([((k >> b) & 1) * 255 for b in range(3)], axis=2).astype(np.uint8)
    return (("gray stripes", gray), ("colour stripes", colour), ("cube corners", corners))


def saturating_files():
    out = []
    for name, img in saturating_pictures():
        for q in (10, 30, 60):
            for sub in ((0, 1, 2) if img.shape[2] == 3 else (0,)):
                hv = SAMPLING[sub][0] if img.shape[2] == 3 else (1, 1)
                tag = SAMPLING[sub][1] if img.shape[2] == 3 else "gray"
                out.append(entry(f"saturating {name} {tag} q{q}", save(img, quality=q, subsampling=sub), 24, 40, img.shape[2], hv, "flat"))
    return out


LISTS = {"sweep": sweep_files, "layouts": layout_files, "optimised": optimised_files, "saturating": saturating_files}
_FILES, _PIXELS = {}, {}


def files(which):
    if which not in _FILES:
        _FILES[which] = LISTS[which]()
    return _FILES[which]


def reference(oracle, f):
    """oracle.jpeg_decode of a file, computed once for all the tests that compare with it (read-only)."""
    if f.name not in _PIXELS:
        px = oracle.jpeg_decode(f.data)
        px.setflags(write=False)
        _PIXELS[f.name] = px
    return _PIXELS[f.name]


def geometry(f):
    """(c_w, c_rows, nblocks) of a file from what it was built to be: chroma plane size in samples, blocks of the whole frame."""
    hm, vm = f.hv
    mcux, mcuy = -(-f.w // (8 * hm)), -(-f.h // (8 * vm))
    nblocks = mcux * mcuy * (1 if f.nc == 1 else hm * vm + f.nc - 1)      # luma hm x vm blocks per MCU, one per other component
    return -(-f.w // hm), -(-f.h // vm), nblocks


def table_summary(data):
    """(longest code word of any table, longest end-of-block code of the AC tables)."""
    t = js.huffman_tables(data)
    return max(x[2] for x in t), max(x[3] for x in t if x[0] == 1)


def device_takes(f):
    """The staging rule of csrc/fl_jpeghuff.cpp jpeg_entropy_stage, restated: a sequential file of 1 or 3 components in one scan, of at
    least 7 bits per block (below that the stream is periodic and stays with the host decoder)."""
    segs, _ = js.segments(f.data)
    one_scan = [m for m, _ in segs].count(js.SOF0) == 1 and segs[-1][1][0] == f.nc
    return f.nc in (1, 3) and one_scan and js.entropy_bits(f.data) >= 7 * geometry(f)[2]


ONE_SUBSEQUENCE = 1024    # bits the device decodes in one walk (csrc/fl_jpegdec.h kJhSubBits): a shorter scan involves no speculation


def where(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    y, x, c = bad[0]
    return f"{len(bad)} bytes differ, first at y={y} x={x} c={c}: {got[y, x, c]} != {want[y, x, c]}"


# ------------------------------------------------------------------------------------ the lists are what they claim (CPU) --

def test_the_surgery_reads_a_file_it_did_not_write():
    """huffman_tables and entropy_bits on a default Pillow file: the Annex K tables (longest codes 9 / 16 / 11 / 16 bits, end-of-block
    codes of 4 and 2 bits, T.81 tables K.3 - K.6) and a scan as long as the file says."""
    data = save(synth.photo(40, 56, 3, index=1), quality=85, subsampling=2)
    assert sorted(js.huffman_tables(data)) == [(0, 0, 9, None), (0, 1, 11, None), (1, 0, 16, 4), (1, 1, 16, 2)]
    segs, scan = js.segments(data)
    body = data[scan:-2]
    assert data[-2:] == b"\xff\xd9" and js.entropy_bits(data) == 8 * (len(body) - body.count(b"\xff\x00"))
    rst = save(synth.photo(40, 56, 3, index=1), quality=85, subsampling=2, restart_marker_blocks=2)
    assert js.entropy_bits(rst) % 8 == 0 and js.entropy_bits(rst) > js.entropy_bits(data)      # (padding in front of every marker)
    assert js.frame(js.to_440(save(synth.photo(16, 24, 3), subsampling=1))) == (24, 16, [(1, 1, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)])
    assert js.dqt16(data) != data and len(js.dqt16(data)) == len(data) + 128


def test_sweep_covers_every_row_end_of_the_fast_form():
    """color_group handles a row's ends by position (`x0 ? ..`, `last < 2`, `last < 3`, W - x0 pixels stored) and a one-row tail by
    `rows`: each w % 4 with an odd and with an even height, chroma planes 1, 2, 3 and more samples wide, 1, 2 and more rows high --
    and one row high under a row of several groups, which Pillow's 1 x 1 picture never was."""
    by_layout = {}
    for f in files("sweep"):
        by_layout.setdefault(f.hv, []).append(f)
    assert set(by_layout) == {(1, 1), (2, 1), (2, 2)}
    assert {f.w for f in by_layout[(1, 1)]} == {1, 2, 3, 5, 6, 7, 63}
    for hv in ((2, 1), (2, 2)):
        fs = by_layout[hv]
        assert sorted(f.w for f in fs) == list(range(1, 65))
        for r in range(4):
            assert any(f.w % 4 == r and f.h % 2 == 1 for f in fs) and any(f.w % 4 == r and f.h % 2 == 0 for f in fs), (hv, r)
            assert {f.h for f in fs if f.w % 4 == r} == set(HEIGHTS), (hv, r)
        cw = {geometry(f)[0] for f in fs}
        rows = {geometry(f)[1] for f in fs}
        assert {1, 2, 3} <= cw and max(cw) >= 4 and {1, 2} <= rows and max(rows) >= 3, (hv, cw, rows)
        assert any(geometry(f)[1] == 1 and geometry(f)[0] >= 4 for f in fs), hv
        assert any(geometry(f)[2] > 32 for f in fs), "more blocks than one workgroup of the IDCT takes"
    for f in files("sweep"):
        assert js.frame(f.data) == (f.h, f.w, [(1,) + f.hv + (0,), (2, 1, 1, 1), (3, 1, 1, 1)]), f.name


def test_layout_files_are_the_layouts_they_claim():
    fs = {f.name: f for f in files("layouts")}
    assert len(fs) == 13
    for f in fs.values():
        h, w, comps = js.frame(f.data)
        segs = js.segments(f.data)[0]
        adobe = [p[11] for m, p in segs if m == js.APP14 and p[:5] == b"Adobe"]
        jfif = [p for m, p in segs if m == js.APP0 and p[:5] == b"JFIF\0"]
        assert (h, w, len(comps)) == (f.h, f.w, f.nc), f.name
        assert (adobe == [0] and not jfif) if f.rgb else (not adobe and len(jfif) == 1), f.name
        if f.name.startswith("4:4:0"):
            assert [c[1:3] for c in comps] == [(1, 2), (1, 1), (1, 1)]
        if f.name.startswith("gray 2x2"):
            assert comps[0][1:3] == (2, 2)
        if f.name.startswith("dqt16"):
            dqt = [p for m, p in segs if m == js.DQT]
            assert dqt and all(len(p) % 129 == 0 and all(p[o] >> 4 == 1 for o in range(0, len(p), 129)) for p in dqt)
    assert {f.hv for f in fs.values() if f.rgb} == {(1, 1), (2, 1), (2, 2)}
    assert [(f.h, f.w) for f in fs.values() if f.hv == (1, 2)] == [(56, 40), (53, 37), (17, 16), (1, 1), (300, 9)]


def test_optimised_files_hold_the_tables_the_default_files_never_show():
    fs = files("optimised")
    assert len(fs) == sum(1 for case in CASES if not case[5]) + 4 == 18
    tabs = {f.name: table_summary(f.data) for f in fs}
    for f in fs:
        assert f.data != f.twin and js.huffman_tables(f.data) != js.huffman_tables(f.twin), f.name
    assert any(longest == 16 for longest, eob in tabs.values()), tabs
    assert any(longest >= 13 and eob <= 7 for longest, eob in tabs.values()), tabs      # past the lookahead, end of block still fused
    assert any(eob > 7 for longest, eob in tabs.values()), tabs                        # not fused (el > 7 in jpeg_entropy_stage)
    assert all(table_summary(f.twin)[1] <= 4 for f in fs)                              # Annex K: 4 and 2 bits
    # tables of one single code: the DC table of the 8 x 8 picture (one block per component), the AC tables of the 1 x 1 picture
    # (nothing but end-of-block codes)
    one_code = {(f.name, tc) for f in fs for tc, th, longest, eob in js.huffman_tables(f.data) if longest == 1}
    assert {tc for name, tc in one_code} == {0, 1}, one_code


def test_saturating_pictures_saturate(oracle):
    """The condition is on the inputs, so it is asserted on the ORACLE's pixels: at least a fifth of the decoded bytes sit at 0 or 255,
    i.e. sat17 / clamp8 decide them (coarse quantisation of hard edges overshoots on both sides)."""
    fs = files("saturating")
    assert len(fs) == 3 + 9 + 9
    for f in fs:
        px = reference(oracle, f)
        share = float(((px == 0) | (px == 255)).mean())
        assert share >= 0.20, (f.name, share)


# ------------------------------------------------------------------------------------------ oracle and host half (CPU) --

@pytest.mark.parametrize("which", list(LISTS))
def test_host_half_reads_the_oracles_coefficients(fl, oracle, which):
    for f in files(which):
        info = fl.jpeg_info(f.data)
        assert (info["height"], info["width"], info["components"], info["supported"], info["progressive"]) == (f.h, f.w, f.nc, 1, 0), f.name
        if f.nc == 3:
            assert (info["h_max"], info["v_max"]) == f.hv and info["channels"] == 3, f.name
        assert info["adobe_transform"] == (1 if f.rgb else 0), f.name                  # (the ABI reports the APP14 byte + 1, 0 = none)
        hdr, got, _ = fl.debug_jpeg_blob(f.data)
        want = oracle.jpeg_file_coefficients(f.data)
        assert (hdr["height"], hdr["width"], hdr["nc"], hdr["hmax"], hdr["vmax"]) == (f.h, f.w, f.nc) + f.hv, f.name
        assert hdr["nblocks"] == geometry(f)[2] == want.shape[0], f.name
        assert hdr["is_rgb"] == int(f.rgb), f.name
        assert got.shape == want.shape and np.array_equal(got, want), f.name
        assert oracle.jpeg_info(f.data)[:4] == (0, f.w, f.h, f.nc), f.name


def test_optimised_files_hold_the_coefficients_of_their_twins(fl, oracle):
    """libjpeg quantises a picture identically whether it then writes Annex K tables or optimised ones: the twins hold the same
    coefficients and decode to the same pixels -- both table readers checked against files that share nothing but the picture."""
    for f in files("optimised"):
        want = oracle.jpeg_file_coefficients(f.twin)
        assert np.array_equal(oracle.jpeg_file_coefficients(f.data), want), f.name
        assert np.array_equal(fl.debug_jpeg_blob(f.data)[1], want), f.name
        assert np.array_equal(reference(oracle, f), oracle.jpeg_decode(f.twin)), f.name


def test_rewritten_tables_and_sampling_bytes_change_nothing(fl, oracle):
    """16-bit quantiser tables of the same steps, and a single component that announces 2 x 2: the same picture as before."""
    checked = 0
    for f in files("layouts"):
        if f.same_as is None:
            continue
        assert f.data != f.same_as
        hdr, got, blob = fl.debug_jpeg_blob(f.data)
        hdr0, got0, blob0 = fl.debug_jpeg_blob(f.same_as)
        assert np.array_equal(got, got0) and np.array_equal(blob, blob0), f.name      # (the blob carries the quantiser steps too)
        assert np.array_equal(oracle.jpeg_file_coefficients(f.data), oracle.jpeg_file_coefficients(f.same_as)), f.name
        assert np.array_equal(reference(oracle, f), oracle.jpeg_decode(f.same_as)), f.name
        checked += 1
    assert checked == 2


def pillow_comparable(f):
    """libjpeg switches from interpolation to sample replication when a sub-sampled plane is at most 2 samples wide (jdsample.c:
    `downsampled_width > 2` for the fancy up-samplers); zune-jpeg interpolates regardless.  On noise that is 15 - 29 LSB between the
    two LIBRARIES and says nothing about either restatement, so those files are left out of this comparison -- and of no other."""
    return f.hv == (1, 1) or geometry(f)[0] > 2


@pytest.mark.parametrize("which", list(LISTS))
def test_oracle_vs_libjpeg_inside_the_pinned_bound(oracle, which):
    """The bound of test_oracle_decoder_vs_libjpeg_on_synthetic_streams, unchanged: max <= 4 (<= 2 for one component), mean < 1."""
    left_out = [f for f in files(which) if not pillow_comparable(f)]
    assert all(f.w <= 4 and f.hv != (1, 1) for f in left_out) and len(left_out) <= (8 if which == "sweep" else 1), [f.name for f in left_out]
    for f in files(which):
        if not pillow_comparable(f):
            continue
        pil = Image.open(io.BytesIO(f.data))
        assert pil.mode == ("L" if f.nc == 1 else "RGB"), f.name
        ref = np.array(pil).reshape(f.h, f.w, f.nc)
        d = np.abs(reference(oracle, f).astype(np.int16) - ref.astype(np.int16))
        assert int(d.max()) <= (2 if f.nc == 1 else 4) and float(d.mean()) < 1.0, (f.name, int(d.max()), float(d.mean()))


# ------------------------------------------------------------------------------------------------ device half (GPU) --

def decode_both_ways(gpu_state, oracle, f):
    """One file through gpu_state.decode_jpeg with the host entropy decoder (the blob's i16 / i8 form, the IDCT's general loop) and
    with the device's (full wide blocks, the IDCT's 16-byte loads): pixels are the oracle's both times.  Returns (device decodes,
    retries) counted by the second run."""
    want = reference(oracle, f)
    gpu_state.debug_set("host_huffman", 1)
    got = gpu_state.decode_jpeg(f.data)
    assert np.array_equal(got, want), (f.name, "host entropy decoder", where(got, want))
    gpu_state.debug_set("host_huffman", 0)
    gpu_state.debug_set("device_huffman_min_bytes", 0)
    gpu_state.debug_set("device_huffman_always", 1)
    s0 = gpu_state.stats()
    got = gpu_state.decode_jpeg(f.data)
    s1 = gpu_state.stats()
    assert np.array_equal(got, want), (f.name, "device entropy decoder", where(got, want))
    return s1["jpeg_device_huffman"] - s0["jpeg_device_huffman"], s1["jpeg_device_huffman_retries"] - s0["jpeg_device_huffman_retries"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(LISTS))
def test_device_decode_is_bit_identical_on_every_list(fl, gpu_state, oracle, which):
    """Every file of every list, both entropy paths, against the oracle decoder.  Which side decoded the second run is asserted against
    the staging rule restated in device_takes; a photo file must not need the host retry, which would let the host decoder hide a
    failure of the device's, and neither must a file of a single subsequence, which is decoded from its first bit with nothing guessed.
    (Longer noise and stripe files may: fuzz_jpegdec.py notes chains of states that do not settle on them.)"""
    seen = []
    for f in files(which):
        dev, retries = decode_both_ways(gpu_state, oracle, f)
        assert dev == int(device_takes(f)), (f.name, dev, js.entropy_bits(f.data), geometry(f)[2])
        if f.content == "photo" or js.entropy_bits(f.data) <= ONE_SUBSEQUENCE:
            assert retries == 0, f.name
        seen.append((f, dev, retries))
        print(f"{f.name}: device {dev}, retries {retries}, tables {table_summary(f.data)}")
    assert sum(dev for f, dev, r in seen) >= len(seen) // 2, "most files are meant to reach the device entropy decoder"
    if which == "optimised":
        # an end-of-block code the tables do not fuse (longer than 7 bits), decoded by the device itself.  Observed on an MI355X: the photo
        # file 200x301 q100 (16-bit codes, 9-bit end of block) is, without a retry; both noise files (120x160 q98 4:4:4, end of block 13
        # bits, and q100 4:2:0, 11 bits) are staged for the device and end in the host retry -- their chains of states do not settle
        assert any(dev == 1 and r == 0 and table_summary(f.data)[1] > 7 for f, dev, r in seen)
        assert any(dev == 1 and r == 0 and table_summary(f.data)[0] == 16 for f, dev, r in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("entropy", ["host", "device"])
def test_mixed_layouts_in_one_batch(fl, gpu_state, oracle, entropy):
    """One flgpu_transform_batch over pictures of every colour mode: the grids are sized by the batch's largest picture and the mode is
    per job, so a small pixel-wise job beside a large fast-form one (and the reverse) must each see its own geometry."""
    lay = {f.name: f for f in files("layouts")}
    sweep = {f.name: f for f in files("sweep")}
    opt = {f.name: f for f in files("optimised")}
    batch = [lay["4:4:0 56x40"], lay["rgb 4:4:4 37x53"], lay["rgb 4:2:0 64x96"], lay["gray 2x2 33x47"], lay["dqt16 4:2:0 40x56"],
             opt["optimised photo 4:2:0 37x53 q70"], sweep["sweep 4:2:0 3x3"],
             entry("4:2:2 64x96", save(synth.photo(64, 96, 3, index=11), quality=85, subsampling=1), 64, 96, 3, (2, 1), "photo")]
    p = fl.make_params(40, 30)
    want = [gpu_state.process_pixels(reference(oracle, f), p) for f in batch]         # the pixel-source path, checked against the oracle elsewhere
    if entropy == "host":
        gpu_state.debug_set("host_huffman", 1)
    else:
        gpu_state.debug_set("device_huffman_min_bytes", 0)
        gpu_state.debug_set("device_huffman_always", 1)
    s0 = gpu_state.stats()
    got = gpu_state.process_batch([f.data for f in batch], [p] * len(batch))
    s1 = gpu_state.stats()
    for f, a, b in zip(batch, got, want):
        assert np.array_equal(a, b), (f.name, where(a, b))
    assert s1["jpeg_device_huffman"] - s0["jpeg_device_huffman"] == (sum(device_takes(f) for f in batch) if entropy == "device" else 0)
    assert all(f.content == "photo" or js.entropy_bits(f.data) <= ONE_SUBSEQUENCE for f in batch)
    assert s1["jpeg_device_huffman_retries"] == s0["jpeg_device_huffman_retries"]
