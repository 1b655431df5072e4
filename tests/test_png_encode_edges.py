"""FLGPU_FE_PNG where the corpus of test_png_encode.py never goes (csrc/fl_png.hip): filtered streams that end on, one before and
one or two bytes after a multiple of the 32 KB segment, a row across three segments, matches at distance 32768 and of length 258,
stored and dynamic segments side by side, Adler-32 sums at their moduli, every tie of the adaptive filter's `<=` chain, the
qualities either side of the level thresholds, and batches whose PNG jobs differ in size so that one filter workgroup serves two
pictures and the scratch offsets are unequal.

Every picture is synthetic and seeded; every file is produced twice and must be the same bytes both times (the hash chains must
not depend on the order of the LDS atomics); every file goes through check_stream against the FE_NONE pixels and segment_chunks,
and each edge a case is there for is asserted on the file or on the model, not assumed.  No compression-ratio bar lives here
(zlib never uses distance 32768, and the 512-byte lanes clip matches): sizes against zlib are printed, and the only caps asserted
are derived ones -- max_out_bytes, the stored form of a segment, and the window case's second chunk against its first."""
import threading
import zlib

import numpy as np
import pytest

import deflate_walk as dw
import synth
from png_enc_model import SEG, check_stream, chunks_of, filter_rows, filter_scores, filtered_bytes, max_out_bytes, segment_chunks

QUALITY = {"best": 30, "default": 75, "fast": 95}    # csrc/fl_png.h png_level: < 50 Best, < 85 Default, otherwise Fast
ALL_LEVELS = tuple(QUALITY.values())


def noise(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def smooth(w, h, c, seed):
    """A slow ramp in both directions with one bit of seeded texture."""
    yy, xx, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    tex = np.random.default_rng(seed).integers(0, 2, (h, w, c))
    return ((xx * 3 // 8 + yy * 5 + ch * 37 + tex) & 255).astype(np.uint8)


def segment_lengths(w, h, c):
    f = filtered_bytes(w, h, c)
    n = (f + SEG - 1) // SEG
    return [SEG] * (n - 1) + [f - (n - 1) * SEG]


def png_params(fl, quality):
    return fl.make_params(quality=quality, front_end=fl.FE_PNG)


@pytest.fixture(scope="module")
def encode(fl, gpu_state):
    """encode(px, quality) -> (file, zlib stream, filtered stream, segments' deflate bodies): encoded twice, both files identical,
    checked against the FE_NONE pixels of the same request and against the segment layout."""
    def run(px, quality):
        seen = gpu_state.process_pixels(px, fl.make_params())
        assert np.array_equal(seen, px), "FE_NONE without a size is the identity"
        p = png_params(fl, quality)
        data = gpu_state.process_pixels(px, p)
        again = gpu_state.process_pixels(px, p)
        assert isinstance(data, bytes) and data == again, "two runs of one request gave different files"
        h, w, c = px.shape
        assert len(data) <= max_out_bytes(w, h, c)
        z, raw = check_stream(data, seen, quality)
        raw2, bodies = segment_chunks(data)
        assert raw2 == raw and len(bodies) == len(segment_lengths(w, h, c))
        return data, z, raw, bodies
    return run


def report(name, z, raw):
    print(f"{name}: device {len(z)} / zlib -6 {len(zlib.compress(raw, 6))} / zlib -1 {len(zlib.compress(raw, 1))}")


def walk_segments(bodies, raw):
    """The walker over every segment's body; the symbols of segment s, replayed on the filtered bytes before it, must be its bytes."""
    assert len(bodies) <= 4, "the walker is kept to files of at most four segments"
    out = []
    for s, body in enumerate(bodies):
        blocks, end = dw.walk(body)
        assert (end + 7) // 8 == len(body), f"segment {s}: bytes behind its last block"
        assert dw.replay(blocks, history=raw[:s * SEG]) == raw[s * SEG:(s + 1) * SEG], f"segment {s}"
        out.append(blocks)
    return out


# ------------------------------------------------------------------------------------------------------ geometry --

# (w, h, c, filtered bytes, length of the last segment, levels)
GEOMETRY = [
    (127, 256, 1, 32768, 32768, (75,)),          # exactly one full segment, nothing behind it
    (85, 128, 3, 32768, 32768, (75,)),
    (1170, 7, 4, 32767, 32767, (75,)),
    (910, 9, 4, 32769, 1, ALL_LEVELS),           # last segment: 1 byte, no hashable position
    (127, 512, 1, 65536, 32768, (75,)),
    (16384, 1, 4, 65537, 1, ALL_LEVELS),         # one row over three segments, last segment 1 byte
    (8192, 2, 4, 65538, 2, ALL_LEVELS),          # last segment: 2 bytes
    (1, 1, 1, 2, 2, ALL_LEVELS), (1, 1, 2, 3, 3, ALL_LEVELS), (1, 1, 3, 4, 4, ALL_LEVELS), (1, 1, 4, 5, 5, ALL_LEVELS),
    (2, 1, 1, 3, 3, ALL_LEVELS),
]


def test_the_geometry_table_is_what_it_says():
    for w, h, c, f, tail, _ in GEOMETRY:
        assert filtered_bytes(w, h, c) == f and segment_lengths(w, h, c)[-1] == tail, (w, h, c)
    assert len(segment_lengths(16384, 1, 4)) == 3 and len(segment_lengths(8192, 2, 4)) == 3 and len(segment_lengths(910, 9, 4)) == 2
    assert len(segment_lengths(127, 256, 1)) == 1 and len(segment_lengths(85, 128, 3)) == 1 and len(segment_lengths(127, 512, 1)) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["noise", "smooth"])
@pytest.mark.parametrize("w,h,c,fbytes,tail,levels", GEOMETRY, ids=[f"{g[0]}x{g[1]}x{g[2]}" for g in GEOMETRY])
def test_segment_geometry(fl, gpu_state, encode, w, h, c, fbytes, tail, levels, content):
    px = (noise if content == "noise" else smooth)(w, h, c, seed=w + h + c)
    lens = segment_lengths(w, h, c)
    for q in levels:
        data, z, raw, bodies = encode(px, q)
        assert len(raw) == fbytes and [len(b) <= 5 + n for b, n in zip(bodies, lens)] == [True] * len(lens)
        report(f"{w}x{h}x{c} {content} q{q}", z, raw)
        if len(lens) <= 4 and (tail <= 2 or fbytes <= 8):
            blocks = walk_segments(bodies, raw)
            assert sum(len(dw.replay(b, history=raw[:s * SEG])) for s, b in enumerate(blocks)) == fbytes
            assert len(dw.replay(blocks[-1], history=raw[:(len(lens) - 1) * SEG])) == tail, "the tail segment's own bytes"
            assert [b.final for bl in blocks for b in bl][-1] and not any([b.final for bl in blocks for b in bl][:-1])
        if content == "noise":
            # (a few bytes of "noise" may well deflate, a kilobyte and more does not)
            assert all((body[0] & 6) == 0 for body, n in zip(bodies, lens) if n >= 1024), "noise segments are stored blocks"
            p = png_params(fl, q)
            assert gpu_state.process_pixels(px, p, capacity=-len(data)) == data
            with pytest.raises(fl.FanlinError) as e:
                gpu_state.process_pixels(px, p, capacity=-(len(data) - 1))
            assert e.value.status == fl.ERR_BUFFER_TOO_SMALL


# -------------------------------------------------------------------------------------------------- history window --

def window_picture():
    """127 x 512 x 1: rows 256..511 repeat rows 0..255, all zero but for about 300 bytes of noise that start 40 bytes into the
    512 bytes of one parse lane (rows 40..43 of each half are lane 10's)."""
    half = np.zeros((256, 127, 1), np.uint8)
    flat = half.reshape(-1)
    start = 40 * 127 + 40
    flat[start:start + 300] = np.random.default_rng(77).integers(1, 256, 300, dtype=np.uint8)
    return np.concatenate([half, half])


def test_the_window_picture_filters_to_two_identical_halves():
    px = window_picture()
    assert not px[255].any() and not px[511].any()
    _, raw = filter_rows(px)
    assert len(raw) == 2 * SEG and raw[:SEG] == raw[SEG:]
    nz = np.flatnonzero(np.frombuffer(raw[:SEG], np.uint8).reshape(256, 128)[:, 1:].any(axis=1))
    assert nz.min() >= 40 and nz.max() <= 43, "the marker stays inside the four rows of one lane"


@pytest.mark.gpu
@pytest.mark.parametrize("level", list(QUALITY))
def test_matches_reach_distance_32768_and_length_258(encode, level):
    q = QUALITY[level]
    data, z, raw, bodies = encode(window_picture(), q)
    report(f"window q{q}", z, raw)
    first, second = walk_segments(bodies, raw)
    matches = [m for b in second for m in b.matches()]
    hist = {}
    for length, dist in matches:
        hist[dist] = hist.get(dist, 0) + 1
    print(f"window q{q}: second segment's distances {sorted(hist.items())}, longest match {max(m[0] for m in matches)}")
    assert all(1 <= d <= 32768 and 3 <= n <= 258 for n, d in matches)
    assert any(d == 32768 for _, d in matches), "no match at distance 32768 (the first byte of the window)"
    assert any(n == 258 and d == 32768 for n, d in matches), "the marker was not matched at full length from the first half"
    assert any(n == 258 for n, _ in matches)
    assert any(d == 1 for _, d in matches), "no run coded at distance 1"
    assert all(d < 32768 for b in first for _, d in b.matches())
    chunk1, chunk2 = 12 + 2 + len(bodies[0]), 12 + len(bodies[1])
    assert chunk2 <= chunk1 + 64, (chunk1, chunk2)            # the same data again, with the first half to copy from
    assert chunk2 < (12 + 5 + SEG) // 8


# ------------------------------------------------------------------------------------------- stored / dynamic mix --

@pytest.mark.gpu
@pytest.mark.parametrize("order", ["stored_then_dynamic", "dynamic_then_stored"])
def test_stored_and_dynamic_segments_side_by_side(encode, order):
    rnd, zero = noise(127, 256, 1, seed=3), np.zeros((256, 127, 1), np.uint8)
    px = np.concatenate([rnd, zero] if order == "stored_then_dynamic" else [zero, rnd])
    for q in ALL_LEVELS:
        data, z, raw, bodies = encode(px, q)
        report(f"{order} q{q}", z, raw)
        blocks = walk_segments(bodies, raw)
        types = tuple(b[0].type for b in blocks)
        assert types == ((dw.STORED, dw.DYNAMIC) if order == "stored_then_dynamic" else (dw.DYNAMIC, dw.STORED)), types
        flat = [b for bl in blocks for b in bl]
        assert [b.final for b in flat] == [False] * (len(flat) - 1) + [True], "BFINAL on the last block and on no other"
        if order == "stored_then_dynamic":
            assert len(blocks[0]) == 1 and len(bodies[0]) == 5 + SEG and len(blocks[1]) == 1    # no flush behind a stored block
        else:
            # the dynamic block, then the empty stored block that ends the segment on a byte boundary
            assert [b.type for b in blocks[0]] == [dw.DYNAMIC, dw.STORED] and blocks[0][1].symbols == []
            assert len(blocks[1]) == 1 and len(bodies[1]) == 5 + SEG


# ----------------------------------------------------------------------------------------------------- Adler-32 --

@pytest.mark.gpu
@pytest.mark.parametrize("w,h,c,fbytes", [(1023, 128, 1, 131072), (255, 128, 4, 130688)])
def test_adler_sums_of_four_segments_of_ff(encode, w, h, c, fbytes):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w * c), indexing="ij")      # x counts the row's bytes
    px = ((-(xx + yy)) & 255).astype(np.uint8).reshape(h, w, c)
    _, raw = filter_rows(px)
    share = raw.count(0xFF) / len(raw)
    print(f"{w}x{h}x{c}: {100 * share:.2f} % of the filtered bytes are 0xFF")
    assert len(raw) == fbytes and len(segment_lengths(w, h, c)) == 4 and share > 0.99
    for q in ALL_LEVELS:
        data, z, raw2, bodies = encode(px, q)     # zlib's inflate checks the Adler-32; segment_chunks compares the value too
        assert raw2 == raw and len(bodies) == 4
        report(f"adler {w}x{h}x{c} q{q}", z, raw)


# ------------------------------------------------------------------------------------------------- filter ties --

def tie_table():
    """name -> picture.  What each one reaches is asserted by the test from filter_scores, not taken from its name."""
    t = {"zero": np.zeros((5, 9, 3), np.uint8)}
    for c in (1, 2, 3, 4):
        t[f"h1_c{c}"] = synth.photo(1, 31, c, index=50 + c)
        t[f"w1_c{c}"] = synth.photo(41, 1, c, index=60 + c)
        t[f"photo_c{c}"] = synth.photo(23, 31, c, index=70 + c)
    t["sub_up"] = np.array([[128, 16, 144, 32, 16, 80], [32, 80, 0, 96, 16, 176]], np.uint8).reshape(2, 6, 1)
    t["up_avg"] = np.array([[32, 56, 8, 32, 32, 80, 24, 16, 64, 40], [24, 80, 64, 24, 48, 88, 80, 72, 64, 56]], np.uint8).reshape(2, 5, 2)
    t["avg_paeth"] = np.array([[88, 24, 40, 88], [80, 48, 0, 48]], np.uint8).reshape(2, 4, 1)
    t["byte128_sub_paeth"] = np.array([[0, 0], [128, 128]], np.uint8).reshape(2, 2, 1)
    t["byte128_all"] = np.array([[0, 128, 128]], np.uint8).reshape(1, 3, 1)
    t["byte128_loser"] = np.array([[48, 225, 14, 142, 70], [176, 168, 78, 143, 66]], np.uint8).reshape(2, 5, 1)
    # a row of constant colour under a busy one: Sub alone is best
    busy = synth.photo(1, 40, 3, index=81)
    t["sub_alone"] = np.concatenate([busy, np.full((1, 40, 3), 90, np.uint8)])
    for rb, w, c in ((1, 1, 1), (2, 2, 1), (2, 1, 2), (3, 3, 1), (3, 1, 3), (63, 63, 1), (63, 21, 3), (64, 64, 1), (64, 16, 4), (64, 32, 2),
                     (65, 65, 1), (127, 127, 1), (129, 43, 3), (129, 129, 1)):
        assert rb == w * c
        t[f"rb{rb}_{w}x{c}"] = synth.photo(6, w, c, index=90 + rb + c)
    return t


def test_the_tie_table_reaches_every_tie_and_every_choice():
    t = tie_table()
    score = {k: filter_scores(px) for k, px in t.items()}
    choice = {k: filter_rows(px)[0] for k, px in t.items()}
    assert all(px.shape[0] <= 64 and px.shape[1] * px.shape[2] <= 129 for px in t.values())
    assert not score["zero"].any() and set(choice["zero"]) == {4}                       # four scores tie: the last filter wins
    for c in (1, 2, 3, 4):
        s = score[f"h1_c{c}"][0]
        assert s[0] == s[3] and s[0] < min(s[1], s[2]) and choice[f"h1_c{c}"][0] == 4     # one row: Sub == Paeth
        s = score[f"w1_c{c}"]
        assert (s[:, 1] == s[:, 3]).all() and (choice[f"w1_c{c}"] == 4).sum() > 20        # one column: Up == Paeth
    s = score["sub_up"][1]
    assert s[0] == s[1] < min(s[2], s[3]) and choice["sub_up"][1] == 2
    s = score["up_avg"][1]
    assert s[1] == s[2] < min(s[0], s[3]) and choice["up_avg"][1] == 3
    s = score["avg_paeth"][1]
    assert s[2] == s[3] < min(s[0], s[1]) and choice["avg_paeth"][1] == 4
    s = score["sub_alone"][1]
    assert s[0] < min(s[1:]) and choice["sub_alone"][1] == 1
    # byte 128 in the winning row: it has to come out as 128, and Sub == Paeth == |(i8)128| = 128 ties once more
    for k in ("byte128_sub_paeth", "byte128_all"):
        h, w, c = t[k].shape
        rows = np.frombuffer(filter_rows(t[k])[1], np.uint8).reshape(h, 1 + w * c)
        assert (rows[-1, 1:] == 128).any() and choice[k][-1] == 4, k
        s = score[k][-1]
        assert s[0] == s[3] == 128 < min(s[1], s[2])
    # byte 128 in a losing row: Up holds one and loses to Average by 32; counted as 0, as 127 - 128 or as -128 it would win
    s = score["byte128_loser"][1]
    up_row = (t["byte128_loser"][1, :, 0].astype(int) - t["byte128_loser"][0, :, 0]) & 255
    assert (up_row == 128).sum() == 1 and choice["byte128_loser"][1] == 3 and s[2] < s[1] < s[2] + 128 and s[2] < min(s[0], s[3])
    everything = np.concatenate(list(choice.values()))
    assert set(everything) == {1, 2, 3, 4}
    assert {px.shape[2] for px in t.values()} == {1, 2, 3, 4}
    assert {px.shape[1] * px.shape[2] for px in t.values()} >= {1, 2, 3, 63, 64, 65, 127, 129}


@pytest.mark.gpu
def test_filter_ties_go_to_the_later_filter(encode):
    for name, px in tie_table().items():
        try:
            encode(px, 75)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


# ------------------------------------------------------------------------------------------------------- levels --

@pytest.mark.gpu
def test_quality_thresholds_select_the_level(encode):
    px = synth.photo(30, 40, 3, index=44)
    flevel, files = {}, {}
    for q in (0, 49, 50, 84, 85, 100):
        data, z, raw, _ = encode(px, q)          # check_stream asserts FLEVEL = 3 below 50, 2 below 85, 0 from 85 on
        flevel[q], files[q] = z[1] >> 6, data
    assert flevel == {0: 3, 49: 3, 50: 2, 84: 2, 85: 0, 100: 0}
    assert flevel[49] != flevel[50] and files[49] != files[50]
    assert flevel[84] != flevel[85] and files[84] != files[85]
    assert files[0] == files[49] and files[50] == files[84] and files[85] == files[100]


# ------------------------------------------------------------------------------------------------ mixed batches --

def png_jobs():
    """(picture, quality): heights 1, 2, 3, 5 and 7 (four rows make one filter workgroup, so workgroups straddle pictures), unequal
    widths and channel counts, two multi-segment pictures of the geometry table, a 1 x 1; the three levels in turn."""
    pics = [synth.photo(1, 37, 3, index=101), synth.photo(2, 130, 1, index=102), synth.photo(3, 9, 4, index=103),
            synth.photo(5, 64, 2, index=104), smooth(910, 9, 4, seed=105), synth.photo(7, 301, 3, index=106),
            noise(8192, 2, 4, seed=107), synth.photo(1, 1, 4, index=108)]
    return [(px, ALL_LEVELS[i % 3]) for i, px in enumerate(pics)]


def same(a, b):
    if isinstance(a, bytes):
        return isinstance(b, bytes) and a == b
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("y", "u", "v", "a")) and a.has_alpha == b.has_alpha


@pytest.fixture(scope="module")
def solo(fl, gpu_state, encode):
    """The PNG jobs one at a time, each checked in full."""
    return [encode(px, q)[0] for px, q in png_jobs()]


@pytest.mark.gpu
def test_a_mixed_batch_in_two_orders(fl, gpu_state, solo):
    pngs = [(px, png_params(fl, q)) for px, q in png_jobs()]
    others = [(synth.photo(48, 64, 3, index=111), fl.make_params(quality=75, front_end=fl.FE_JPEG)),
              (synth.photo(40, 50, 3, index=112), fl.make_params(20, 10)),
              (synth.photo(24, 32, 3, index=113), fl.make_params(front_end=fl.FE_WEBP420)),
              (synth.photo(33, 47, 1, index=114), fl.make_params(quality=90, front_end=fl.FE_JPEG))]
    # PNG jobs with a neighbour of another kind after every second one
    entries, want = [], []
    for i, (job, alone) in enumerate(zip(pngs, solo)):
        entries.append(job)
        want.append(alone)
        if i % 2 == 1:
            entries.append(others[i // 2])
            want.append(gpu_state.process_pixels(*others[i // 2]))
    assert len(entries) == 12 and len({p.shape for p, _ in pngs}) == 8
    orders = [list(range(12)), [int(k) for k in np.random.default_rng(5).permutation(12)]]
    assert orders[0] != orders[1]
    for order in orders:
        outs = gpu_state.process_batch([entries[k][0] for k in order], [entries[k][1] for k in order])
        for k, out in zip(order, outs):
            assert same(want[k], out), f"entry {k} of order {order} differs from the same request alone"


@pytest.mark.gpu
def test_unequal_png_jobs_through_the_device_batch(fl, gpu_state, solo):
    import torch
    jobs = png_jobs()
    src = [torch.from_numpy(px).cuda() for px, _ in jobs]
    caps = [max_out_bytes(px.shape[1], px.shape[0], px.shape[2]) for px, _ in jobs]
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for cap in caps]
    gpu_state.process_batch_device([t.data_ptr() for t in src], [px.shape for px, _ in jobs], [png_params(fl, q) for _, q in jobs],
                                   [t.data_ptr() for t in dst], caps, stream=torch.cuda.current_stream().cuda_stream)
    res = gpu_state.batch_results()
    for i, (flags, nbytes) in enumerate(res):
        assert flags & fl.IMG_ENCODED and nbytes == len(solo[i]), i
        assert dst[i][:nbytes].cpu().numpy().tobytes() == solo[i], i


@pytest.mark.gpu
def test_unequal_png_jobs_from_16_threads(fl, gpu_state, solo):
    jobs = png_jobs()
    got, errors = [None] * 16, []

    def run(i):
        try:
            px, q = jobs[i % len(jobs)]
            got[i] = gpu_state.process_pixels(px, png_params(fl, q))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        assert got[i] == solo[i % len(jobs)], i
