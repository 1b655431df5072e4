"""FLGPU_FE_WEBP_LOSSLESS where the corpus of test_webp_lossless.py never goes (csrc/fl_webpll.hip): runs that start and end on the
first and last pixel of a tile (4096) and of a thread (16), forced references of 4096 against the tile's edge, tiles wholly inside a
run, pictures of 257 tiles (the second round of the per-picture carry and scan kernels), the code kernel's branches (simple codes, one
used code-length symbol, the folds to 15 and to 7 bits, all 24 length symbols), the header's 14-bit fields at 16384, unequal jobs in
one launch, and destinations off 4-byte alignment.

The pictures are tests/vp8l_cases.py's, each with the property that makes it an edge.  Host half: the property holds and the system's
libwebp decodes the model's file (tests/vp8l_model.py) to the picture.  Device half, for the identity request: the FE_NONE pixels
are the picture, the stream is the model's byte for byte, libwebp decodes it to the picture, and it fits max_out_bytes."""
import struct
import threading

import numpy as np
import pytest

import synth
import vp8l_cases as vc
import vp8l_model as vm


# ---------------------------------------------------------------------------------------------------- host side --

def test_from_residuals_is_the_inverse_of_residuals():
    rng = np.random.default_rng(1)
    for w, h in ((1, 1), (7, 1), (1, 7), (13, 9)):
        res = rng.integers(0, 256, (w * h, 4), dtype=np.uint8)
        for c in (4, 3, 2, 1):
            r = res.copy()
            if c in (1, 3):
                r[:, 0] = 0
            if c < 3:
                r[:, 1] = r[:, 3] = 0
            px = vc.from_residuals(r, w, h, c)
            assert px.shape == (h, w, c) and np.array_equal(vm.residuals(px), r), (w, h, c)
    with pytest.raises(AssertionError):
        vc.from_residuals(res, 13, 9, 3)


@pytest.mark.parametrize("name", vc.NAMES)
def test_the_case_is_the_edge_it_says_and_the_model_is_valid(name):
    assert vm.have_decoder(), "libwebp (or Pillow with WebP) is needed to check the streams"
    vc.check(name)
    px, data = vc.get(name), vc.model(name)
    h, w, c = px.shape
    assert len(data) <= vm.max_out_bytes(w, h)
    assert np.array_equal(vm.decode_rgba(data), vm.into_rgba8(px))


def test_the_run_pictures_hold_the_whole_grid_and_the_three_tile_edges():
    held = {p for b in vc.RUN_PICTURES for p in b}
    assert held >= {(s, L) for s in (0, 1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192) for L in (1, 2, 3, 4096, 4097, 4098, 8193, 8194)}
    assert held >= {(s, L - 1) for s in vc.RUN_STARTS for L in (4096, 4097, 4098, 8193, 8194)}, "the lengths read as pixel counts"
    assert {(e - L) % 16 for e in vc.RUN_ENDS for L in (1, 2, 3)} >= {12, 13, 14, 15} and {e % 16 for e in vc.RUN_ENDS} >= {15, 0}
    forced, ends, inside = {}, {}, {}
    for j in range(len(vc.RUN_PICTURES)):
        for kind in ("own", "zero"):
            name = "runs%02d_%s" % (j, kind)
            m, flag = vc.flags_of(vc.get(name))
            if len(vc.forced_reference_ends_a_tile(m, flag)):
                forced[name] = True
            if len(vc.run_ends_on_a_tile(m, flag)):
                ends[name] = True
            if vc.tiles_inside_a_run(m, flag):
                inside[name] = True
    # each of the three with the run's own tuple and with the zero tuple (a missing neighbour reads as zero)
    for found in (forced, ends, inside):
        assert any(n.endswith("own") for n in found) and any(n.endswith("zero") for n in found), found
    j = vc.picture_of((4095, 8193))
    m, flag = vc.flags_of(vc.get("runs%02d_own" % j))
    assert list(vc.forced_reference_ends_a_tile(m, flag)) == [8191] and vc.tiles_inside_a_run(m, flag) == [2]
    m, flag = vc.flags_of(vc.get("runs%02d_own" % vc.picture_of((4092, 3))))
    assert 4095 in vc.run_ends_on_a_tile(m, flag)
    assert {vc.get(n).shape[2] for n in vc.NAMES} == {1, 2, 3, 4}


def test_the_alignment_cases_cover_every_tail_and_both_parities():
    n = [struct.unpack("<I", vc.model(name)[16:20])[0] for name in vc.ALIGNMENT_CASES]
    assert {x % 4 for x in n} == {0, 1, 2, 3} and {x < 16 for x in n} == {True, False}
    assert all(len(vc.model(name)) == 20 + x + (x & 1) for name, x in zip(vc.ALIGNMENT_CASES, n))
    # a device batch wants 4 w h bytes of every destination, whatever its front end: these files are no shorter, so a capacity of
    # exactly the file's length is one the library takes
    assert all(len(vc.model(name)) >= 4 * vc.get(name).shape[0] * vc.get(name).shape[1] for name in vc.ALIGNMENT_CASES)


# -------------------------------------------------------------------------------------------------- device side --

def lossless(fl):
    return fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", vc.NAMES)
def test_the_stream_is_the_models(fl, gpu_state, name):
    assert vm.have_decoder(), "libwebp (or Pillow with WebP) is needed to check the streams"
    px = vc.get(name)
    h, w, c = px.shape
    seen = gpu_state.process_pixels(px, fl.make_params())
    assert np.array_equal(seen, px), "FE_NONE without a size is the identity"
    data = gpu_state.process_pixels(px, lossless(fl))
    assert isinstance(data, bytes) and len(data) <= vm.max_out_bytes(w, h)
    want = vc.model(name)
    if data != want:
        k = next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want)))
        raise AssertionError(f"{name}: {len(data)} bytes against the model's {len(want)}, first difference at byte {k}")
    assert np.array_equal(vm.decode_rgba(data), vm.into_rgba8(px))


# ------------------------------------------------------------------------------------------------ unequal jobs --

JOB_CASES = ("one_pixel_0", "line_4096x1_run", "line_4097x1_literal", "line_8193x1_zero_run", None, "tiles257_noise_band")
JOB_TILES = (1, 1, 2, 3, 15, 257)


def job_pictures():
    return [np.random.default_rng(300).integers(0, 256, (200, 300, 4), dtype=np.uint8) if n is None else vc.get(n) for n in JOB_CASES]


def test_the_jobs_have_the_tile_counts_they_are_there_for():
    assert tuple(-(-px.shape[0] * px.shape[1] // vc.TILE) for px in job_pictures()) == JOB_TILES


def same(a, b):
    if isinstance(a, bytes):
        return isinstance(b, bytes) and a == b
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("y", "u", "v", "a")) and a.has_alpha == b.has_alpha


@pytest.fixture(scope="module")
def entries(fl, gpu_state):
    """(picture, params, the output of that request alone), by ascending size of the lossless jobs, a neighbour of another kind
    behind each of them; the lossless outputs are the model's."""
    others = [(synth.photo(48, 64, 3, index=111), fl.make_params(quality=75, front_end=fl.FE_JPEG)),
              (synth.photo(40, 50, 3, index=112), fl.make_params(quality=75, front_end=fl.FE_PNG)),
              (synth.photo(40, 50, 3, index=113), fl.make_params(20, 10)),
              (synth.photo(24, 32, 4, index=114), fl.make_params(front_end=fl.FE_WEBP420)),
              (synth.photo(33, 47, 3, index=115), fl.make_params(quality=80, front_end=fl.FE_WEBP_LOSSY)),
              (synth.photo(9, 11, 1, index=116), fl.make_params())]
    out = []
    for name, px, other in zip(JOB_CASES, job_pictures(), others):
        alone = gpu_state.process_pixels(px, lossless(fl))
        assert alone == (vc.model(name) if name else vm.encode(px))
        out.append((px, lossless(fl), alone))
        out.append((other[0], other[1], gpu_state.process_pixels(*other)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_unequal_jobs_among_other_entries(fl, gpu_state, entries, order):
    es = entries if order == "ascending" else entries[::-1]
    outs = gpu_state.process_batch([e[0] for e in es], [e[1] for e in es])
    for k, (e, out) in enumerate(zip(es, outs)):
        assert same(e[2], out), f"entry {k} ({order}) differs from the same request alone"


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_unequal_jobs_through_the_device_batch(fl, gpu_state, entries, order):
    import torch
    es = entries if order == "ascending" else entries[::-1]
    src = [torch.from_numpy(np.array(e[0])).cuda() for e in es]
    plans = [fl.plan_output(e[1], e[0].shape[1], e[0].shape[0], e[0].shape[2]) for e in es]
    caps = [int(pl.max_out_bytes) for pl in plans]
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for cap in caps]
    gpu_state.process_batch_device([t.data_ptr() for t in src], [e[0].shape for e in es], [e[1] for e in es],
                                   [t.data_ptr() for t in dst], caps, stream=torch.cuda.current_stream().cuda_stream)
    res = gpu_state.batch_results()
    for k, (e, (flags, nbytes)) in enumerate(zip(es, res)):
        out = fl._split_output(dst[k].cpu().numpy(), plans[k], e[1].front_end, flags, nbytes)
        assert same(e[2], out), f"entry {k} ({order}) differs from the same request alone"


@pytest.mark.gpu
def test_unequal_jobs_from_16_threads(fl, gpu_state, entries):
    got, errors = [None] * 16, []

    def run(i):
        try:
            e = entries[i % len(entries)]
            got[i] = gpu_state.process_pixels(e[0], e[1])
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        assert same(entries[i % len(entries)][2], got[i]), i


# ------------------------------------------------------------------------------------- destinations off alignment --

FILL, FRONT = 0xA5, 8      # every buffer is FRONT + k + capacity + FRONT bytes of FILL; the destination starts FRONT + k bytes in


def _unaligned_batch(fl, gpu_state, capacity_of):
    """One device batch: every alignment case at dst = base + k for k = 0 .. 3.  Returns [(name, k, capacity, buffer, flags, bytes)]
    and the status of flgpu_batch_results."""
    import torch
    jobs = [(name, k) for name in vc.ALIGNMENT_CASES for k in range(4)]
    pics = {name: torch.from_numpy(np.array(vc.get(name))).cuda() for name in vc.ALIGNMENT_CASES}
    caps = [capacity_of(name, k) for name, k in jobs]
    bufs = [torch.full((FRONT + k + cap + FRONT,), FILL, dtype=torch.uint8, device="cuda") for (name, k), cap in zip(jobs, caps)]
    assert all(b.data_ptr() % 4 == 0 for b in bufs)
    gpu_state.process_batch_device([pics[name].data_ptr() for name, k in jobs], [vc.get(name).shape for name, k in jobs], lossless(fl),
                                   [b.data_ptr() + FRONT + k for b, (name, k) in zip(bufs, jobs)], caps,
                                   stream=torch.cuda.current_stream().cuda_stream)
    srcs, dsts, ps = gpu_state._keep
    rc = fl.load_library().flgpu_batch_results(gpu_state._ctx, len(dsts), dsts)
    return [(name, k, cap, b.cpu().numpy(), d.flags, d.bytes) for (name, k), cap, b, d in zip(jobs, caps, bufs, dsts)], rc


def _check_delivered(fl, name, k, buf, flags, nbytes):
    want = vc.model(name)
    at = FRONT + k
    assert flags & fl.IMG_ENCODED and nbytes == len(want), (name, k, nbytes)
    assert buf[at:at + nbytes].tobytes() == want, (name, k)
    assert (buf[:at] == FILL).all(), f"{name}: bytes in front of dst + {k} were written"
    assert (buf[at + nbytes:] == FILL).all(), f"{name}: bytes behind the file at dst + {k} were written"


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", ["max_out_bytes", "exact"])
def test_destinations_off_alignment(fl, gpu_state, capacity):
    def capacity_of(name, k):
        h, w, _ = vc.get(name).shape
        return vm.max_out_bytes(w, h) if capacity == "max_out_bytes" else len(vc.model(name))
    out, rc = _unaligned_batch(fl, gpu_state, capacity_of)
    assert rc == fl.OK
    for name, k, cap, buf, flags, nbytes in out:
        _check_delivered(fl, name, k, buf, flags, nbytes)


@pytest.mark.gpu
def test_one_byte_short_off_alignment_leaves_the_buffer_alone(fl, gpu_state):
    short = {(name, (i + 1) % 4) for i, name in enumerate(vc.ALIGNMENT_CASES)}      # one entry of every case, at k = 1, 2, 3, 0, ...
    out, rc = _unaligned_batch(fl, gpu_state, lambda name, k: len(vc.model(name)) - ((name, k) in short))
    assert rc == fl.ERR_BUFFER_TOO_SMALL
    for name, k, cap, buf, flags, nbytes in out:
        if (name, k) in short:
            assert nbytes == 0 and (buf == FILL).all(), f"{name}: a file one byte too long for dst + {k} left bytes behind"
        else:
            _check_delivered(fl, name, k, buf, flags, nbytes)
