"""One batch that holds every kind of output at once: all five encoders (three lossy WebP families in descending front-end order with
another between them, an alpha plane whose lossless scratch lies between the lossless pictures', both PNG and JPEG twice), both planar
front ends, plain pixels, and one encoder fed by the blur's scratch.  Every picture's scratch offsets are running totals over the
batch's jobs, so the test pins that a picture's output does not depend on its neighbours: in the given order and in a shuffled one,
through the host batch and the device batch, every output equals the same request sent alone."""
import random

import numpy as np
import pytest

import synth


def _alpha_picture(h, w):
    img = synth.photo(h, w, 4, index=7).copy()
    img[:, :, 3] = (np.add.outer(np.arange(h), np.arange(w)) * 5 % 256).astype(np.uint8)  # real alpha: a ramp, opaque nowhere in particular
    return img


def _requests(fl):
    mp = fl.make_params
    return [
        (synth.photo(15, 33, 3, index=1), mp(quality=1, front_end=fl.FE_WEBP_LOSSY_I4_AP_LF, segments=True)),
        (synth.photo(48, 64, 3, index=2), mp(quality=75, front_end=fl.FE_JPEG)),
        (_alpha_picture(48, 64), mp(quality=75, front_end=fl.FE_WEBP_LOSSY, alpha_vp8l=True, segments=True)),
        (synth.photo(17, 17, 2, index=3), mp(front_end=fl.FE_PNG)),
        (synth.photo(64, 64, 4, index=4), mp(quality=100, front_end=fl.FE_WEBP_LOSSLESS)),
        (synth.photo(32, 24, 3, index=5), mp(front_end=fl.FE_JFIF444)),
        (synth.photo(47, 33, 3, index=6), mp(front_end=fl.FE_WEBP420)),
        (synth.photo(30, 40, 3, index=8), mp(20, 15)),
        (synth.uniform(1, 1, 3, index=9), mp(quality=75, front_end=fl.FE_WEBP_LOSSY_AP)),
        (synth.photo(16, 16, 3, index=10), mp(quality=75, front_end=fl.FE_JPEG, blur_sigma=1.5)),
        (synth.uniform(1, 1, 4, index=11), mp(front_end=fl.FE_PNG)),
        (synth.uniform(1, 1, 4, index=12), mp(quality=100, front_end=fl.FE_WEBP_LOSSLESS)),
    ]


def _same(got, want):
    if isinstance(want, bytes):
        return isinstance(got, bytes) and got == want
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and np.array_equal(got, want)
    return (got.has_alpha == want.has_alpha and all(np.array_equal(getattr(got, k), getattr(want, k)) for k in "yuv") and
            (want.a is None) == (got.a is None) and (want.a is None or np.array_equal(got.a, want.a)))


@pytest.fixture(scope="module")
def solo(fl, gpu_state):
    """Every request sent alone: the reference of all the tests below (computed once, never changed)."""
    reqs = _requests(fl)
    return reqs, [gpu_state.process_pixels(img, p) for img, p in reqs]


@pytest.mark.gpu
def test_host_batch_equals_solo_in_both_orders(fl, gpu_state, solo):
    reqs, want = solo
    assert len(reqs) == 12 and len(want[1]) > 64  # (the first JPEG is longer than the capacity the last test cuts it to)
    orders = [list(range(len(reqs))), list(range(len(reqs)))]
    random.Random(20260).shuffle(orders[1])
    assert orders[1] != orders[0]
    for order in orders:
        got = gpu_state.process_batch([reqs[i][0] for i in order], [reqs[i][1] for i in order])
        for k, i in enumerate(order):
            assert _same(got[k], want[i]), (order, k, i)


def _device_batch(fl, gpu_state, reqs, caps):
    import torch
    src = [torch.from_numpy(np.ascontiguousarray(img)).cuda() for img, _ in reqs]
    dst = [torch.zeros(max(c, 1), dtype=torch.uint8, device="cuda") for c in caps]
    gpu_state.process_batch_device([t.data_ptr() for t in src], [img.shape for img, _ in reqs], [p for _, p in reqs],
                                   [t.data_ptr() for t in dst], caps, stream=torch.cuda.current_stream().cuda_stream)
    return dst


@pytest.mark.gpu
def test_device_batch_with_exact_capacities(fl, gpu_state, solo):
    reqs, want = solo
    plans = [fl.plan_output(p, img.shape[1], img.shape[0], img.shape[2]) for img, p in reqs]
    dst = _device_batch(fl, gpu_state, reqs, [int(pl.max_out_bytes) for pl in plans])
    res = gpu_state.batch_results()
    for i, ((img, p), (flags, nbytes)) in enumerate(zip(reqs, res)):
        if isinstance(want[i], bytes):
            assert flags & fl.IMG_ENCODED and not flags & fl.IMG_FRONTEND_PLANES and nbytes == len(want[i]), i
        elif p.front_end in (fl.FE_JFIF444, fl.FE_WEBP420):
            assert flags & fl.IMG_FRONTEND_PLANES and not flags & fl.IMG_ENCODED and nbytes == plans[i].out_bytes, i
        else:
            assert not flags & (fl.IMG_ENCODED | fl.IMG_FRONTEND_PLANES) and nbytes == plans[i].pixel_bytes, i
        assert _same(fl._split_output(dst[i].cpu().numpy(), plans[i], p.front_end, flags, nbytes), want[i]), i


@pytest.mark.gpu
def test_device_batch_with_the_first_jpeg_cut_to_64_bytes(fl, gpu_state, solo):
    """A destination below the plan's out_bytes is refused when the batch is planned, before anything is enqueued: the wrapper raises
    out of process_batch_device, so there are no result words to read -- the raise and its status are what can be asserted."""
    reqs, want = solo
    caps = [int(fl.plan_output(p, img.shape[1], img.shape[0], img.shape[2]).max_out_bytes) for img, p in reqs]
    caps[1] = 64
    with pytest.raises(fl.FanlinError) as e:
        _device_batch(fl, gpu_state, reqs, caps)
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL


@pytest.mark.gpu
def test_host_batch_with_the_first_jpeg_cut_to_64_bytes(fl, gpu_state, solo):
    """The host batch learns a stream's length only after the batch has run: the call reports buffer-too-small, that picture's length
    is 0, and every other picture is delivered."""
    import ctypes as C
    reqs, want = solo
    n = len(reqs)
    imgs = [np.ascontiguousarray(img) for img, _ in reqs]
    plans = [fl.plan_output(p, a.shape[1], a.shape[0], a.shape[2]) for a, (_, p) in zip(imgs, reqs)]
    outs = [np.zeros(64 if i == 1 else max(int(pl.max_out_bytes), 1), np.uint8) for i, pl in enumerate(plans)]
    srcs = (fl.flgpu_image * n)(*[fl.flgpu_image(a.ctypes.data, a.nbytes, a.shape[1], a.shape[0], a.shape[2], 0) for a in imgs])
    dsts = (fl.flgpu_image * n)(*[fl.flgpu_image(o.ctypes.data, o.nbytes, 0, 0, 0, 0) for o in outs])
    ps = (fl.flgpu_params * n)(*[p for _, p in reqs])
    assert fl.load_library().flgpu_transform_batch(gpu_state._ctx, n, srcs, ps, dsts) == fl.ERR_BUFFER_TOO_SMALL
    for i in range(n):
        if i == 1:
            assert dsts[i].bytes == 0 and dsts[i].flags & fl.IMG_ENCODED
        else:
            assert _same(fl._split_output(outs[i], plans[i], reqs[i][1].front_end, dsts[i].flags, dsts[i].bytes), want[i]), i
