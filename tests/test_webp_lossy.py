"""FLGPU_FE_WEBP_LOSSY on the device: the finished lossy WebP file for the WebP arm below quality 100 (reference
src/handler.rs:293-297).  Every file equals the restated encoder's (tests/vp8_model.py) on the planes the same request returns with
FLGPU_FE_WEBP420 -- which libwebp decodes to exactly the model's reconstruction (tests/test_webp_lossy_host.py) -- on every
entry path, alone or in a mixed batch."""
import io
import math
import threading

import numpy as np
import pytest

import png_write
import synth
import vp8_cases
import vp8_lib
import vp8_model as vm
import vp8l_model
import webp_lib
from test_webp_lossy_host import PSNR_DEFICIT_BAR_DB

Q = "w=300&h=200&webp=true&quality=75"


def _model_of(fl, st, img, key, **kw):
    """The model's file for the request: its planes are what the same request returns with FE_WEBP420."""
    pl = st.process_pixels(img, fl.make_params(front_end=fl.FE_WEBP420, **kw))
    return vp8_cases.model(key, pl.y, pl.u, pl.v, kw["quality"], pl.a if pl.has_alpha else None)[0], pl


@pytest.fixture(scope="module")
def big():
    return synth.photo(1080, 1920, 3, index=3)


@pytest.mark.gpu
def test_every_corpus_file_equals_the_model(fl, gpu_state):
    bad = []
    for name, img, q in vp8_cases.corpus():
        data = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY))
        want, pl = _model_of(fl, gpu_state, img, "dev:" + name, quality=q)
        h, w = img.shape[:2]
        assert isinstance(data, bytes) and len(data) <= vm.max_out_bytes(w, h), name
        assert pl.has_alpha == name.endswith("_a") == (data[12:16] == b"VP8X"), name
        if data != want:
            bad.append(name)
    assert not bad, bad
    assert gpu_state.stats()["frontend_launches"] > 0 and gpu_state.debug_get("webp_lossy_ns") > 0


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state, big):
    corpus = {name: (img, q) for name, img, q in vp8_cases.corpus()}
    picks = ["photo_1x1_q75_a", "photo_300x200_q75", "photo_17x17_q30_a", "noise_64x48_q99", "photo_16x144_q99", "flat_64x48_q75",
             "photo_15x33_q1", "photo_128x16_q75_a"]
    images = [corpus[n][0] for n in picks]
    params = [fl.make_params(quality=corpus[n][1], front_end=fl.FE_WEBP_LOSSY) for n in picks]
    small = big[:500, :700].copy()
    for fe, q in ((fl.FE_JPEG, 75), (fl.FE_PNG, 75), (fl.FE_WEBP_LOSSLESS, 100), (fl.FE_NONE, 75), (fl.FE_WEBP420, 75), (fl.FE_WEBP_LOSSY, 30)):
        images.append(small)
        params.append(fl.make_params(300, 200, quality=q, front_end=fe))
    alone = [gpu_state.process_pixels(i, p) for i, p in zip(images, params)]
    outs = gpu_state.process_batch(images, params)
    for k, (got, want) in enumerate(zip(outs, alone)):
        fe = params[k].front_end
        if fe == fl.FE_NONE:
            assert np.array_equal(got, want), k
        elif fe == fl.FE_WEBP420:
            assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in "yuva") and got.has_alpha == want.has_alpha, k
        else:
            assert isinstance(got, bytes) and got == want, (k, fe)
    for k, n in enumerate(picks):
        assert outs[k] == _model_of(fl, gpu_state, images[k], "dev:" + n, quality=corpus[n][1])[0], n


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state, big):
    import torch
    p = fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY)
    alone = gpu_state.process_pixels(big, p)
    assert alone == _model_of(fl, gpu_state, big, "dev:big", w=300, h=200, quality=75)[0]
    # 16 concurrent callers through the queue, mixed with JPEG and planes
    kinds = [fl.FE_WEBP_LOSSY, fl.FE_JPEG, fl.FE_WEBP420, fl.FE_WEBP_LOSSY]
    want_jpeg = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_JPEG))
    got, errors = [None] * 16, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=kinds[i % 4]))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        if kinds[i % 4] == fl.FE_WEBP_LOSSY:
            assert got[i] == alone, i
        elif kinds[i % 4] == fl.FE_JPEG:
            assert got[i] == want_jpeg, i
    # flgpu_transform_batch
    assert all(o == alone for o in gpu_state.process_batch([big] * 3, [p] * 3))
    # flgpu_transform_batch_device + flgpu_batch_results
    src = [torch.from_numpy(big).cuda() for _ in range(2)]
    cap = int(fl.plan_output(p, 1920, 1080, 3).max_out_bytes)
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    gpu_state.process_batch_device([t.data_ptr() for t in src], [(1080, 1920, 3)] * 2, p, [t.data_ptr() for t in dst], [cap] * 2,
                                   stream=torch.cuda.current_stream().cuda_stream)
    for i, (flags, nbytes) in enumerate(gpu_state.batch_results()):
        assert flags & fl.IMG_ENCODED and dst[i][:nbytes].cpu().numpy().tobytes() == alone
    # a context of two shards (both on device 0)
    with fl.State(devices=[0, 0]) as two:
        assert all(o == alone for o in two.process_batch([big] * 4, [p] * 4))
        assert two.process_pixels(big, p) == alone
    # State::process_image with the opt-in bit: negotiated, and a WebP source that stays WebP
    accept = fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY)
    for q, fmt, content in ((Q, fl.IN_PNG, accept), (Q, fl.IN_JPEG, accept), ("w=300&h=200&quality=75", fl.IN_WEBP, fl.Format(fl.ENCODE_WEBP_LOSSY)),
                            ("w=300&h=200&webp=true", fl.IN_OTHER, accept)):
        mime, kind, body = gpu_state.process_image(big, q, content, input_format=fmt)
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body == alone, q
    # without the bit: the planes, byte for byte what FE_WEBP420 gives
    mime, kind, planes = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP), input_format=fl.IN_PNG)
    want = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP420))
    assert kind == fl.RESULT_WEBP_PLANES and all(np.array_equal(getattr(planes, f), getattr(want, f)) for f in "yuva")


@pytest.mark.gpu
def test_file_sources_give_the_stream(fl, gpu_state):
    from PIL import Image
    img = synth.photo(360, 640, 3, index=41)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=90)
    accept = fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY)
    p = fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY)
    files = ((gpu_state.process_jpeg, gpu_state.process_jpeg_pixels, b.getvalue()),
             (gpu_state.process_png, gpu_state.process_png_pixels, png_write.write_png(img, 2, filters=[y % 5 for y in range(360)])),
             (gpu_state.process_webp, gpu_state.process_webp_pixels, vp8l_model.encode(img)))
    for process, process_pixels, data in files:
        mime, kind, body = process(data, Q, accept)
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body[:4] == b"RIFF", process.__name__
        assert body == process_pixels(data, p), process.__name__
        assert process(data, Q, fl.Format(fl.ACCEPT_WEBP))[1] == fl.RESULT_WEBP_PLANES
    # the PNG and the lossless WebP decode to the pixels the files were written from: the same stream as from those pixels
    direct = gpu_state.process_pixels(img, p)
    assert gpu_state.process_png(files[1][2], Q, accept)[2] == direct and gpu_state.process_webp(files[2][2], Q, accept)[2] == direct


@pytest.mark.gpu
def test_too_small_destinations(fl, gpu_state):
    name, img, q = vp8_cases.corpus()[2]
    p = fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY)
    full = gpu_state.process_pixels(img, p)
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # a batch with one too-small stream: no bytes claimed for it, its neighbours delivered intact
    lib = fl.load_library()
    cap = int(fl.plan_output(p, 300, 200, 4).max_out_bytes)
    caps = [cap, len(full) - 1, cap]
    outs = [np.zeros(cp, np.uint8) for cp in caps]
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(img.ctypes.data, img.nbytes, 300, 200, 4, 0) for _ in range(3)])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(o.ctypes.data, o.nbytes, 0, 0, 0, 0) for o in outs])
    ps = (fl.flgpu_params * 3)(p, p, p)
    assert lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts) == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0
    for i in (0, 2):
        assert outs[i][:dsts[i].bytes].tobytes() == full


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)


@pytest.mark.gpu
def test_one_request_end_to_end(fl, gpu_state, big):
    from PIL import Image
    mime, kind, body = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY), input_format=fl.IN_PNG)
    assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM)
    im = Image.open(io.BytesIO(body))
    assert im.format == "WEBP" and im.size == (300, 200)
    im.load()
    pl = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP420))
    ours = vp8_lib.decode_yuv(body)[0]
    theirs = vp8_lib.decode_yuv(webp_lib.encode_planes(pl.y, pl.u, pl.v, 75))[0]
    deficit = _psnr(theirs, pl.y) - _psnr(ours, pl.y)
    print(f"Y-PSNR {_psnr(ours, pl.y):.2f} dB, libwebp's encode of the same planes {_psnr(theirs, pl.y):.2f} dB, {len(body)} bytes")
    assert deficit <= PSNR_DEFICIT_BAR_DB
