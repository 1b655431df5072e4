"""FLGPU_FEO_JPEG_420 on the device: FLGPU_FE_JPEG with Cb and Cr halved in both directions.  Every file equals the model's
(tests/jpeg_420_model.py, which tests/test_jpeg_420_host.py judges by Pillow, by the oracle's entropy decoder and against libjpeg), with
and without FLGPU_FEO_JPEG_OPTIMIZE, on every entry path, alone or in a mixed batch; the counters tell the route; without the option
every byte is the oracle encoder's."""
import threading

import numpy as np
import pytest

import jpeg_420_cases as cases
import jpeg_420_model as m
import jpeg_opt_model as jm
import synth

Q = "w=300&h=200&quality=75"


def _n420(st):
    return st.debug_get("jpeg_420")


def _nopt(st):
    return st.debug_get("jpeg_optimized")


def _cap(img):
    return img.shape[0] * img.shape[1] * 16 + 8192


def _p(fl, q, optimize=False, s420=True, **kw):
    return fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_420=s420, jpeg_optimize=optimize, **kw)


def _first_difference(a, b):
    return f"{len(a)} vs {len(b)} bytes, first difference at {next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_corpus_file_equals_the_model_and_the_counters_tell_the_route(fl, gpu_state, oracle, name):
    img, q = cases.get(name)
    h, w, c = img.shape
    want, _ = cases.model(oracle, name)
    n0, o0 = _n420(gpu_state), _nopt(gpu_state)
    data = gpu_state.process_pixels(img, _p(fl, q), capacity=_cap(img))
    assert (_n420(gpu_state), _nopt(gpu_state)) == (n0 + 1, o0)
    assert len(data) <= int(fl.plan_output(_p(fl, q), w, h, c).max_out_bytes)
    assert data == want, _first_difference(data, want)
    # with FLGPU_FEO_JPEG_OPTIMIZE as well
    want_opt, info = cases.model(oracle, name, True)
    both = gpu_state.process_pixels(img, _p(fl, q, True), capacity=_cap(img))
    assert (_n420(gpu_state), _nopt(gpu_state)) == (n0 + 2, o0 + int(info["optimized"]))
    print(name, len(oracle.jpeg_encode(img, q)), "->", len(data), "->", len(both), "optimized" if info["optimized"] else "standard")
    assert both == want_opt, _first_difference(both, want_opt)
    assert (len(both) < len(data)) if info["optimized"] else (both == data)
    with gpu_state.switches(jpeg_optimize_fallback=1):
        assert gpu_state.process_pixels(img, _p(fl, q, True), capacity=_cap(img)) == want, "the fallback is the 4:2:0 Annex K file"
    assert (_n420(gpu_state), _nopt(gpu_state)) == (n0 + 3, o0 + int(info["optimized"]))
    # without the new bit: the oracle encoder's file, and the counter stands
    plain = gpu_state.process_pixels(img, _p(fl, q, s420=False), capacity=_cap(img))
    assert plain == oracle.jpeg_encode(img, q) and _n420(gpu_state) == n0 + 3


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state, oracle):
    names = ["photo_300x200_q100", "photo_1x1_c3_q75", "row_9_mcus_q75", "quadrants_16x16_q75", "photo_9x7_c4_q1", "noise_32x32_q100", "photo_17x17_c2_q50",
             "row_16_mcus_q1", "flat_24x16_q75", "photo_83x61_c4_q75", "grey_33x17_c1_q75", "checker_yb_64x32_q100"]
    images, params, kinds, labels = [], [], [], []
    for k, n in enumerate(names):          # 4:2:0 and 4:2:0 + _OPTIMIZE, alternating; the large picture both ways
        for optimize in ((False, True) if n == "photo_300x200_q100" else (bool(k & 1),)):
            img, q = cases.get(n)
            images.append(img); params.append(_p(fl, q, optimize)); kinds.append("420o" if optimize else "420"); labels.append(n)
    # plain and _OPTIMIZE pictures without the bit (two of them the same pictures as 4:2:0 neighbours), a PNG and a lossy WebP picture that carry it
    photo = synth.photo(61, 83, 4, index=5)
    big, row = cases.get("photo_300x200_q100")[0], cases.get("row_9_mcus_q75")[0]
    images += [big, row, photo, big, photo, photo]
    params += [_p(fl, 100, s420=False), _p(fl, 75, True, s420=False), _p(fl, 30, s420=False), _p(fl, 100, True, s420=False),
               fl.make_params(quality=75, front_end=fl.FE_PNG, jpeg_420=True), fl.make_params(quality=75, front_end=fl.FE_WEBP_LOSSY, jpeg_420=True)]
    kinds += ["jpeg", "opt", "jpeg", "opt", "png", "webp"]
    labels += [None] * 6
    order = np.random.default_rng(29).permutation(len(images))
    images, params, kinds, labels = ([x[i] for i in order] for x in (images, params, kinds, labels))
    alone = [gpu_state.process_pixels(i, p) for i, p in zip(images, params)]
    n0 = _n420(gpu_state)
    outs = gpu_state.process_batch(images, params)
    assert _n420(gpu_state) - n0 == sum(k in ("420", "420o") for k in kinds)
    for k, (got, want) in enumerate(zip(outs, alone)):
        assert isinstance(got, bytes) and got == want, (k, kinds[k], labels[k])
        if kinds[k] in ("420", "420o"):
            assert got == cases.model(oracle, labels[k], kinds[k] == "420o")[0], (labels[k], kinds[k])
        elif kinds[k] == "jpeg":
            assert got == oracle.jpeg_encode(images[k], params[k].quality), k
        elif kinds[k] == "opt":
            assert got == jm.encode(oracle, images[k], params[k].quality)[0], k
        else:
            assert got == gpu_state.process_pixels(images[k], fl.make_params(quality=75, front_end=params[k].front_end)), kinds[k]


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state, oracle):
    import torch
    name = "photo_83x61_c4_q75"
    img, q = cases.get(name)
    alone, both, plain = cases.model(oracle, name)[0], cases.model(oracle, name, True)[0], oracle.jpeg_encode(img, q)
    p, pb = _p(fl, q), _p(fl, q, True)
    # 16 concurrent callers through the queue, alternating the bit
    got, errors = [None] * 16, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(img, _p(fl, q, s420=(i % 2 == 0)))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        assert got[i] == (alone if i % 2 == 0 else plain), i
    # flgpu_transform_batch
    assert gpu_state.process_batch([img] * 4, [p, pb, p, pb]) == [alone, both, alone, both]
    # flgpu_transform_batch_device + flgpu_batch_results
    h, w, c = img.shape
    src = [torch.from_numpy(img).cuda() for _ in range(2)]
    cap = int(fl.plan_output(p, w, h, c).max_out_bytes)
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    before = _n420(gpu_state)
    gpu_state.process_batch_device([t.data_ptr() for t in src], [(h, w, c)] * 2, p, [t.data_ptr() for t in dst], [cap] * 2,
                                   stream=torch.cuda.current_stream().cuda_stream)
    for i, (flags, nbytes) in enumerate(gpu_state.batch_results()):
        assert flags & fl.IMG_ENCODED and dst[i][:nbytes].cpu().numpy().tobytes() == alone
    assert _n420(gpu_state) - before == 2
    # a second context in the process, and a context of two shards (both on device 0)
    with fl.State(device=0) as other:
        assert other.process_pixels(img, p) == alone and other.process_pixels(img, pb) == both and other.debug_get("jpeg_420") == 2
    with fl.State(devices=[0, 0]) as two:
        assert two.process_batch([img] * 4, [p, pb, pb, p]) == [alone, both, both, alone]
        assert two.process_pixels(img, p) == alone and two.debug_get("jpeg_420") == 5


@pytest.mark.gpu
def test_the_query_level_route_and_the_flagship_request(fl, gpu_state, oracle):
    big = synth.photo(1080, 1920, 3, index=3)
    new = fl.ENCODE_JPEG_420
    pixels = gpu_state.process_pixels(big, fl.make_params(300, 200))
    want, want_both, old = m.encode(oracle, pixels, 75)[0], m.encode(oracle, pixels, 75, True)[0], oracle.jpeg_encode(pixels, 75)
    assert len(want_both) < len(want) < len(old)
    assert gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_JPEG, jpeg_420=True)) == want
    before = _n420(gpu_state)
    mime, kind, body = gpu_state.process_image(big, Q, fl.Format(new), input_format=fl.IN_JPEG)
    assert (mime, kind) == ("image/jpeg", fl.RESULT_JPEG_STREAM) and body == want
    assert gpu_state.process_image(big, Q, fl.Format(new | fl.ENCODE_JPEG_OPTIMIZE), input_format=fl.IN_JPEG)[2] == want_both
    assert gpu_state.process_image(big, Q, fl.Format(new | fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY), input_format=fl.IN_JPEG)[2] == want, "webp accepted, not asked for"
    assert _n420(gpu_state) - before == 3
    # without the bit: today's file; with it on every other arm: what the arm gives without it
    assert gpu_state.process_image(big, Q, fl.Format(0), input_format=fl.IN_JPEG)[2] == old
    for query, content, fmt in ((Q, fl.ENCODE_PNG, fl.IN_PNG), (Q + "&webp=true", fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY, fl.IN_JPEG), (Q, 0, fl.IN_OTHER)):
        a = gpu_state.process_image(big, query, fl.Format(content), input_format=fmt)
        b = gpu_state.process_image(big, query, fl.Format(content | new), input_format=fmt)
        assert a[:2] == b[:2] and (a[2] == b[2] if isinstance(a[2], bytes) else np.array_equal(a[2], b[2])), (query, fmt)
    assert _n420(gpu_state) - before == 3
    # a JPEG file through flgpu_process_jpeg with the accept bit: decoded, resized and coded on the device
    data = oracle.jpeg_encode(synth.photo(120, 200, 3, index=9), 85)
    small = gpu_state.process_pixels(gpu_state.decode_jpeg(data), fl.make_params(64, 48))
    mime, kind, body = gpu_state.process_jpeg(data, "w=64&h=48&quality=50", fl.Format(new))
    assert (mime, kind) == ("image/jpeg", fl.RESULT_JPEG_STREAM) and body == m.encode(oracle, small, 50)[0]
    assert gpu_state.process_jpeg(data, "w=64&h=48&quality=50", fl.Format(new | fl.ENCODE_JPEG_OPTIMIZE))[2] == m.encode(oracle, small, 50, True)[0]
    assert gpu_state.process_jpeg(data, "w=64&h=48&quality=50")[2] == oracle.jpeg_encode(small, 50)
    a = gpu_state.process_jpeg(data, "w=64&h=48&webp=true&quality=50", fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY))
    assert a == gpu_state.process_jpeg(data, "w=64&h=48&webp=true&quality=50", fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | new))
    assert _n420(gpu_state) - before == 5


@pytest.mark.gpu
def test_a_420_file_from_the_device_decodes_on_the_device_to_the_oracles_pixels(fl, gpu_state, oracle):
    for name in ("photo_83x61_c4_q75", "photo_17x17_c2_q50", "photo_300x200_q75"):
        img, q = cases.get(name)
        for optimize in (False, True):
            data = gpu_state.process_pixels(img, _p(fl, q, optimize))
            assert data == cases.model(oracle, name, optimize)[0]
            assert np.array_equal(gpu_state.decode_jpeg(data), oracle.jpeg_decode(data)), (name, optimize)


@pytest.mark.gpu
def test_a_destination_one_byte_short(fl, gpu_state, oracle):
    img, q = cases.get("photo_83x61_c4_q75")
    for optimize in (False, True):
        full = cases.model(oracle, "photo_83x61_c4_q75", optimize)[0]
        with pytest.raises(fl.FanlinError) as e:
            gpu_state.process_pixels(img, _p(fl, q, optimize), capacity=-(len(full) - 1))
        assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
        assert gpu_state.process_pixels(img, _p(fl, q, optimize), capacity=-len(full)) == full
