"""FLGPU_FEO_JPEG_PROGRESSIVE on the device: FLGPU_FE_JPEG writing a progressive file of five scans.  Every file equals the model's
(tests/jpeg_prog_model.py, which tests/test_jpeg_progressive_host.py judges by Pillow and by the library's own entropy decoder), with
and without FLGPU_FEO_JPEG_OPTIMIZE, on every entry path, alone or in a mixed batch; the counters tell the route; with
FLGPU_FEO_JPEG_420 the bit is ignored; without it every byte is the oracle encoder's."""
import threading

import numpy as np
import pytest

import jpeg_420_model as m420
import jpeg_opt_model as jm
import jpeg_prog_cases as cases
import jpeg_prog_model as pm
import synth

Q = "w=300&h=200&quality=75"


def _counters(st):
    return tuple(st.debug_get(k) for k in ("jpeg_progressive", "jpeg_optimized", "jpeg_420"))


def _p(fl, q, progressive=True, optimize=False, s420=False, **kw):
    return fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_progressive=progressive, jpeg_optimize=optimize, jpeg_420=s420, **kw)


def _first_difference(a, b):
    return f"{len(a)} vs {len(b)} bytes, first difference at {next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_corpus_file_equals_the_model_and_the_counters_tell_the_route(fl, gpu_state, oracle, name):
    img, q = cases.get(oracle, name)
    h, w, c = img.shape
    want, _ = cases.model(oracle, name)
    n0, o0, s0 = _counters(gpu_state)
    data = gpu_state.process_pixels(img, _p(fl, q))
    assert _counters(gpu_state) == (n0 + 1, o0, s0)
    assert len(data) <= int(fl.plan_output(_p(fl, q), w, h, c).max_out_bytes)
    print(name, len(data), "bytes")
    assert data == want, _first_difference(data, want)
    # with FLGPU_FEO_JPEG_OPTIMIZE as well: the same file, and jpeg_optimized does not move
    both = gpu_state.process_pixels(img, _p(fl, q, optimize=True))
    assert both == want, _first_difference(both, want)
    assert _counters(gpu_state) == (n0 + 2, o0, s0)
    if name in cases.LARGE:
        return
    # without the bit: the oracle encoder's file, and the counter stands
    plain = gpu_state.process_pixels(img, _p(fl, q, progressive=False))
    assert plain == oracle.jpeg_encode(img, q) and _counters(gpu_state) == (n0 + 2, o0, s0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["photo_83x61_c4_q75", "photo_17x17_c2_q50", "row_33_blocks_period_2"])
def test_with_420_the_bit_is_ignored(fl, gpu_state, oracle, name):
    img, q = cases.get(oracle, name)
    n0, o0, s0 = _counters(gpu_state)
    for optimize in (False, True):
        want, info = m420.encode(oracle, img, q, optimize)
        assert gpu_state.process_pixels(img, _p(fl, q, s420=True, optimize=optimize)) == want, (name, optimize)
        assert gpu_state.process_pixels(img, _p(fl, q, progressive=False, s420=True, optimize=optimize)) == want, (name, optimize)
        o0 += 2 * int(info["optimized"])
        s0 += 2
        assert _counters(gpu_state) == (n0, o0, s0)


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state, oracle):
    names = ["photo_300x200_q75", "photo_1x1_c3_q75", "row_33_blocks_period_2", "run_lengths_q50", "photo_9x7_c4_q1", "noise_32x32_q100", "photo_17x17_c2_q50",
             "row_65_blocks_period_17", "flat_8x8_q75", "photo_83x61_c4_q75", "photo_33x17_c1_q75", "band_ends_q50", "fold_cb_256x176_q75", "ends_in_run_q75"]
    images, params, kinds, labels = [], [], [], []
    for k, n in enumerate(names):          # progressive, every other one with _OPTIMIZE as well
        img, q = cases.get(oracle, n)
        images.append(img); params.append(_p(fl, q, optimize=bool(k & 1))); kinds.append("prog"); labels.append(n)
    # standard, _OPTIMIZE and 4:2:0 pictures (two of them the same pictures as progressive neighbours, one 4:2:0 picture with the bit),
    # a PNG and a lossy WebP picture that carry the bit
    photo = synth.photo(61, 83, 4, index=5)
    big, row = cases.get(oracle, "photo_300x200_q75")[0], cases.get(oracle, "row_33_blocks_period_2")[0]
    images += [big, row, photo, big, photo, photo, photo, photo]
    params += [_p(fl, 75, False), _p(fl, 75, False, optimize=True), _p(fl, 30, False), _p(fl, 100, False, optimize=True), _p(fl, 75, False, s420=True),
               _p(fl, 50, True, s420=True), fl.make_params(quality=75, front_end=fl.FE_PNG, jpeg_progressive=True),
               fl.make_params(quality=75, front_end=fl.FE_WEBP_LOSSY, jpeg_progressive=True)]
    kinds += ["jpeg", "opt", "jpeg", "opt", "420", "420", "png", "webp"]
    labels += [None] * 8
    order = np.random.default_rng(31).permutation(len(images))
    images, params, kinds, labels = ([x[i] for i in order] for x in (images, params, kinds, labels))
    alone = [gpu_state.process_pixels(i, p) for i, p in zip(images, params)]
    n0 = _counters(gpu_state)[0]
    outs = gpu_state.process_batch(images, params)
    assert _counters(gpu_state)[0] - n0 == len(names)
    for k, (got, want) in enumerate(zip(outs, alone)):
        assert isinstance(got, bytes) and got == want, (k, kinds[k], labels[k])
        if kinds[k] == "prog":
            assert got == cases.model(oracle, labels[k])[0], labels[k]
        elif kinds[k] == "jpeg":
            assert got == oracle.jpeg_encode(images[k], params[k].quality), k
        elif kinds[k] == "opt":
            assert got == jm.encode(oracle, images[k], params[k].quality)[0], k
        elif kinds[k] == "420":
            assert got == m420.encode(oracle, images[k], params[k].quality)[0], k
        else:
            assert got == gpu_state.process_pixels(images[k], fl.make_params(quality=75, front_end=params[k].front_end)), kinds[k]


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state, oracle):
    import torch
    name = "photo_83x61_c4_q75"
    img, q = cases.get(oracle, name)
    alone, plain = cases.model(oracle, name)[0], oracle.jpeg_encode(img, q)
    p, pb = _p(fl, q), _p(fl, q, optimize=True)
    # 16 concurrent callers through the queue, alternating the bit
    got, errors = [None] * 16, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(img, _p(fl, q, progressive=(i % 2 == 0)))
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
    assert gpu_state.process_batch([img] * 4, [p, pb, p, pb]) == [alone] * 4
    # flgpu_transform_batch_device + flgpu_batch_results
    h, w, c = img.shape
    src = [torch.from_numpy(img).cuda() for _ in range(2)]
    cap = int(fl.plan_output(p, w, h, c).max_out_bytes)
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    before = _counters(gpu_state)[0]
    gpu_state.process_batch_device([t.data_ptr() for t in src], [(h, w, c)] * 2, p, [t.data_ptr() for t in dst], [cap] * 2,
                                   stream=torch.cuda.current_stream().cuda_stream)
    for i, (flags, nbytes) in enumerate(gpu_state.batch_results()):
        assert flags & fl.IMG_ENCODED and dst[i][:nbytes].cpu().numpy().tobytes() == alone
    assert _counters(gpu_state)[0] - before == 2
    # a second context in the process, and a context of two shards (both on device 0)
    with fl.State(device=0) as other:
        assert other.process_pixels(img, p) == alone and other.process_pixels(img, pb) == alone and other.debug_get("jpeg_progressive") == 2
    with fl.State(devices=[0, 0]) as two:
        assert two.process_batch([img] * 4, [p, pb, pb, p]) == [alone] * 4
        assert two.process_pixels(img, p) == alone and two.debug_get("jpeg_progressive") == 5


@pytest.mark.gpu
def test_the_query_level_route_and_the_flagship_request(fl, gpu_state, oracle):
    big = synth.photo(1080, 1920, 3, index=3)
    new = fl.ENCODE_JPEG_PROGRESSIVE
    pixels = gpu_state.process_pixels(big, fl.make_params(300, 200))
    want, old = pm.encode(oracle, pixels, 75)[0], oracle.jpeg_encode(pixels, 75)
    assert gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_JPEG, jpeg_progressive=True)) == want
    before = _counters(gpu_state)
    mime, kind, body = gpu_state.process_image(big, Q, fl.Format(new), input_format=fl.IN_JPEG)
    assert (mime, kind) == ("image/jpeg", fl.RESULT_JPEG_STREAM) and body == want
    assert gpu_state.process_image(big, Q, fl.Format(new | fl.ENCODE_JPEG_OPTIMIZE), input_format=fl.IN_JPEG)[2] == want
    assert gpu_state.process_image(big, Q, fl.Format(new | fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY), input_format=fl.IN_JPEG)[2] == want, "webp accepted, not asked for"
    assert _counters(gpu_state) == (before[0] + 3, before[1], before[2])
    # with the 4:2:0 bit: the 4:2:0 file; without the bit: today's file; with it on every other arm: what the arm gives without it
    assert gpu_state.process_image(big, Q, fl.Format(new | fl.ENCODE_JPEG_420), input_format=fl.IN_JPEG)[2] == m420.encode(oracle, pixels, 75)[0]
    assert gpu_state.process_image(big, Q, fl.Format(0), input_format=fl.IN_JPEG)[2] == old
    for query, content, fmt in ((Q, fl.ENCODE_PNG, fl.IN_PNG), (Q + "&webp=true", fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY, fl.IN_JPEG), (Q, 0, fl.IN_OTHER)):
        a = gpu_state.process_image(big, query, fl.Format(content), input_format=fmt)
        b = gpu_state.process_image(big, query, fl.Format(content | new), input_format=fmt)
        assert a[:2] == b[:2] and (a[2] == b[2] if isinstance(a[2], bytes) else np.array_equal(a[2], b[2])), (query, fmt)
    assert _counters(gpu_state)[0] == before[0] + 3
    # a JPEG file through flgpu_process_jpeg with the accept bit: decoded, resized and coded on the device
    data = oracle.jpeg_encode(synth.photo(120, 200, 3, index=9), 85)
    small = gpu_state.process_pixels(gpu_state.decode_jpeg(data), fl.make_params(64, 48))
    mime, kind, body = gpu_state.process_jpeg(data, "w=64&h=48&quality=50", fl.Format(new))
    assert (mime, kind) == ("image/jpeg", fl.RESULT_JPEG_STREAM) and body == pm.encode(oracle, small, 50)[0]
    assert gpu_state.process_jpeg(data, "w=64&h=48&quality=50")[2] == oracle.jpeg_encode(small, 50)
    a = gpu_state.process_jpeg(data, "w=64&h=48&webp=true&quality=50", fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY))
    assert a == gpu_state.process_jpeg(data, "w=64&h=48&webp=true&quality=50", fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | new))
    assert _counters(gpu_state)[0] == before[0] + 4


@pytest.mark.gpu
def test_a_progressive_file_from_the_device_decodes_on_the_device_to_the_oracles_pixels(fl, gpu_state, oracle):
    for name in ("photo_83x61_c4_q75", "photo_17x17_c2_q50", "photo_300x200_q75", "run_lengths_q50"):
        img, q = cases.get(oracle, name)
        data = gpu_state.process_pixels(img, _p(fl, q))
        assert data == cases.model(oracle, name)[0]
        assert np.array_equal(gpu_state.decode_jpeg(data), oracle.jpeg_decode(oracle.jpeg_encode(img, q))), name


@pytest.mark.gpu
def test_a_destination_one_byte_short(fl, gpu_state, oracle):
    for name in ("photo_83x61_c4_q75", "noise_32x32_q100"):
        img, q = cases.get(oracle, name)
        full = cases.model(oracle, name)[0]
        with pytest.raises(fl.FanlinError) as e:
            gpu_state.process_pixels(img, _p(fl, q), capacity=-(len(full) - 1))
        assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
        assert gpu_state.process_pixels(img, _p(fl, q), capacity=-len(full)) == full
