"""FLGPU_FEO_JPEG_OPTIMIZE on the device: FLGPU_FE_JPEG with Huffman tables built from the picture's own symbol counts.  Every file equals
the model's (tests/jpeg_opt_model.py: the oracle's coefficients, the rule of csrc/fl_jpeg_opt_core.h, the never-larger decision) -- which
Pillow decodes to exactly the standard file's pixels (tests/test_jpeg_optimize_host.py) -- on every entry path, alone or in a mixed
batch; the counter tells whether the picture's tables went out; without the option every byte is the oracle encoder's."""
import threading

import numpy as np
import pytest

import jpeg_opt_cases as cases
import jpeg_opt_model as jm
import synth

Q = "w=300&h=200&quality=75"


def _count(st):
    return st.debug_get("jpeg_optimized")


def _cap(img):
    return img.shape[0] * img.shape[1] * 16 + 4096


def _opt(fl, st, img, q, **kw):
    return st.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_optimize=True, **kw), capacity=_cap(img))


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_corpus_file_equals_the_model_and_the_counter_tells_the_branch(fl, gpu_state, oracle, name):
    img, q = cases.get(oracle, name)
    want, info = cases.model(oracle, name)
    before = _count(gpu_state)
    data = _opt(fl, gpu_state, img, q)
    moved = _count(gpu_state) - before
    plain = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_JPEG), capacity=_cap(img))
    assert _count(gpu_state) - before == moved, "without the option the counter stands"
    print(name, len(plain), "->", len(data), "optimized" if moved else "standard")
    assert plain == oracle.jpeg_encode(img, q), "without the option: the oracle encoder's file"
    assert moved == int(info["optimized"]) and (len(data) < len(plain) if moved else data == plain)
    assert len(data) <= int(fl.plan_output(fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_optimize=True), img.shape[1], img.shape[0], img.shape[2]).max_out_bytes)
    assert data == want, f"{len(data)} vs {len(want)} bytes, first difference at {next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), None)}"


@pytest.mark.gpu
def test_the_fallback_switch_gives_the_plain_file(fl, gpu_state, oracle):
    before = _count(gpu_state)
    with gpu_state.switches(jpeg_optimize_fallback=1):
        for name in ("photo_83x61_c4_q75", "row_33_blocks_q50", "flat_24x16_q75", "fold_256x176_q75", "photo_300x200_q100"):
            img, q = cases.get(oracle, name)
            assert _opt(fl, gpu_state, img, q) == oracle.jpeg_encode(img, q) == cases.model(oracle, name, True)[0], name
    assert _count(gpu_state) == before, "a picture that fell back is not counted"
    img, q = cases.get(oracle, "photo_83x61_c4_q75")
    assert _opt(fl, gpu_state, img, q) == cases.model(oracle, "photo_83x61_c4_q75")[0] and _count(gpu_state) == before + 1


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state, oracle):
    names = ["photo_300x200_q100", "photo_1x1_c3_q75", "row_17_blocks_q75", "fold_256x176_q75", "photo_9x7_c4_q1", "all_ac", "busy_lanes", "photo_8x8_c1_q50",
             "row_32_blocks_q1", "flat_24x16_q75", "photo_83x61_c4_q75"]
    images = [cases.get(oracle, n)[0] for n in names]
    params = [fl.make_params(quality=cases.get(oracle, n)[1], front_end=fl.FE_JPEG, jpeg_optimize=True) for n in names]
    kinds = ["opt"] * len(names)
    # plain JPEG pictures (two of them the same pictures as optimised neighbours), a PNG and a lossy WebP picture: all ignore the bit
    photo = synth.photo(61, 83, 4, index=5)
    images += [cases.get(oracle, "photo_300x200_q100")[0], cases.get(oracle, "row_17_blocks_q75")[0], photo, photo, photo]
    params += [fl.make_params(quality=100, front_end=fl.FE_JPEG), fl.make_params(quality=75, front_end=fl.FE_JPEG),
               fl.make_params(quality=30, front_end=fl.FE_JPEG), fl.make_params(quality=75, front_end=fl.FE_PNG, jpeg_optimize=True),
               fl.make_params(quality=75, front_end=fl.FE_WEBP_LOSSY, jpeg_optimize=True)]
    kinds += ["jpeg", "jpeg", "jpeg", "png", "webp"]
    order = np.random.default_rng(23).permutation(len(images))
    images, params, kinds = [images[i] for i in order], [params[i] for i in order], [kinds[i] for i in order]
    labels = [names[i] if i < len(names) else None for i in order]
    alone = [gpu_state.process_pixels(i, p) for i, p in zip(images, params)]
    before = _count(gpu_state)
    outs = gpu_state.process_batch(images, params)
    moved = _count(gpu_state) - before
    optimized = 0
    for k, (got, want) in enumerate(zip(outs, alone)):
        assert isinstance(got, bytes) and got == want, (k, kinds[k], labels[k])
        if kinds[k] == "opt":
            model, info = cases.model(oracle, labels[k])
            optimized += int(info["optimized"])
            assert got == model, labels[k]
        elif kinds[k] == "jpeg":
            assert got == oracle.jpeg_encode(images[k], params[k].quality), k
        else:
            plain = fl.make_params(quality=75, front_end=params[k].front_end)
            assert got == gpu_state.process_pixels(images[k], plain), kinds[k]
    assert moved == optimized == len(names)


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state, oracle):
    import torch
    name = "photo_83x61_c4_q75"
    img, q = cases.get(oracle, name)
    alone, plain = cases.model(oracle, name)[0], oracle.jpeg_encode(img, q)
    p = fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_optimize=True)
    kinds = [(True, alone), (False, plain)]
    # 16 concurrent callers through the queue
    got, errors = [None] * 16, []

    def run(i):
        try:
            got[i] = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_optimize=kinds[i % 2][0]))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        assert got[i] == kinds[i % 2][1], i
    # flgpu_transform_batch
    assert all(o == alone for o in gpu_state.process_batch([img] * 3, [p] * 3))
    # flgpu_transform_batch_device + flgpu_batch_results
    h, w, c = img.shape
    src = [torch.from_numpy(img).cuda() for _ in range(2)]
    cap = int(fl.plan_output(p, w, h, c).max_out_bytes)
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    before = _count(gpu_state)
    gpu_state.process_batch_device([t.data_ptr() for t in src], [(h, w, c)] * 2, p, [t.data_ptr() for t in dst], [cap] * 2,
                                   stream=torch.cuda.current_stream().cuda_stream)
    for i, (flags, nbytes) in enumerate(gpu_state.batch_results()):
        assert flags & fl.IMG_ENCODED and dst[i][:nbytes].cpu().numpy().tobytes() == alone
    assert _count(gpu_state) - before == 2
    # a second context in the process, and a context of two shards (both on device 0)
    with fl.State(device=0) as other:
        assert other.process_pixels(img, p) == alone and other.debug_get("jpeg_optimized") == 1
    with fl.State(devices=[0, 0]) as two:
        assert all(o == alone for o in two.process_batch([img] * 4, [p] * 4))
        assert two.process_pixels(img, p) == alone and two.debug_get("jpeg_optimized") == 5


@pytest.mark.gpu
def test_the_query_level_route_and_the_flagship_request(fl, gpu_state, oracle):
    big = synth.photo(1080, 1920, 3, index=3)
    new = fl.ENCODE_JPEG_OPTIMIZE
    pixels = gpu_state.process_pixels(big, fl.make_params(300, 200))
    want, info = jm.encode(oracle, pixels, 75)
    old = oracle.jpeg_encode(pixels, 75)
    assert info["optimized"] and len(want) < len(old)
    assert gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_JPEG, jpeg_optimize=True)) == want
    before = _count(gpu_state)
    mime, kind, body = gpu_state.process_image(big, Q, fl.Format(new), input_format=fl.IN_JPEG)
    assert (mime, kind) == ("image/jpeg", fl.RESULT_JPEG_STREAM) and body == want
    assert gpu_state.process_image(big, Q, fl.Format(new | fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY), input_format=fl.IN_JPEG)[2] == want, "webp accepted, not asked for"
    assert _count(gpu_state) - before == 2
    # without the bit: today's file; with it on every other arm: what the arm gives without it
    assert gpu_state.process_image(big, Q, fl.Format(0), input_format=fl.IN_JPEG)[2] == old
    for query, content, fmt in ((Q, fl.ENCODE_PNG, fl.IN_PNG), (Q + "&webp=true", fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY, fl.IN_JPEG), (Q, 0, fl.IN_OTHER)):
        a = gpu_state.process_image(big, query, fl.Format(content), input_format=fmt)
        b = gpu_state.process_image(big, query, fl.Format(content | new), input_format=fmt)
        assert a[:2] == b[:2] and (a[2] == b[2] if isinstance(a[2], bytes) else np.array_equal(a[2], b[2])), (query, fmt)
    assert _count(gpu_state) - before == 2
    # a JPEG file through flgpu_process_jpeg with the accept bit: decoded, resized and coded on the device
    data = oracle.jpeg_encode(synth.photo(120, 200, 3, index=9), 85)
    decoded = gpu_state.decode_jpeg(data)
    mime, kind, body = gpu_state.process_jpeg(data, "w=64&h=48&quality=50", fl.Format(new))
    assert (mime, kind) == ("image/jpeg", fl.RESULT_JPEG_STREAM)
    assert body == jm.encode(oracle, gpu_state.process_pixels(decoded, fl.make_params(64, 48)), 50)[0]
    assert gpu_state.process_jpeg(data, "w=64&h=48&quality=50")[2] == oracle.jpeg_encode(gpu_state.process_pixels(decoded, fl.make_params(64, 48)), 50)
    # a PNG file through flgpu_process_png, a negotiated WebP from the JPEG file: the bit does nothing
    import png_write
    png = png_write.write_png(synth.photo(40, 56, 3, index=11), 2, filters=[y % 5 for y in range(40)])
    for content in (0, fl.ENCODE_PNG):
        a, b = gpu_state.process_png(png, "w=32&h=24", fl.Format(content)), gpu_state.process_png(png, "w=32&h=24", fl.Format(content | new))
        assert a[:2] == b[:2] and (a[2] == b[2] if isinstance(a[2], bytes) else np.array_equal(a[2], b[2]))
    a = gpu_state.process_jpeg(data, "w=64&h=48&webp=true&quality=50", fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY))
    assert a == gpu_state.process_jpeg(data, "w=64&h=48&webp=true&quality=50", fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY | new))
    assert _count(gpu_state) - before == 3


@pytest.mark.gpu
def test_a_destination_one_byte_short(fl, gpu_state, oracle):
    img, q = cases.get(oracle, "photo_83x61_c4_q75")
    h, w, c = img.shape
    p = fl.make_params(quality=q, front_end=fl.FE_JPEG, jpeg_optimize=True)
    full = cases.model(oracle, "photo_83x61_c4_q75")[0]
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # a batch with one too-small stream: no bytes claimed for it, its neighbours delivered intact, nothing past any capacity
    lib = fl.load_library()
    cap, guard = int(fl.plan_output(p, w, h, c).max_out_bytes), 64
    caps = [cap, len(full) - 1, cap]
    offs = [0, cap + guard, cap + guard + len(full) - 1 + guard]
    buf = np.full(offs[2] + cap + guard, 0xA5, np.uint8)
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(img.ctypes.data, img.nbytes, w, h, c, 0) for _ in range(3)])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(buf.ctypes.data + o, cp, 0, 0, 0, 0) for o, cp in zip(offs, caps)])
    ps = (fl.flgpu_params * 3)(p, p, p)
    assert lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts) == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0
    for i in range(3):
        assert (buf[offs[i] + caps[i]:offs[i] + caps[i] + guard] == 0xA5).all(), "nothing past the capacity"
    for i in (0, 2):
        assert buf[offs[i]:offs[i] + dsts[i].bytes].tobytes() == full
