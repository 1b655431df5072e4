"""FLGPU_FEO_ALPHA_VP8L on the device: the lossy WebP front ends write the alpha plane of a translucent picture as a VP8L stream wherever
that is smaller.  Every file equals with_alpha(model file, plane) (tests/vp8_alpha_model.py over the families' own models) on the
planes the same request returns with FLGPU_FE_WEBP420 -- which libwebp decodes to exactly the plane and the twin's Y, U, V
(tests/test_webp_lossy_alpha_host.py) --, on every entry path, alone or in a mixed batch; without the option every byte is as before."""
import threading

import numpy as np
import pytest

import png_write
import vp8_alpha_cases as cases_mod
import vp8_alpha_model as am
import vp8_ap_cases
import vp8_cases
import vp8_lf_cases
import vp8l_model

FAMILIES = ("FE_WEBP_LOSSY", "FE_WEBP_LOSSY_I4_AP", "FE_WEBP_LOSSY_AP_LF")
# front end -> (B_PRED, adaptive probabilities, loop filter)
TRAITS = {"FE_WEBP_LOSSY": (False, False, False), "FE_WEBP_LOSSY_I4": (True, False, False), "FE_WEBP_LOSSY_AP": (False, True, False),
          "FE_WEBP_LOSSY_I4_AP": (True, True, False), "FE_WEBP_LOSSY_LF": (False, False, True), "FE_WEBP_LOSSY_I4_LF": (True, False, True),
          "FE_WEBP_LOSSY_AP_LF": (False, True, True), "FE_WEBP_LOSSY_I4_AP_LF": (True, True, True)}


def _twin_model(fl, st, img, key, family, quality):
    """(the family's model file with the raw plane, the planes): the planes are what the same request returns with FE_WEBP420."""
    pl = st.process_pixels(img, fl.make_params(front_end=fl.FE_WEBP420, quality=quality))
    a = pl.a if pl.has_alpha else None
    i4, adapt, lf = TRAITS[family]
    if lf:
        return vp8_lf_cases.model(f"alpha:{key}", pl.y, pl.u, pl.v, quality, a, i4, adapt, None)[0], pl
    return vp8_ap_cases.model(f"alpha:{key}", pl.y, pl.u, pl.v, quality, a, i4, adapt)[0], pl


def _want(fl, st, img, key, family, quality):
    twin, pl = _twin_model(fl, st, img, key, family, quality)
    return (am.with_alpha(twin, pl.a) if pl.has_alpha else twin), twin


def _count(st):
    return st.debug_get("webp_alpha_vp8l")


NAMES = [name for name, _, _ in cases_mod.planes()]
assert {b for _, _, b in cases_mod.planes()} == {"compressed", "raw", "opaque"}  # (every branch of the rule is in the corpus)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_corpus_file_equals_the_model_and_the_counter_tells_the_branch(fl, gpu_state, family, name):
    fe = getattr(fl, family)
    img, q, branch = cases_mod.get(name)
    want, twin = _want(fl, gpu_state, img, name, family, q)
    before = _count(gpu_state)
    data = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe, alpha_vp8l=True))
    moved = _count(gpu_state) - before
    plain = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe))
    assert _count(gpu_state) - before == moved, "without the option the counter stands"
    payload = am.alph_of(data) if data[12:16] == b"VP8X" else None
    got = "opaque" if payload is None else "compressed" if payload[0] == 1 else "raw"
    print(name, family, len(plain), "->", len(data), got)
    assert plain == twin, "without the option: the existing model's file"
    assert got == branch and moved == (branch == "compressed") and len(data) <= len(plain)
    assert data == want


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state):
    corpus = {name: (img, q, branch) for name, img, q, branch in cases_mod.corpus()}
    # (name, family, option): translucent and opaque pictures, with and without the option, neighbours of different size and branch
    jobs = [("disc_300x200", "FE_WEBP_LOSSY", True), ("disc_300x200", "FE_WEBP_LOSSY", False), ("noise_64x48", "FE_WEBP_LOSSY_I4_AP", True),
            ("opaque_64x48", "FE_WEBP_LOSSY", True), ("mod3_130x70", "FE_WEBP_LOSSY_AP_LF", True), ("zero_17x17", "FE_WEBP_LOSSY_I4_AP", True),
            ("runs_4097x2", "FE_WEBP_LOSSY_AP_LF", False), ("runs_4097x2", "FE_WEBP_LOSSY_I4", True), ("ramp_1x1", "FE_WEBP_LOSSY_LF", True),
            ("last_33x15", "FE_WEBP_LOSSY_AP", True), ("opaque_64x48", "FE_WEBP_LOSSY_I4_AP", False), ("ramp_16x144", "FE_WEBP_LOSSY_I4_AP_LF", True),
            ("mod3_130x70", "FE_WEBP_LOSSY_I4_LF", True)]
    images = [corpus[n][0] for n, _, _ in jobs]
    params = [fl.make_params(quality=corpus[n][1], front_end=getattr(fl, f), alpha_vp8l=o) for n, f, o in jobs]
    disc = corpus["disc_300x200"][0]
    # a lossless WebP file and a JPEG beside them; both ignore the option
    images += [disc, disc, corpus["mod3_130x70"][0]]
    params += [fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS), fl.make_params(quality=75, front_end=fl.FE_JPEG, alpha_vp8l=True),
               fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS, alpha_vp8l=True)]
    order = np.random.default_rng(17).permutation(len(images))
    images, params = [images[i] for i in order], [params[i] for i in order]
    names = [(jobs[i] if i < len(jobs) else None) for i in order]
    alone = [gpu_state.process_pixels(i, p) for i, p in zip(images, params)]
    before = _count(gpu_state)
    outs = gpu_state.process_batch(images, params)
    compressed = sum(1 for j in names if j and j[2] and corpus[j[0]][2] == "compressed")
    assert _count(gpu_state) - before == compressed
    for k, (got, want) in enumerate(zip(outs, alone)):
        assert isinstance(got, bytes) and got == want, (k, names[k])
    for k, j in enumerate(names):
        if j is None:
            if params[k].front_end == fl.FE_WEBP_LOSSLESS:
                assert outs[k] == vp8l_model.encode(images[k]), k
                assert outs[k] == gpu_state.process_pixels(images[k], fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS)), k
            else:
                assert outs[k] == gpu_state.process_pixels(images[k], fl.make_params(quality=75, front_end=fl.FE_JPEG)), k
            continue
        name, family, option = j
        want, twin = _want(fl, gpu_state, images[k], name, family, corpus[name][1])
        assert outs[k] == (want if option else twin), j


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state):
    import torch
    img, q, _ = cases_mod.get("disc_300x200")
    kinds = [(getattr(fl, f), o) for f in FAMILIES for o in (True, False)] + [(fl.FE_JPEG, True), (fl.FE_WEBP_LOSSLESS, True)]
    want = {k: gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=k[0], alpha_vp8l=k[1])) for k in kinds}
    for f in FAMILIES:
        with_option, twin = _want(fl, gpu_state, img, "disc_300x200", f, q)
        assert want[(getattr(fl, f), True)] == with_option and want[(getattr(fl, f), False)] == twin and len(with_option) < len(twin), f
    # 16 concurrent callers through the queue
    got, errors = [None] * 16, []

    def run(i):
        try:
            fe, o = kinds[i % len(kinds)]
            got[i] = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe, alpha_vp8l=o))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(16):
        assert got[i] == want[kinds[i % len(kinds)]], i
    # flgpu_transform_batch
    p = fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY, alpha_vp8l=True)
    alone = want[(fl.FE_WEBP_LOSSY, True)]
    assert all(o == alone for o in gpu_state.process_batch([img] * 3, [p] * 3))
    # flgpu_transform_batch_device + flgpu_batch_results
    src = [torch.from_numpy(img).cuda() for _ in range(2)]
    cap = int(fl.plan_output(p, 300, 200, 4).max_out_bytes)
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    before = _count(gpu_state)
    gpu_state.process_batch_device([t.data_ptr() for t in src], [(200, 300, 4)] * 2, p, [t.data_ptr() for t in dst], [cap] * 2,
                                   stream=torch.cuda.current_stream().cuda_stream)
    for i, (flags, nbytes) in enumerate(gpu_state.batch_results()):
        assert flags & fl.IMG_ENCODED and dst[i][:nbytes].cpu().numpy().tobytes() == alone
    assert _count(gpu_state) - before == 2
    # a context of two shards (both on device 0)
    with fl.State(devices=[0, 0]) as two:
        assert all(o == alone for o in two.process_batch([img] * 4, [p] * 4))
        assert two.process_pixels(img, p) == alone and two.debug_get("webp_alpha_vp8l") == 5


@pytest.mark.gpu
def test_a_translucent_png_through_the_query_level_route(fl, gpu_state):
    img, _, _ = cases_mod.get("disc_300x200")
    png = png_write.write_png(img, 6, filters=[y % 5 for y in range(200)])
    query = "webp=true&quality=75"
    lossy = fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY
    mime, kind, old = gpu_state.process_png(png, query, fl.Format(lossy))
    before = _count(gpu_state)
    mime, kind, body = gpu_state.process_png(png, query, fl.Format(lossy | fl.ENCODE_WEBP_LOSSY_ALPHA))
    assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and _count(gpu_state) - before == 1
    pl = gpu_state.process_png_pixels(png, fl.make_params(quality=75, front_end=fl.FE_WEBP420))
    assert pl.has_alpha and np.array_equal(pl.a, img[..., 3])
    twin = vp8_cases.model("alpha:png:disc", pl.y, pl.u, pl.v, 75, pl.a)[0]
    assert old == twin and body == am.with_alpha(twin, pl.a) and len(body) < len(old)
    assert am.alph_of(body)[0] == 1 and am.alph_of(old)[0] == 0
    # the library's own decoder reads the compressed chunk back to exactly the plane, and the same colours as from the raw-alpha file
    pixels, pixels_old = gpu_state.decode_webp_lossy(body), gpu_state.decode_webp_lossy(old)
    assert pixels.shape == (200, 300, 4) and np.array_equal(pixels[..., 3], img[..., 3]) and np.array_equal(pixels, pixels_old)
    # the other selecting bits keep their meaning beside the new one, fall-backs included; the bit alone gives the planes
    every = lossy | fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS | fl.ENCODE_WEBP_LOSSY_FILTER | fl.ENCODE_WEBP_LOSSY_ALPHA
    mime, kind, body = gpu_state.process_png(png, query, fl.Format(every))
    assert kind == fl.RESULT_WEBP_STREAM
    assert body == gpu_state.process_png_pixels(png, fl.make_params(quality=75, front_end=fl.FE_WEBP_LOSSY_I4_AP_LF, alpha_vp8l=True))
    assert am.alph_of(body) == am.alph_of(am.with_alpha(twin, pl.a))
    mime, kind, planes = gpu_state.process_png(png, query, fl.Format(fl.ACCEPT_WEBP | fl.ENCODE_WEBP_LOSSY_ALPHA | fl.ENCODE_WEBP_LOSSY_I4))
    assert kind == fl.RESULT_WEBP_PLANES and all(np.array_equal(getattr(planes, f), getattr(pl, f)) for f in "yuva")
    # a decoded picture through flgpu_process_image, and a WebP source that stays WebP
    mime, kind, got = gpu_state.process_image(img, query, fl.Format(lossy | fl.ENCODE_WEBP_LOSSY_ALPHA), input_format=fl.IN_PNG)
    assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and got == am.with_alpha(twin, pl.a)
    sized = gpu_state.process_pixels(img, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY, alpha_vp8l=True))
    mime, kind, got = gpu_state.process_image(img, "w=300&h=200&quality=75", fl.Format(fl.ENCODE_WEBP_LOSSY | fl.ENCODE_WEBP_LOSSY_ALPHA), input_format=fl.IN_WEBP)
    assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and got == sized and am.alph_of(got)[0] == 1
    assert len(got) < len(gpu_state.process_image(img, "w=300&h=200&quality=75", fl.Format(fl.ENCODE_WEBP_LOSSY), input_format=fl.IN_WEBP)[2])


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_a_destination_one_byte_short(fl, gpu_state, family):
    img, q, branch = cases_mod.get("mod3_130x70")
    assert branch == "compressed"
    p = fl.make_params(quality=q, front_end=getattr(fl, family), alpha_vp8l=True)
    full = gpu_state.process_pixels(img, p)
    assert am.alph_of(full)[0] == 1 and len(full) < len(gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=getattr(fl, family))))
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # a batch with one too-small stream: no bytes claimed for it and none written, its neighbours delivered intact
    lib = fl.load_library()
    cap, guard = int(fl.plan_output(p, 130, 70, 4).max_out_bytes), 64
    caps = [cap, len(full) - 1, cap]
    offs = [0, cap + guard, cap + guard + len(full) - 1 + guard]
    buf = np.full(offs[2] + cap + guard, 0xA5, np.uint8)
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(img.ctypes.data, img.nbytes, 130, 70, 4, 0) for _ in range(3)])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(buf.ctypes.data + o, cp, 0, 0, 0, 0) for o, cp in zip(offs, caps)])
    ps = (fl.flgpu_params * 3)(p, p, p)
    assert lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts) == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0 and (buf[offs[1]:offs[1] + caps[1]] == 0xA5).all(), "no partial file"
    for i in range(3):
        assert (buf[offs[i] + caps[i]:offs[i] + caps[i] + guard] == 0xA5).all(), "nothing past the capacity"
    for i in (0, 2):
        assert buf[offs[i]:offs[i] + dsts[i].bytes].tobytes() == full
