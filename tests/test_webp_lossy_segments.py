"""FLGPU_FEO_SEGMENTS on the device: the lossy WebP front ends sort a picture's macroblocks into classes by activity and code each class
at its own quantiser index.  Every file equals the model's (tests/vp8_seg_model.py) on the planes the same request returns with
FLGPU_FE_WEBP420 -- which libwebp decodes to exactly the model's reconstruction (tests/test_webp_lossy_segments_host.py) --, on every
entry path, alone or in a mixed batch; the counter tells whether the frame went out segmented; without the option every byte is as
before."""
import threading

import numpy as np
import pytest

import png_write
import synth
import vp8_alpha_model as am
import vp8_ap_cases
import vp8_lf_cases
import vp8_lib
import vp8_seg_cases as cases_mod
import vp8l_model

FAMILIES = cases_mod.FAMILIES
NAMES = [name for name, _, _ in cases_mod.corpus()]
Q = "w=300&h=200&webp=true&quality=75"


def _planes(fl, st, img, **kw):
    return st.process_pixels(img, fl.make_params(front_end=fl.FE_WEBP420, **kw))


def _model(fl, st, img, key, family, segments=True, **kw):
    """(the model's file, its stats, the planes): the planes are what the same request returns with FE_WEBP420."""
    pl = _planes(fl, st, img, **kw)
    i4, adapt, filt = FAMILIES[family]
    data, rec, shown, stats = cases_mod.model("dev:" + key, pl.y, pl.u, pl.v, kw["quality"], pl.a if pl.has_alpha else None, i4, adapt, filt, segments)
    return data, stats, pl, shown


def _twin(fl, st, img, key, family, **kw):
    """The existing models' file of the request without the option."""
    pl = _planes(fl, st, img, **kw)
    i4, adapt, filt = FAMILIES[family]
    a = pl.a if pl.has_alpha else None
    if filt:
        return vp8_lf_cases.model("segdev:" + key, pl.y, pl.u, pl.v, kw["quality"], a, i4, adapt, None)[0]
    return vp8_ap_cases.model("segdev:" + key, pl.y, pl.u, pl.v, kw["quality"], a, i4, adapt)[0]


def _count(st):
    return st.debug_get("webp_lossy_segments")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_corpus_file_equals_the_model_and_the_counter_tells_the_branch(fl, gpu_state, family, name):
    fe = getattr(fl, family)
    img, q = cases_mod.get(name)
    want, stats, pl, shown = _model(fl, gpu_state, img, name, family, quality=q)
    twin = _twin(fl, gpu_state, img, name, family, quality=q)
    before = _count(gpu_state)
    data = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe, segments=True))
    moved = _count(gpu_state) - before
    plain = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe))
    assert _count(gpu_state) - before == moved, "without the option the counter stands"
    print(name, family, len(plain), "->", len(data), "segmented" if moved else "not segmented", stats["seg"]["qi"])
    h, w = img.shape[:2]
    assert len(data) <= int(fl.plan_output(fl.make_params(quality=q, front_end=fe, segments=True), w, h, 4).max_out_bytes)
    assert plain == twin, "without the option: the existing model's file"
    assert moved == int(stats["seg"]["on"]) and (data == plain) == (not stats["seg"]["on"])
    assert data == want
    if name.endswith("_a"):
        # both options: the segmented frame behind the compressed ALPH chunk
        both = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe, segments=True, alpha_vp8l=True))
        assert both == am.with_alpha(want, pl.a) and len(both) < len(data) and am.alph_of(both)[0] == 1


@pytest.mark.gpu
def test_the_library_and_libwebp_decode_a_device_file_alike(fl, gpu_state):
    """Round trip through the library's own decode front end: segment map, absolute quantisers and per-segment filter levels."""
    for name, family in (("letterbox_300x200_q30", "FE_WEBP_LOSSY_AP_LF"), ("bands_64x64_q75", "FE_WEBP_LOSSY_I4_AP"), ("gradnoise_192x64_q1", "FE_WEBP_LOSSY_AP_LF"),
                         ("photo_64x48_q30_a", "FE_WEBP_LOSSY")):
        img, q = cases_mod.get(name)
        data = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=getattr(fl, family), segments=True, alpha_vp8l=name.endswith("_a")))
        want, stats, pl, shown = _model(fl, gpu_state, img, name, family, quality=q)
        assert stats["seg"]["on"] and (family != "FE_WEBP_LOSSY_AP_LF" or stats["chosen"] > 0), name
        theirs_yuv, theirs = vp8_lib.decode_yuv(data), vp8_lib.decode_rgba(data)
        got = gpu_state.debug_vp8_planes(data, filtered=True)
        pixels = gpu_state.decode_webp_lossy(data)
        assert all(np.array_equal(g, r) for g, r in zip(theirs_yuv, shown)) and all(np.array_equal(g, r) for g, r in zip(got, shown)), name
        assert np.array_equal(pixels, theirs[..., :pixels.shape[2]]), name


@pytest.mark.gpu
def test_a_mixed_batch_gives_what_each_request_gives_alone(fl, gpu_state):
    corpus = {name: (img, q) for name, img, q in cases_mod.corpus()}
    # (name, front end, segments, compressed alpha): segmented, degenerate and plain jobs of several families and sizes as neighbours
    jobs = [("letterbox_300x200_q75", "FE_WEBP_LOSSY", True, False), ("letterbox_300x200_q75", "FE_WEBP_LOSSY", False, False),
            ("bands_64x64_q30", "FE_WEBP_LOSSY_I4_AP", True, False), ("flat_64x48_q75", "FE_WEBP_LOSSY_AP_LF", True, False),
            ("gradnoise_192x64_q1", "FE_WEBP_LOSSY_AP_LF", True, False), ("photo_1x1_q30", "FE_WEBP_LOSSY_I4", True, False),
            ("photo_304x272_q75", "FE_WEBP_LOSSY_LF", True, False), ("photo_16x144_q30", "FE_WEBP_LOSSY_I4_AP_LF", True, False),
            ("photo_64x48_q30_a", "FE_WEBP_LOSSY_AP", True, True), ("photo_64x48_q30_a", "FE_WEBP_LOSSY_I4_LF", False, True),
            ("photo_33x15_q1", "FE_WEBP_LOSSY", True, False), ("skew_256x32_q99", "FE_WEBP_LOSSY_I4_AP", True, False),
            ("photo_17x17_q75", "FE_WEBP_LOSSY_AP_LF", False, False)]
    images = [corpus[n][0] for n, _, _, _ in jobs]
    params = [fl.make_params(quality=corpus[n][1], front_end=getattr(fl, f), segments=s, alpha_vp8l=a) for n, f, s, a in jobs]
    photo = corpus["letterbox_300x200_q75"][0]
    # a JPEG and a lossless WebP file beside them; both ignore the option
    images += [photo, corpus["bands_64x64_q30"][0]]
    params += [fl.make_params(quality=75, front_end=fl.FE_JPEG, segments=True), fl.make_params(quality=100, front_end=fl.FE_WEBP_LOSSLESS, segments=True)]
    order = np.random.default_rng(19).permutation(len(images))
    images, params = [images[i] for i in order], [params[i] for i in order]
    names = [(jobs[i] if i < len(jobs) else None) for i in order]
    alone = [gpu_state.process_pixels(i, p) for i, p in zip(images, params)]
    before = _count(gpu_state)
    outs = gpu_state.process_batch(images, params)
    moved = _count(gpu_state) - before
    segmented = 0
    for k, (got, want) in enumerate(zip(outs, alone)):
        assert isinstance(got, bytes) and got == want, (k, names[k])
    for k, j in enumerate(names):
        if j is None:
            if params[k].front_end == fl.FE_WEBP_LOSSLESS:
                assert outs[k] == vp8l_model.encode(images[k]), k
            else:
                assert outs[k] == gpu_state.process_pixels(images[k], fl.make_params(quality=75, front_end=fl.FE_JPEG)), k
            continue
        name, family, seg, alpha = j
        if family in FAMILIES:
            want, stats, pl, _ = _model(fl, gpu_state, images[k], name, family, segments=seg, quality=corpus[name][1])
            segmented += bool(seg and stats["seg"]["on"])
            assert outs[k] == (am.with_alpha(want, pl.a) if alpha else want), j
        else:
            plain = gpu_state.process_pixels(images[k], fl.make_params(quality=corpus[name][1], front_end=getattr(fl, family), alpha_vp8l=alpha))
            on = seg and name not in cases_mod.DEGENERATE
            segmented += on
            assert (outs[k] != plain) == on and vp8_lib.decode_yuv(outs[k]) is not None, j
    assert moved == segmented and segmented >= 8


@pytest.mark.gpu
def test_every_path_gives_identical_bytes(fl, gpu_state):
    import torch
    name = "letterbox_300x200_q75"
    img, q = cases_mod.get(name)
    kinds = [(getattr(fl, f), o) for f in FAMILIES for o in (True, False)] + [(fl.FE_JPEG, True), (fl.FE_WEBP_LOSSLESS, True)]
    want = {k: gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=k[0], segments=k[1])) for k in kinds}
    for f in FAMILIES:
        with_option = _model(fl, gpu_state, img, name, f, quality=q)[0]
        assert want[(getattr(fl, f), True)] == with_option and want[(getattr(fl, f), False)] == _twin(fl, gpu_state, img, name, f, quality=q), f
        assert with_option != want[(getattr(fl, f), False)]
    # 16 concurrent callers through the queue
    got, errors = [None] * 16, []

    def run(i):
        try:
            fe, o = kinds[i % len(kinds)]
            got[i] = gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=fe, segments=o))
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
    p = fl.make_params(quality=q, front_end=fl.FE_WEBP_LOSSY, segments=True)
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
        assert two.process_pixels(img, p) == alone and two.debug_get("webp_lossy_segments") == 5


@pytest.mark.gpu
def test_the_query_level_route_and_the_flagship_request(fl, gpu_state):
    big = synth.photo(1080, 1920, 3, index=3)
    lossy, new = fl.ENCODE_WEBP_LOSSY, fl.ENCODE_WEBP_LOSSY_SEGMENTS
    # the flagship request (1080p -> w=300&h=200&webp=true&quality=75) equals the model
    want = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY, segments=True))
    model, stats, pl, _ = _model(fl, gpu_state, big, "big", "FE_WEBP_LOSSY", w=300, h=200, quality=75)
    old = gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY))
    assert want == model and stats["seg"]["on"] and want != old and old == _twin(fl, gpu_state, big, "big", "FE_WEBP_LOSSY", w=300, h=200, quality=75)
    before = _count(gpu_state)
    for q, fmt, content in ((Q, fl.IN_PNG, fl.Format(fl.ACCEPT_WEBP | lossy | new)), (Q, fl.IN_JPEG, fl.Format(fl.ACCEPT_WEBP | lossy | new)),
                            ("w=300&h=200&quality=75", fl.IN_WEBP, fl.Format(lossy | new))):
        mime, kind, body = gpu_state.process_image(big, q, content, input_format=fmt)
        assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM) and body == want, q
    assert _count(gpu_state) - before == 3
    # without the new bit: the twin's file; the bit alone, or without ENCODE_WEBP_LOSSY: the planes
    assert gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | lossy), input_format=fl.IN_PNG)[2] == old
    for bits in (new, new | fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS | fl.ENCODE_WEBP_LOSSY_FILTER):
        mime, kind, planes = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | bits), input_format=fl.IN_PNG)
        assert kind == fl.RESULT_WEBP_PLANES and all(np.array_equal(getattr(planes, f), getattr(pl, f)) for f in "yuva")
    # the other selecting bits keep their meaning beside the new one
    every = lossy | fl.ENCODE_WEBP_LOSSY_I4 | fl.ENCODE_WEBP_LOSSY_PROBS | fl.ENCODE_WEBP_LOSSY_FILTER | fl.ENCODE_WEBP_LOSSY_ALPHA | new
    mime, kind, body = gpu_state.process_image(big, Q, fl.Format(fl.ACCEPT_WEBP | every), input_format=fl.IN_PNG)
    assert kind == fl.RESULT_WEBP_STREAM
    assert body == gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY_I4_AP_LF, segments=True, alpha_vp8l=True))
    assert body != gpu_state.process_pixels(big, fl.make_params(300, 200, quality=75, front_end=fl.FE_WEBP_LOSSY_I4_AP_LF))
    # a PNG file through flgpu_process_png with the accept bit
    img, q = cases_mod.get("bands_64x64_q75")
    png = png_write.write_png(img, 6, filters=[y % 5 for y in range(64)])
    mime, kind, body = gpu_state.process_png(png, "webp=true&quality=75", fl.Format(fl.ACCEPT_WEBP | lossy | new))
    assert (mime, kind) == ("image/webp", fl.RESULT_WEBP_STREAM)
    assert body == _model(fl, gpu_state, img, "bands_64x64_q75", "FE_WEBP_LOSSY", quality=75)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_destination_one_byte_short(fl, gpu_state, family):
    img, q = cases_mod.get("bands_64x64_q30")
    p = fl.make_params(quality=q, front_end=getattr(fl, family), segments=True)
    full = gpu_state.process_pixels(img, p)
    assert full != gpu_state.process_pixels(img, fl.make_params(quality=q, front_end=getattr(fl, family)))
    with pytest.raises(fl.FanlinError) as e:
        gpu_state.process_pixels(img, p, capacity=-(len(full) - 1))
    assert e.value.status == fl.ERR_BUFFER_TOO_SMALL
    assert gpu_state.process_pixels(img, p, capacity=-len(full)) == full
    # a batch with one too-small stream: no bytes claimed for it and none written, its neighbours delivered intact
    lib = fl.load_library()
    cap, guard = int(fl.plan_output(p, 64, 64, 4).max_out_bytes), 64
    caps = [cap, len(full) - 1, cap]
    offs = [0, cap + guard, cap + guard + len(full) - 1 + guard]
    buf = np.full(offs[2] + cap + guard, 0xA5, np.uint8)
    srcs = (fl.flgpu_image * 3)(*[fl.flgpu_image(img.ctypes.data, img.nbytes, 64, 64, 4, 0) for _ in range(3)])
    dsts = (fl.flgpu_image * 3)(*[fl.flgpu_image(buf.ctypes.data + o, cp, 0, 0, 0, 0) for o, cp in zip(offs, caps)])
    ps = (fl.flgpu_params * 3)(p, p, p)
    assert lib.flgpu_transform_batch(gpu_state._ctx, 3, srcs, ps, dsts) == fl.ERR_BUFFER_TOO_SMALL
    assert dsts[1].bytes == 0 and (buf[offs[1]:offs[1] + caps[1]] == 0xA5).all(), "no partial file"
    for i in range(3):
        assert (buf[offs[i] + caps[i]:offs[i] + caps[i] + guard] == 0xA5).all(), "nothing past the capacity"
    for i in (0, 2):
        assert buf[offs[i]:offs[i] + dsts[i].bytes].tobytes() == full
