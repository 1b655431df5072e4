"""The lossy WebP encoder's corpus (tests/test_webp_lossy_host.py, tests/test_webp_lossy.py): small Rgba8 pictures where a VP8 coder
can go wrong -- partial macroblocks, one to nine macroblock rows (the partition rule wraps at nine), every intra mode, skipped
macroblocks, the longest token category, translucent pixels -- and a cache of the model's files, so that each is computed once."""
import numpy as np

import synth
import vp8_model

QUALITIES = (1, 30, 75, 99)
# (width, height): 16x144 has nine macroblock rows, so row 8 wraps into partition 0 of 8
SIZES = ((1, 1), (1, 17), (16, 16), (17, 17), (15, 33), (33, 15), (64, 48), (16, 144), (128, 16))


def _rgba(rgb, alpha=None):
    h, w = rgb.shape[:2]
    a = np.full((h, w, 1), 255, np.uint8) if alpha is None else alpha.reshape(h, w, 1).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb[..., :3], a], axis=2))


def letterboxed_photo(w=300, h=200, index=61):
    out = np.empty((h, w, 3), np.uint8)
    out[:] = (32, 32, 32)
    bar = h // 5
    out[bar:h - bar] = synth.photo(h - 2 * bar, w, 3, index=index)
    return _rgba(out)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(w, h, kind):
    y, x = np.mgrid[0:h, 0:w]
    t = {"h": x * 3, "v": y * 4, "d": x * 2 + y * 2}[kind]
    return _rgba(np.stack([t % 256, (255 - t) % 256, (t // 2) % 256], axis=2).astype(np.uint8))


def alpha_ramp(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 7 + y * 3) % 256).astype(np.uint8)


def corpus():
    """[(name, Rgba8 picture, quality)]; names ending in `_a` are translucent."""
    out = [(f"photo_300x200_q{q}", letterboxed_photo(), q) for q in QUALITIES]
    for k, (w, h) in enumerate(SIZES):
        q = QUALITIES[k % 4]
        out.append((f"photo_{w}x{h}_q{q}", _rgba(synth.photo(h, w, 3, index=50 + k)), q))
        q = QUALITIES[(k + 2) % 4]
        out.append((f"photo_{w}x{h}_q{q}_a", _rgba(synth.photo(h, w, 3, index=70 + k), alpha_ramp(w, h)), q))
    out += [
        ("flat_64x48_q75", _rgba(np.full((48, 64, 3), 130, np.uint8)), 75),  # Y = U = V = 128: the DC prediction without neighbours
        ("flat_17x17_q1_a", _rgba(np.full((17, 17, 3), 200, np.uint8), alpha_ramp(17, 17)), 1),
        ("noise_64x48_q99", _rgba(noise(64, 48, 1)), 99),
        ("noise_64x48_q1", _rgba(noise(64, 48, 2)), 1),
        ("noise_33x15_q30_a", _rgba(noise(33, 15, 3), alpha_ramp(33, 15)), 30),
        ("ramp_h_64x48_q75", ramp(64, 48, "h"), 75),
        ("ramp_v_64x48_q75", ramp(64, 48, "v"), 75),
        ("ramp_d_64x48_q30", ramp(64, 48, "d"), 30),
    ]
    return out


_MODEL = {}


def model(key, y, u, v, quality, a=None):
    """vp8_model.encode, once per key."""
    if key not in _MODEL:
        _MODEL[key] = vp8_model.encode(y, u, v, quality, a)
    return _MODEL[key]
