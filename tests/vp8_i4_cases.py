"""The corpus of the lossy WebP encoder's I4 variant (tests/test_webp_lossy_i4_host.py, tests/test_webp_lossy_i4.py): the smallest
Rgba8 pictures at which a coder that mixes I16 and B_PRED macroblocks can go wrong -- a single macroblock with all borders, two per
side with padding and the right edge's above-right rule, an interior macroblock with all eight neighbours, 1 / 2 / 4 / 8
partitions, the flagship output -- with photo, noise, flat and constructed content (edges at several angles, ramps, flat and busy
macroblocks side by side), and a cache of the model's files, so that each is computed once."""
import numpy as np

import synth
import vp8_cases
import vp8_i4_model
from vp8_cases import _rgba, alpha_ramp, letterboxed_photo, noise, ramp

QUALITIES = (1, 30, 75, 99)
SIZES = ((1, 1), (4, 4), (16, 16), (17, 17), (15, 33), (33, 15), (48, 48), (64, 48), (128, 16), (16, 144), (16, 64))  # (the last: four partitions)


def edges(w, h, angle_deg, period=24):
    """Hard dark / bright stripes at an angle: what the directional sub-block predictors are for."""
    y, x = np.mgrid[0:h, 0:w]
    t = np.deg2rad(angle_deg)
    s = np.floor((x * np.cos(t) + y * np.sin(t)) / (period / 2.0)).astype(np.int64) & 1
    g = np.where(s == 1, 220, 30).astype(np.uint8)
    return _rgba(np.stack([g, g, (g // 2 + 40).astype(np.uint8)], axis=2))


def patchwork(w, h, seed):
    """Macroblocks in a checkerboard: flat ones (I16, skipped once their neighbours let the DC prediction be exact) and noisy ones
    (B_PRED) -- every adjacency of the two kinds in one picture."""
    out = np.full((h, w, 3), 128, np.uint8)
    rnd = noise(w, h, seed)
    for mby in range((h + 15) // 16):
        for mbx in range((w + 15) // 16):
            if (mbx + mby) & 1:
                out[mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = rnd[mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16]
    return _rgba(out)


def ramp_with_noise(w, h, kind, seed):
    """A ramp (I16: V, H or TM predicts it) whose second macroblock column is noise (B_PRED)."""
    out = ramp(w, h, kind)[..., :3].copy()
    out[:, 16:32] = noise(w, h, seed)[:, 16:32]
    return _rgba(out)


def corpus():
    """[(name, Rgba8 picture, quality)]; names ending in `_a` are translucent."""
    out = [(f"photo_300x200_q{q}", letterboxed_photo(), q) for q in QUALITIES]
    for k, (w, h) in enumerate(SIZES):
        q = QUALITIES[k % 4]
        out.append((f"photo_{w}x{h}_q{q}", _rgba(synth.photo(h, w, 3, index=50 + k)), q))
        q = QUALITIES[(k + 1) % 4]
        out.append((f"noise_{w}x{h}_q{q}", _rgba(noise(w, h, 10 + k)), q))
    for k, (w, h) in enumerate(((1, 1), (17, 17), (33, 15), (48, 48))):
        q = QUALITIES[(k + 2) % 4]
        out.append((f"photo_{w}x{h}_q{q}_a", _rgba(synth.photo(h, w, 3, index=70 + k), alpha_ramp(w, h)), q))
    for k, angle in enumerate((0, 22, 45, 67, 90, 112, 135, 157)):
        w, h = ((48, 48), (33, 15), (64, 48), (15, 33))[k % 4]
        out.append((f"edges{angle}_{w}x{h}_q{QUALITIES[k % 4]}", edges(w, h, angle), QUALITIES[k % 4]))
    out += [
        ("flat_48x48_q75", _rgba(np.full((48, 48, 3), 130, np.uint8)), 75),
        ("flat_17x17_q1_a", _rgba(np.full((17, 17, 3), 200, np.uint8), alpha_ramp(17, 17)), 1),
        ("patchwork_48x48_q75", patchwork(48, 48, 5), 75),
        ("patchwork_64x48_q30_a", _rgba(patchwork(64, 48, 6)[..., :3], alpha_ramp(64, 48)), 30),
        ("patchwork_128x16_q99", patchwork(128, 16, 7), 99),
        ("patchwork_16x144_q1", patchwork(16, 144, 8), 1),
        ("ramp_h_noise_64x48_q75", ramp_with_noise(64, 48, "h", 20), 75),
        ("ramp_v_noise_64x48_q75", ramp_with_noise(64, 48, "v", 21), 75),
        ("ramp_d_noise_64x48_q30", ramp_with_noise(64, 48, "d", 22), 30),
    ]
    return out


_MODEL = {}


def model(key, y, u, v, quality, a=None):
    """vp8_i4_model.encode, once per key."""
    if key not in _MODEL:
        _MODEL[key] = vp8_i4_model.encode(y, u, v, quality, a)
    return _MODEL[key]


def model_i16(key, y, u, v, quality, a=None):
    """vp8_model.encode (FE_WEBP_LOSSY's file on the same planes), once per key."""
    return vp8_cases.model("i4cases:" + key, y, u, v, quality, a)
