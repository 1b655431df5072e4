"""The corpus of the lossy WebP encoder's loop-filtered variants (tests/test_webp_lossy_filter_host.py,
tests/test_webp_lossy_filter.py) and a cache of the model's analyses, evaluations and files, so that each is computed once.

One list serves the four families (B_PRED allowed or not, adaptive probabilities or not): the filter sees a family only through the
reconstruction and the macroblocks' inner-edge flags.  Pictures are small; the shapes are the ones the filter can get wrong:
1 x 1 (one macroblock, inner edges only), 17 x 17 (2 x 2 macroblocks, the first real macroblock edges), 16 x 144 (one column, no
left edges), 128 x 16 (one row, no top edges), 33 x 15 and 15 x 33 (padding excluded from D), 64 x 48 (diagonals of two) and, twice
only, 300 x 200 (a longest diagonal of ten macroblocks: more than one round of a 256-thread workgroup at 32 lanes a macroblock).
Content: photo, noise, ramps, flat, a faint gradient, edges0_48x48_q1 (skipped I16 macroblocks, whose inner edges stay; at quality
1 the B_PRED penalty is so large that this encoder codes none of its macroblocks B_PRED, whichever family), a grey diagonal wave
(with B_PRED allowed it has skipped B_PRED macroblocks, whose inner edges are filtered all the same: the sub-block predictors
follow the diagonal so well that nothing is left to code) and a patchwork with alpha (the VP8X container).  Qualities 1, 30, 50, 75, 99; forced base
levels 1 ({0, 1, 1, 2}), 2, 10, 15 ({0, 8, 15, 23}: across the first hev threshold), 27 ({.., 41}: across the second), 40, 42
({.., 63}: the clamp), 63.

The cases were picked by running the generators below through the model on the CPU; what they reach is asserted by
tests/test_webp_lossy_filter_host.py: each candidate position chosen at least twice, level 0 chosen with L0 > 0, exact ties between
distinct levels resolved downwards, and cases whose runner-up is within 1 % of the winner.

A macroblock coded with Y2 levels alone whose sixteen DCs all come out 0 cannot be constructed with this encoder: the dequantised
Y2 block has steps of at least 8 (y2_dc = 2 x y1_dc >= 8, y2_ac >= 8), the inverse WHT's outputs before the shift are t = H in
with H H^T = 16 I, and sixteen zero DCs need every t + 3 in 0..7, so |in| = |H^T t| / 16 <= 4 < 8 for every coefficient: in = 0.
The model still computes the flag (`y2_only`) and the host test asserts that no corpus picture has one."""
import numpy as np

import synth
import vp8_i4_cases
import vp8_lf_model as lf
from vp8_cases import _rgba, alpha_ramp, letterboxed_photo, noise, ramp

VARIANTS = ((False, False), (True, False), (False, True), (True, True))  # (B_PRED allowed, adaptive probabilities): the four families
FORCED = (1, 2, 10, 15, 27, 40, 42, 63)


def faint(w, h, amp):
    """A low-contrast horizontal gradient on grey."""
    y, x = np.mgrid[0:h, 0:w]
    g = (128 + (x * amp) // max(w, h)).astype(np.uint8)
    return _rgba(np.stack([g, g, g], axis=2))


def wave(w, h, period, amp):
    """A grey sine wave along the falling diagonal."""
    y, x = np.mgrid[0:h, 0:w]
    g = np.round(128 + amp * np.sin((x - y) * 2 * np.pi / period)).astype(np.uint8)
    return _rgba(np.stack([g, g, g], axis=2))


def _photo(w, h, k):
    return _rgba(synth.photo(h, w, 3, index=50 + k))


def _noise(w, h, k):
    return _rgba(noise(w, h, 10 + k))


def corpus():
    """[(name, Rgba8 picture, quality, forced base level or None)]; names ending in `_a` are translucent."""
    out = [
        ("photo_300x200_q30", letterboxed_photo(), 30, None),
        ("photo_300x200_q50", letterboxed_photo(), 50, None),
        ("photo_1x1_q1", _photo(1, 1, 0), 1, None),
        ("photo_17x17_q1", _photo(17, 17, 1), 1, None),
        ("photo_17x17_q75", _photo(17, 17, 1), 75, None),
        ("noise_17x17_q30", _noise(17, 17, 1), 30, None),
        ("photo_16x144_q1", _photo(16, 144, 2), 1, None),
        ("noise_16x144_q1", _noise(16, 144, 2), 1, None),
        ("photo_128x16_q1", _photo(128, 16, 3), 1, None),
        ("noise_128x16_q50", _noise(128, 16, 3), 50, None),
        ("photo_33x15_q1", _photo(33, 15, 4), 1, None),
        ("noise_33x15_q75", _noise(33, 15, 4), 75, None),
        ("photo_15x33_q75", _photo(15, 33, 5), 75, None),
        ("noise_15x33_q30", _noise(15, 33, 5), 30, None),
        ("photo_64x48_q1", _photo(64, 48, 6), 1, None),
        ("photo_64x48_q99", _photo(64, 48, 6), 99, None),
        ("noise_64x48_q30", _noise(64, 48, 6), 30, None),
        ("ramp_h_64x48_q30", ramp(64, 48, "h"), 30, None),
        ("ramp_d_64x48_q30", ramp(64, 48, "d"), 30, None),
        ("flat_64x48_q75", _rgba(np.full((48, 64, 3), 130, np.uint8)), 75, None),
        ("faint_64x48_q30", faint(64, 48, 3), 30, None),
        ("edges0_48x48_q1", vp8_i4_cases.edges(48, 48, 0), 1, None),
        ("wave32_64x48_q30", wave(64, 48, 32, 20), 30, None),
        ("wave48_64x48_q50", wave(64, 48, 48, 20), 50, None),
        ("patchwork_64x48_q30_a", _rgba(vp8_i4_cases.patchwork(64, 48, 6)[..., :3], alpha_ramp(64, 48)), 30, None),
        ("patchwork_64x48_q30_b15_a", _rgba(vp8_i4_cases.patchwork(64, 48, 6)[..., :3], alpha_ramp(64, 48)), 30, 15),
        ("photo_17x17_q30_b42", _photo(17, 17, 1), 30, 42),
    ]
    out += [(f"photo_64x48_q50_b{b}", _photo(64, 48, 6), 50, b) for b in FORCED]
    return out


def analysis_key(name):
    """Cases that differ only in the forced base level share one analysis."""
    parts = [p for p in name.split("_") if not (p[0] == "b" and p[1:].isdigit())]
    return "_".join(parts)


_AN, _EV, _FILES = {}, {}, {}


def analysis(key, y, u, v, quality, i4):
    k = (key, bool(i4))
    if k not in _AN:
        _AN[k] = lf.analyse(y, u, v, quality, i4)
    return _AN[k]


def model(key, y, u, v, quality, a=None, i4=False, adapt=True, base=None):
    """(file, reconstruction, filtered reconstruction, stats) as lf.encode gives them, once per (key, family, base); `key` names
    the planes (and the quality), so cases that share them share the analysis."""
    k = (key, bool(i4), bool(adapt), base)
    if k not in _FILES:
        an = analysis(key, y, u, v, quality, i4)
        if k[:2] + k[3:] not in _EV:  # (the filter does not see the probabilities)
            _EV[k[:2] + k[3:]] = lf.evaluate(an, y, u, v, base)
        _FILES[k] = lf.encode_analysed(an, y, u, v, a, adapt, base, _EV[k[:2] + k[3:]])
    return _FILES[k]
