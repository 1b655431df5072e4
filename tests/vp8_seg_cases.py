"""The corpus of FLGPU_FEO_SEGMENTS (tests/test_webp_lossy_segments_host.py, tests/test_webp_lossy_segments.py) and a cache of the
model's analyses and files, so that each is computed once.  The shapes are the smallest at which each part can go wrong:

  photo_1x1            one macroblock: degenerate (one bin)
  flat_64x48           every macroblock flat: degenerate
  noise_64x48          uniform noise: every macroblock in bin 255 -- one bin, degenerate
  photo_17x17, photo_33x15   partial macroblocks: edge replication inside the activity
  photo_16x144         nine macroblock rows: eight token partitions with wrap, one column of ids
  gradnoise_192x64     a grey gradient beside uniform noise: exactly two used classes (0 and 3), at every quality (at 99 the offsets
                       of amp = 1 are 0 and the file is the twin's)
  skew_256x32_q99      three quarters gradient, one quarter noise: the mean centre sits low, so at quality 99 (amp = 1) the noise
                       class comes out at index 1 and the gradient's offset clamps at index 0 -- segmented at qi = 0
  bands_64x64          four 16-row bands of grey noise of rising amplitude (8, 23, 38, 53, chosen with the model on the CPU): four
                       used classes with strictly rising indices at quality 30 and 75
  letterbox_300x200    vp8_cases.letterboxed_photo: flat bars kept out of the classification, 13 x 19 macroblocks
  photo_304x272        19 x 17 = 323 macroblocks: more macroblocks than threads in the segment kernel's workgroup
  photo_64x48_q30_a    translucent: with FLGPU_FEO_ALPHA_VP8L too on the device
Quality 1 clamps an upper class at index 127 (gradnoise_192x64_q1); quality 99 is the amp = 1 path."""
import numpy as np

import synth
import vp8_seg_model as sm
from vp8_cases import _rgba, alpha_ramp, letterboxed_photo, noise

# the three families the twin and the device are compared on: name -> (B_PRED, adaptive probabilities, loop filter)
FAMILIES = {"FE_WEBP_LOSSY": (False, False, False), "FE_WEBP_LOSSY_I4_AP": (True, True, False), "FE_WEBP_LOSSY_AP_LF": (False, True, True)}
BAND_AMPLITUDES = (8, 23, 38, 53)


def gradnoise(w, h, split, seed=21):
    """Columns [0, split): a horizontal grey gradient; the rest: uniform grey noise."""
    g = np.zeros((h, w), np.uint8)
    g[:, :split] = (np.arange(split) * 255 // max(1, split - 1))[None, :]
    g[:, split:] = np.random.default_rng(seed).integers(0, 256, (h, w - split), dtype=np.uint8)
    return _rgba(np.stack([g, g, g], axis=2))


def bands(w=64, h=64, seed=22):
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w), np.uint8)
    for k, amp in enumerate(BAND_AMPLITUDES):
        g[16 * k:16 * k + 16] = 128 + rng.integers(-amp, amp + 1, (16, w))
    return _rgba(np.stack([g, g, g], axis=2))


def _photo(w, h, k):
    return _rgba(synth.photo(h, w, 3, index=80 + k))


def corpus():
    """[(name, Rgba8 picture, quality)]; names ending in `_a` are translucent."""
    out = [
        ("photo_1x1_q30", _photo(1, 1, 0), 30),
        ("flat_64x48_q75", _rgba(np.full((48, 64, 3), 130, np.uint8)), 75),
        ("noise_64x48_q30", _rgba(noise(64, 48, 23)), 30),
        ("photo_17x17_q75", _photo(17, 17, 1), 75),
        ("photo_33x15_q1", _photo(33, 15, 2), 1),
        ("photo_16x144_q30", _photo(16, 144, 3), 30),
    ]
    out += [(f"gradnoise_192x64_q{q}", gradnoise(192, 64, 96), q) for q in (1, 30, 75, 99)]
    out += [
        ("skew_256x32_q99", gradnoise(256, 32, 192), 99),
        ("bands_64x64_q30", bands(), 30),
        ("bands_64x64_q75", bands(), 75),
        ("letterbox_300x200_q30", letterboxed_photo(), 30),
        ("letterbox_300x200_q75", letterboxed_photo(), 75),
        ("photo_304x272_q75", _photo(304, 272, 4), 75),
        ("photo_64x48_q30_a", _rgba(synth.photo(48, 64, 3, index=85), alpha_ramp(64, 48)), 30),
    ]
    return out


DEGENERATE = ("photo_1x1_q30", "flat_64x48_q75", "noise_64x48_q30")


def get(name):
    return {n: (img, q) for n, img, q in corpus()}[name]


_AN, _FILES = {}, {}


def analysis(key, y, u, v, quality, i4, segments=True):
    """sm.analyse, once per (key, B_PRED, segments); `key` names the planes and the quality."""
    k = (key, bool(i4), bool(segments))
    if k not in _AN:
        _AN[k] = sm.analyse(y, u, v, quality, i4, segments, adapt=True)
    return _AN[k]


def model(key, y, u, v, quality, a=None, i4=False, adapt=False, filt=False, segments=True):
    """(file, reconstruction, what a decoder shows, stats) as sm.encode gives them, once per (key, family, segments)."""
    k = (key, bool(i4), bool(adapt), bool(filt), bool(segments))
    if k not in _FILES:
        _FILES[k] = sm.encode_analysed(analysis(key, y, u, v, quality, i4, segments), y, u, v, a, adapt, filt)
    return _FILES[k]
