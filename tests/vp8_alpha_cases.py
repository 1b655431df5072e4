"""The alpha corpus of FLGPU_FEO_ALPHA_VP8L (tests/test_webp_lossy_alpha_host.py, tests/test_webp_lossy_alpha.py): small alpha planes
where the VP8L coder of an ALPH chunk can go wrong, each over a picture for the lossy coder.  `branch` is what the rule makes of the
plane -- "compressed" (header byte 1 and a stream strictly smaller than the plane), "raw" (the chunk as without the option) or
"opaque" (no ALPH chunk at all); the host test asserts that the model takes it, with the payload bytes given here (measured with
tests/vp8_alpha_model.py on the CPU).

  ramp_WxH            vp8_cases.alpha_ramp on the translucent sizes of vp8_cases.SIZES: 1 x 1 (raw: 1 + 8 bytes of stream against 1 + 1),
                      partial macroblocks, nine macroblock rows; 1 x 17 is raw too (1 + 51 against 1 + 17), the others compressed in
                      54 or 55 bytes
  noise_64x48         uniform noise: the stream is not smaller than the plane -- raw, 3,073 bytes
  under_64x48         2,945 samples of noise, then zeros: the stream is 3,071 bytes, one under the plane's 3,072 -- compressed, 3,072 bytes
  tie_64x48           one more sample of noise: the stream is 3,072 bytes, the payloads tie -- raw (the inequality is strict)
  zero_17x17          translucent, one literal and one run of 288 -- compressed, 52 bytes
  last_33x15          all 255 but the last pixel 254: the translucency flag set by one sample, a run that ends on the pixel before
                      the last and a literal behind it -- compressed, 53 bytes
  mod3_130x70         (x + y) % 3 * 100: three tiles, literals on both sides of the tile edges -- compressed, 2,326 of 9,101 bytes
  runs_4097x2         4,000 columns of 0, then 97 of 9: runs over 4,096, runs carried across a tile edge and a row edge -- compressed, 56 of 8,195 bytes
  disc_300x200        an anti-aliased disc, the use case, 15 tiles -- compressed, 1,353 of 60,001 bytes
  falloff_300x200     a soft radial falloff not in the corpus: tools/webp_lossy_probe.py measures it (13,902 bytes)
  opaque_64x48        every sample 255: no ALPH chunk"""
import numpy as np

import synth
import vp8_cases


def disc(w=300, h=200, r=80.0):
    """An anti-aliased disc: coverage from the distance to the edge, one pixel of ramp."""
    y, x = np.mgrid[0:h, 0:w]
    d = np.sqrt((x - (w - 1) / 2.0) ** 2 + (y - (h - 1) / 2.0) ** 2)
    return np.clip(np.rint((r + 0.5 - d) * 255.0), 0, 255).astype(np.uint8)


def falloff(w=300, h=200):
    y, x = np.mgrid[0:h, 0:w]
    d = np.sqrt(((x - (w - 1) / 2.0) / (w / 2.0)) ** 2 + ((y - (h - 1) / 2.0) / (h / 2.0)) ** 2)
    return np.clip(np.rint(255.0 * (1.0 - d)), 0, 255).astype(np.uint8)


def _last(w, h):
    a = np.full((h, w), 255, np.uint8)
    a[-1, -1] = 254
    return a


def _noise_then_zeros(w, h, k):
    a = np.zeros(w * h, np.uint8)
    a[:k] = np.random.default_rng(7).integers(0, 256, w * h, dtype=np.uint8)[:k]
    return a.reshape(h, w)


def _mod3(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) % 3 * 100).astype(np.uint8)


def _runs(w, h):
    a = np.zeros((h, w), np.uint8)
    a[:, 4000:] = 9
    return a


def planes():
    """[(name, plane (h, w) uint8, branch)]"""
    out = []
    for w, h in vp8_cases.SIZES:
        out.append((f"ramp_{w}x{h}", vp8_cases.alpha_ramp(w, h), "raw" if w * h <= 17 else "compressed"))
    out += [
        ("noise_64x48", np.random.default_rng(5).integers(0, 256, (48, 64), dtype=np.uint8), "raw"),
        ("under_64x48", _noise_then_zeros(64, 48, 2945), "compressed"),
        ("tie_64x48", _noise_then_zeros(64, 48, 2946), "raw"),
        ("zero_17x17", np.zeros((17, 17), np.uint8), "compressed"),
        ("last_33x15", _last(33, 15), "compressed"),
        ("mod3_130x70", _mod3(130, 70), "compressed"),
        ("runs_4097x2", _runs(4097, 2), "compressed"),
        ("disc_300x200", disc(), "compressed"),
        ("opaque_64x48", np.full((48, 64), 255, np.uint8), "opaque"),
    ]
    return out


# payload bytes (header byte included) the model gives, where the docstring above states them
MEASURED = {"ramp_1x1": 2, "ramp_1x17": 18, "noise_64x48": 3073, "under_64x48": 3072, "tie_64x48": 3073, "zero_17x17": 52, "last_33x15": 53, "mod3_130x70": 2326, "runs_4097x2": 56,
            "disc_300x200": 1353}


def corpus():
    """[(name, Rgba8 picture, quality, branch)]: every plane over a photo of its size, the qualities alternating."""
    out = []
    for k, (name, a, branch) in enumerate(planes()):
        h, w = a.shape
        out.append((name, vp8_cases._rgba(synth.photo(h, w, 3, index=90 + k), a), (30, 75)[k % 2], branch))
    return out


def get(name):
    return {n: (img, q, b) for n, img, q, b in corpus()}[name]
