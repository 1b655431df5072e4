"""What FLGPU_FE_WEBP_LOSSY_I4 buys over FLGPU_FE_WEBP_LOSSY, on the models (tests/vp8_i4_model.py against tests/vp8_model.py) and
the inputs of the table in DESIGN.md section 4: the letterboxed synth.photo 300 x 200 at quality 1 / 30 / 75 / 99.  (The flagship
request's planes come from the device's resampler; no host test builds them, so that column is measured by
tools/webp_lossy_probe.py on the GPU.)  No GPU."""
import math

import numpy as np
import pytest

import vp8_cases
import vp8_i4_cases
import vp8_lib
import webp_lib
from test_webp_lossy_host import PSNR_DEFICIT_BAR_DB, SIZE_RATIO_BAR

# Measured: I4 bytes / I16-only bytes 1.000 / 0.900 / 0.746 / 0.731 (q = 1 / 30 / 75 / 99; at q = 1 the penalty leaves every
# macroblock of this picture I16 and the files are the same), Y-PSNR of the I4 reconstruction minus the I16-only one
# +0.00 / +0.37 / +0.06 / +0.00 dB; against libwebp's file at the same q 1.035 / 1.335 / 1.210 / 1.505 (was 1.035 / 1.483 / 1.622 /
# 2.059).  The files are deterministic: the bar on the Y-PSNR deficit is the worst measured one (I16-only minus I4: 0.00 dB,
# none) rounded up to the next 0.05 dB.
MEASURED_SIZE_VS_I16 = (1.000, 0.900, 0.746, 0.731)
MEASURED_SIZE_VS_LIBWEBP = (1.035, 1.335, 1.210, 1.505)
MEASURED_PSNR_GAIN_DB = (0.00, 0.37, 0.06, 0.00)
PSNR_DEFICIT_VS_I16_BAR_DB = 0.05


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)


@pytest.fixture(scope="module")
def table(oracle):
    """[(q, planes y u v, I4 (file, reconstruction, stats), I16-only (file, reconstruction, stats))]"""
    y, u, v, has_alpha = oracle.webp_yuv420(vp8_cases.letterboxed_photo())
    assert not has_alpha
    return [(q, (y, u, v), vp8_i4_cases.model(f"photo_300x200_q{q}", y, u, v, q), vp8_i4_cases.model_i16(f"photo_300x200_q{q}", y, u, v, q))
            for q in vp8_cases.QUALITIES]


def test_the_i4_file_is_never_larger_and_smaller_from_quality_30_up(table):
    for k, (q, (y, u, v), (d4, r4, s4), (d16, r16, s16)) in enumerate(table):
        gain = _psnr(r4[0], y) - _psnr(r16[0], y)
        hist = np.bincount(s4["bmodes"][s4["bmodes"] >= 0], minlength=10).tolist()
        print(f"q={q}: I4 {len(d4)} bytes against I16-only {len(d16)} ({len(d4) / len(d16):.3f}); Y-PSNR {_psnr(r4[0], y):.2f} dB against "
              f"{_psnr(r16[0], y):.2f} dB ({gain:+.3f}); {int(s4['i4'].sum())} of {s4['i4'].size} macroblocks B_PRED, modes {hist}")
        assert len(d4) <= len(d16), q
        if q >= 30:
            assert len(d4) < len(d16), q
        assert -gain <= PSNR_DEFICIT_VS_I16_BAR_DB, q
        assert abs(len(d4) / len(d16) - MEASURED_SIZE_VS_I16[k]) < 0.001 and abs(gain - MEASURED_PSNR_GAIN_DB[k]) < 0.01, "the record above is stale"


def test_the_bars_held_against_libwebp_hold_for_the_i4_files(table):
    assert webp_lib.load() is not None and vp8_lib.load() is not None
    for k, (q, (y, u, v), (d4, r4, s4), _) in enumerate(table):
        ref = webp_lib.encode_planes(y, u, v, q)
        ref_y = vp8_lib.decode_yuv(ref)[0]
        ratio, deficit = len(d4) / len(ref), _psnr(ref_y, y) - _psnr(r4[0], y)
        print(f"q={q}: {len(d4)} bytes against libwebp's {len(ref)} (ratio {ratio:.3f}); Y-PSNR deficit {deficit:+.2f} dB")
        assert ratio <= SIZE_RATIO_BAR and deficit <= PSNR_DEFICIT_BAR_DB, q
        assert abs(ratio - MEASURED_SIZE_VS_LIBWEBP[k]) < 0.001, "the record above is stale"
