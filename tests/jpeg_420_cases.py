"""The corpus of FLGPU_FEO_JPEG_420, shared by tests/test_jpeg_420_host.py (CPU) and tests/test_jpeg_420.py (GPU): the smallest pictures
at which each part of the option can go wrong.  (name, picture, quality); pictures and model files are built once per process.  The
coding grid runs 8 MCUs per wave and 2 waves per workgroup, the pack kernel 512 units per round over 32 KB windows of the scan."""
import functools

import numpy as np

import synth

QUALITIES = (1, 50, 75, 100)
ROW_MCUS = (7, 8, 9, 15, 16, 17)      # one row of MCUs around the wave (8) and workgroup (16) edges of the coding and statistics grids


def _checker(a, b):
    yy, xx = np.mgrid[0:32, 0:64]
    return np.where((((yy >> 4) + (xx >> 4)) & 1)[:, :, None] == 0, np.array(a, np.uint8), np.array(b, np.uint8)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _corpus():
    out = [("photo_1x1_c3_q75", synth.photo(1, 1, 3, index=1), 75), ("photo_8x8_c1_q50", synth.photo(8, 8, 1, index=2), 50),
           ("photo_9x7_c4_q1", synth.photo(7, 9, 4, index=3), 1), ("photo_16x16_c3_q100", synth.photo(16, 16, 3, index=4), 100),
           ("photo_17x17_c2_q50", synth.photo(17, 17, 2, index=6), 50), ("photo_83x61_c4_q75", synth.photo(61, 83, 4, index=5), 75)]
    for k, n in enumerate(ROW_MCUS):
        q = QUALITIES[k % 4]
        out.append((f"row_{n}_mcus_q{q}", synth.photo(16, 16 * n, 3, index=20 + n), q))
    flat = np.empty((16, 24, 3), np.uint8)
    flat[:] = (90, 140, 200)
    out.append(("flat_24x16_q75", flat, 75))
    quad = np.empty((16, 16, 3), np.uint8)  # four flat Y blocks of different colours: their chroma block is not flat
    quad[:8, :8], quad[:8, 8:], quad[8:, :8], quad[8:, 8:] = (200, 30, 40), (20, 180, 60), (40, 50, 220), (230, 220, 30)
    out.append(("quadrants_16x16_q75", quad, 75))
    out.append(("grey_33x17_c1_q75", synth.photo(17, 33, 1, index=8), 75))  # luma that is not flat over chroma that is
    out.append(("noise_32x32_q100", synth.uniform(32, 32, 3, index=9), 100))
    out.append(("noise_32x32_q50", synth.uniform(32, 32, 3, index=9), 50))
    out.append(("photo_300x200_q75", synth.photo(200, 300, 3, index=7), 75))
    out.append(("photo_300x200_q100", synth.photo(200, 300, 3, index=7), 100))
    out.append(("checker_bw_64x32_q100", _checker((0, 0, 0), (255, 255, 255)), 100))
    out.append(("checker_yb_64x32_q100", _checker((255, 255, 0), (0, 0, 255)), 100))
    return tuple(out)


def corpus():
    return _corpus()


NAMES = (["photo_1x1_c3_q75", "photo_8x8_c1_q50", "photo_9x7_c4_q1", "photo_16x16_c3_q100", "photo_17x17_c2_q50", "photo_83x61_c4_q75"]
         + [f"row_{n}_mcus_q{QUALITIES[k % 4]}" for k, n in enumerate(ROW_MCUS)]
         + ["flat_24x16_q75", "quadrants_16x16_q75", "grey_33x17_c1_q75", "noise_32x32_q100", "noise_32x32_q50", "photo_300x200_q75", "photo_300x200_q100",
            "checker_bw_64x32_q100", "checker_yb_64x32_q100"])


def get(name):
    for n, img, q in corpus():
        if n == name:
            return img, q
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def model(oracle, name, optimize=False, fallback=False):
    """(file, info) of the model for a corpus case, computed once"""
    import jpeg_420_model as m
    img, q = get(name)
    return m.encode(oracle, img, q, optimize, fallback)


def _ac_bits(syms, std):
    """[(table, AC code bits)] per unit of a scan under the standard tables"""
    out = []
    for t, s, _, vbits in syms:
        if t in (0, 2):
            out.append([t + 1, 0])
        else:
            out[-1][1] += (int(std[t][s]) >> 16) + vbits
    return out


def check_conditions(oracle):
    """What the corpus is there to reach, asserted on the model."""
    import jpeg_420_model as m
    import jpeg_opt_model as jm
    assert [n for n, _, _ in corpus()] == NAMES
    std = jm.standard_tables(oracle.jpeg_header(8, 8, 75))

    def syms(name):
        return model(oracle, name)[1]["syms"]

    def has(name, table, symbol):
        return any(t == table and s == symbol for t, s, _, _ in syms(name))
    # a luma and a chroma unit whose AC code exceeds the 96 bits a unit's record holds (the acbits continuation)
    long_units = {t for t, bits in _ac_bits(syms("noise_32x32_q100"), std) if bits > 96}
    assert long_units == {1, 3}, long_units
    assert has("noise_32x32_q50", 3, 0xF0), "a ZRL symbol in the chroma table"
    assert has("photo_300x200_q75", 1, 0xF0), "a ZRL symbol in the luma table"
    assert has("checker_yb_64x32_q100", 0, 11) and has("checker_yb_64x32_q100", 2, 11), "DC size category 11 in luma and in chroma"
    big, info = model(oracle, "photo_300x200_q100")
    assert len(big) - jm.STD_HEADER_BYTES > 32768 and len(info["coef"]) == 1482 > 2 * 512, "more than one pack window, more than two pack rounds"
    # the quadrants: four flat Y blocks, a chroma block that is not
    coef = model(oracle, "quadrants_16x16_q75")[1]["coef"]
    assert not coef[:4, 1:].any() and coef[4, 1:].any() and coef[5, 1:].any()
    coef = model(oracle, "grey_33x17_c1_q75")[1]["coef"].reshape(-1, 6, 64)
    assert coef[:, :4, 1:].any() and not coef[:, 4:, 1:].any() and not coef[:, 4:, 0].any()
    assert len(model(oracle, "photo_17x17_c2_q50")[1]["coef"]) == 4 * 6
    assert m.planes(oracle, get("photo_17x17_c2_q50")[0])[1].shape == (16, 16)
