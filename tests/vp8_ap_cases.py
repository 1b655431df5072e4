"""The corpus of the lossy WebP encoder's adaptive-probability variants (tests/test_webp_lossy_probs_host.py,
tests/test_webp_lossy_probs.py): the pictures of vp8_cases.corpus() for FE_WEBP_LOSSY_AP and of vp8_i4_cases.corpus() for
FE_WEBP_LOSSY_I4_AP -- they already hold the smallest shapes at which the coder can go wrong --, and a cache of the model's analyses
and files, so that each is computed once."""
import vp8_ap_model as ap
import vp8_cases
import vp8_i4_cases


def corpus(i4):
    """[(name, Rgba8 picture, quality)] of the variant.  Nothing had to be added: between them the two corpora update nodes of all
    four block types, set nodes to 255 and to 1, hold pictures without any update (flat ones, and edges0_48x48_q1 with coded
    macroblocks), and mix B_PRED and I16 macroblocks so that a Y2 context passes through (the patchworks);
    tests/test_webp_lossy_probs_host.py asserts each of these."""
    return vp8_i4_cases.corpus() if i4 else vp8_cases.corpus()


_AN, _FILES = {}, {}


def analysis(key, y, u, v, quality, i4):
    """ap.analyse, once per (key, variant)."""
    k = (key, bool(i4))
    if k not in _AN:
        _AN[k] = ap.analyse(y, u, v, quality, i4)
    return _AN[k]


def model(key, y, u, v, quality, a=None, i4=False, adapt=True):
    """(file, reconstruction, stats) as ap.encode gives them, once per (key, variant, adapt); the analysis is shared."""
    k = (key, bool(i4), bool(adapt))
    if k not in _FILES:
        _FILES[k] = ap.encode_analysed(analysis(key, y, u, v, quality, i4), a, adapt)
    return _FILES[k]
