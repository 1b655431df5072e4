"""ctypes access to the system's libwebp for the lossy WebP DECODER's tests (beside tests/webp_lib.py, which it builds on): the
encoder with the settings that steer segmentation, the loop filter and the ALPH chunk, and the decoder as the arbiter --
WebPDecodeYUV for the planes behind the loop filter, WebPDecodeRGB / WebPDecodeRGBA for the pixels.  Test infrastructure only."""
import ctypes as C

import numpy as np

import webp_lib

# WebPConfig: plain ints at these word offsets (lossless 0, quality 1 as a float)
CONFIG_WORDS = dict(method=2, segments=6, filter_strength=8, filter_sharpness=9, filter_type=10, alpha_compression=12, alpha_filtering=13,
                    alpha_quality=14)


def load():
    lib = webp_lib.load()
    if lib is None:
        return None
    lib.WebPDecodeYUV.restype = C.POINTER(C.c_uint8)
    lib.WebPDecodeYUV.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_uint8)),
                                  C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for name in ("WebPDecodeRGB", "WebPDecodeRGBA"):
        fn = getattr(lib, name)
        fn.restype = C.POINTER(C.c_uint8)
        fn.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.WebPFree.argtypes = [C.c_void_p]
    return lib


def encode(rgba, quality, **settings):
    """rgba: [h, w, 4] (an opaque picture gets no ALPH chunk); settings: names of CONFIG_WORDS"""
    assert load() is not None
    lib, abi = webp_lib._lib, webp_lib._abi
    h, w, c = rgba.shape
    assert c == 4
    pic = webp_lib.WebPPicture()
    assert lib.WebPPictureInitInternal(C.byref(pic), abi) == 1
    pic.use_argb, pic.width, pic.height = 1, w, h
    buf = np.ascontiguousarray(rgba)
    assert lib.WebPPictureImportRGBA(C.byref(pic), buf.ctypes.data_as(C.POINTER(C.c_uint8)), w * 4) == 1
    cfg = webp_lib._config(quality)
    words = C.cast(cfg, C.POINTER(C.c_int))
    for k, v in settings.items():
        words[CONFIG_WORDS[k]] = int(v)
    wr = webp_lib.WebPMemoryWriter()
    lib.WebPMemoryWriterInit(C.byref(wr))
    pic.writer = C.cast(lib.WebPMemoryWrite, C.c_void_p)
    pic.custom_ptr = C.cast(C.pointer(wr), C.c_void_p)
    ok = lib.WebPEncode(cfg, C.byref(pic))
    assert ok == 1, f"WebPEncode failed, error {pic.error_code}"
    data = bytes(bytearray(wr.mem[: wr.size]))
    lib.WebPMemoryWriterClear(C.byref(wr))
    lib.WebPPictureFree(C.byref(pic))
    return data


def decode_yuv(data):
    """-> (y, u, v) as libwebp reconstructs them (loop filter applied), or None where it rejects the file"""
    lib = load()
    w, h, s, cs = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    u, v = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
    y = lib.WebPDecodeYUV(data, len(data), C.byref(w), C.byref(h), C.byref(u), C.byref(v), C.byref(s), C.byref(cs))
    if not y:
        return None
    ch, cw = (h.value + 1) // 2, (w.value + 1) // 2
    out = (np.ctypeslib.as_array(y, shape=(h.value, s.value))[:, :w.value].copy(),
           np.ctypeslib.as_array(u, shape=(ch, cs.value))[:, :cw].copy(), np.ctypeslib.as_array(v, shape=(ch, cs.value))[:, :cw].copy())
    lib.WebPFree(y)
    return out


def decode_pixels(data, channels):
    """WebPDecodeRGB (channels == 3) / WebPDecodeRGBA (4) -> [h, w, channels], or None where libwebp rejects the file"""
    lib = load()
    w, h = C.c_int(), C.c_int()
    p = (lib.WebPDecodeRGB if channels == 3 else lib.WebPDecodeRGBA)(data, len(data), C.byref(w), C.byref(h))
    if not p:
        return None
    out = np.ctypeslib.as_array(p, shape=(h.value, w.value, channels)).copy()
    lib.WebPFree(p)
    return out
