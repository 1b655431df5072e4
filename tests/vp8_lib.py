"""ctypes access to the system's libwebp DECODER -- the judge of the lossy WebP encoder's files (tests/vp8_model.py, fl_vp8.hip).
Test infrastructure only.

  decode_yuv(data)    WebPDecodeYUV: the decoder's own Y, U, V planes, no colour conversion, no upsampling -- what a VP8 encoder's
                      reconstruction must equal byte for byte
  decode_rgba(data)   WebPDecodeRGBA (the alpha plane of a translucent file comes back in channel 3)
  features(data)      WebPGetFeatures: (width, height, has_alpha)"""
import ctypes as C
import ctypes.util

import numpy as np


class WebPBitstreamFeatures(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("has_alpha", C.c_int), ("has_animation", C.c_int), ("format", C.c_int),
                ("pad", C.c_uint32 * 5)]


_lib = None


def load():
    global _lib
    if _lib is None:
        try:
            lib = C.CDLL(ctypes.util.find_library("webp") or "libwebp.so.7")
        except OSError:
            return None
        lib.WebPDecodeYUV.restype = C.POINTER(C.c_uint8)
        lib.WebPDecodeYUV.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_uint8)),
                                      C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.WebPDecodeRGBA.restype = C.POINTER(C.c_uint8)
        lib.WebPDecodeRGBA.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.WebPGetFeaturesInternal.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(WebPBitstreamFeatures), C.c_int]
        lib.WebPFree.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def _plane(ptr, stride, w, h):
    a = np.ctypeslib.as_array(ptr, shape=(h * stride,))[: (h - 1) * stride + w]
    return np.array([a[r * stride: r * stride + w] for r in range(h)], dtype=np.uint8).reshape(h, w)


def decode_yuv(data):
    """-> (y, u, v) or None if libwebp rejects the file."""
    assert load() is not None
    w, h, ys, uvs = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    u, v = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
    y = _lib.WebPDecodeYUV(data, len(data), C.byref(w), C.byref(h), C.byref(u), C.byref(v), C.byref(ys), C.byref(uvs))
    if not y:
        return None
    cw, ch = (w.value + 1) // 2, (h.value + 1) // 2
    out = (_plane(y, ys.value, w.value, h.value), _plane(u, uvs.value, cw, ch), _plane(v, uvs.value, cw, ch))
    _lib.WebPFree(y)  # one allocation holds the three planes
    return out


def decode_rgba(data):
    assert load() is not None
    w, h = C.c_int(), C.c_int()
    p = _lib.WebPDecodeRGBA(data, len(data), C.byref(w), C.byref(h))
    if not p:
        return None
    out = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
    _lib.WebPFree(p)
    return out


def features(data):
    assert load() is not None
    f = WebPBitstreamFeatures()
    for abi in (0x0209, 0x0208):
        if _lib.WebPGetFeaturesInternal(data, len(data), C.byref(f), abi) == 0:
            return f.width, f.height, bool(f.has_alpha)
    return None
