"""The conversion rule of images in device memory (include/line3d_amd.h, "Images in DEVICE memory") as a numpy model: ingest (the caller's elements
to the detector's 8 bits) and egress (the way back).  It shares no code with the product; the tests hold the kernels to it byte for byte."""
import numpy as np

U8, U16, F16, F32 = 0, 1, 2, 3
NUMPY_DTYPE = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}


def to_u8(x, scale):
    """U16 / F16 / F32 elements -> uint8: exact conversion to f32, ONE f32 multiplication, rint (ties to even), NaN -> 0, clamp to 0..255"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        y = x.astype(np.float32) * np.float32(scale)
        r = np.rint(y)
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r, 0, 255).astype(np.uint8)


def from_u8(v, dtype, scale):
    """uint8 -> the caller's dtype: U8 as is; F32 (float)v * scale; F16 that f32 rounded to nearest even; U16 clamp(rint(v * scale), 0, 65535)"""
    v = np.asarray(v, np.uint8)
    if dtype == U8:
        return v.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        y = v.astype(np.float32) * np.float32(scale)
        if dtype == F32:
            return y
        if dtype == F16:
            return y.astype(np.float16)
        r = np.rint(y)
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r, 0, 65535).astype(np.uint16)


def _offsets(width, height, channels, stride_y, stride_x, stride_c, chan):
    det = 1 if channels == 1 else 3
    y = np.arange(height, dtype=np.int64)[:, None, None] * stride_y
    x = np.arange(width, dtype=np.int64)[None, :, None] * stride_x
    c = (np.zeros(1, np.int64) if channels == 1 else np.asarray(chan, np.int64) * stride_c)[None, None, :]
    return y + x + c, det


def ingest(buf, base, width, height, channels, stride_y, stride_x, stride_c, chan=(0, 1, 2), scale=1.0):
    """buf: the flat array of elements the image lives in; base: the element index of (0, 0, 0); strides in elements, signed -> uint8 H x W x (1 or 3)"""
    at, _ = _offsets(width, height, channels, stride_y, stride_x, stride_c, chan)
    return to_u8(np.asarray(buf).reshape(-1)[base + at], scale)


def egress(buf, base, pixels, channels, stride_y, stride_x, stride_c, chan=(0, 1, 2), scale=1.0, dtype=U8):
    """writes uint8 pixels H x W x (1 or 3) into the flat array buf (in place) as k_det_egress must; elements the image does not address stay"""
    pixels = np.asarray(pixels, np.uint8)
    if pixels.ndim == 2:
        pixels = pixels[:, :, None]
    h, w, _ = pixels.shape
    at, _ = _offsets(w, h, channels, stride_y, stride_x, stride_c, chan)
    flat = buf.reshape(-1)
    flat[base + at] = from_u8(pixels, dtype, scale)
    return buf


# ---- the corner table: (dtype, raw elements, scale, expected bytes), expectations written by hand from the rule
def _f16_bits(*bits):
    return np.array(bits, np.uint16).view(np.float16)


CORNERS = [
    # k + 0.5 for even and odd k, -0.5, the top of the range, NaN, both infinities, -0
    (F32, np.array([0.5, 1.5, 2.5, 3.5, -0.5, 254.5, 255.5, np.nan, np.inf, -np.inf, -0.0, 255.49999, 1e30, -1e30], np.float32), 1.0,
     [0, 2, 2, 4, 0, 254, 255, 0, 255, 0, 0, 255, 255, 0]),
    # a tensor in [0, 1] at scale 255; 0 x inf is NaN
    (F32, np.array([0.0, 1.0, 0.5, 1.0 / 255.0, 2.0, -1.0], np.float32), 255.0, [0, 255, 128, 1, 255, 0]),
    (F32, np.array([np.inf, -np.inf, 3.0], np.float32), 0.0, [0, 0, 0]),
    (F16, np.array([0.5, 1.5, 2.5, 3.5, -0.5, 254.5, 255.5, np.nan, np.inf, -np.inf], np.float16), 1.0, [0, 2, 2, 4, 0, 254, 255, 0, 255, 0]),
    # f16 subnormals are exact in f32: bits 1, 3, 0x3ff are 1, 3, 1023 x 2^-24
    (F16, _f16_bits(0x0001, 0x0003, 0x03ff, 0x8001), float(2 ** 24), [1, 3, 255, 0]),
    (F16, _f16_bits(0x0001, 0x0003, 0x0005), float(2 ** 23), [0, 2, 2]),
    # a 16-bit image at 1 / 257
    (U16, np.array([0, 128, 129, 65535, 257, 32896], np.uint16), 1.0 / 257.0, [0, 0, 1, 255, 1, 128]),
    (U16, np.array([0, 1, 2, 3, 255, 256, 65535], np.uint16), 0.5, [0, 0, 1, 2, 128, 128, 255]),
    (U8, np.array([0, 1, 127, 128, 255], np.uint8), float("nan"), [0, 1, 127, 128, 255]),         # scale is ignored
]
