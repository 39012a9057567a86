"""The undistortion contract of include/line3d_amd.h in numpy (float64 / int64): what k_det_undistort (l3d_detect.hip) must give byte for byte.

For output pixel (column j, row i):
    x = (j - cx) / fx,  y = (i - cy) / fy,  r2 = x x + y y,  kr = 1 + (k2 r2 + k1) r2,  u = fx (x kr) + cx,  v = fy (y kr) + cy
u outside (-1, width) or v outside (-1, height) (NaN included): 0.  Otherwise iu = rint(32 u), iv = rint(32 v) (ties to even),
x0 = floor(iu / 32), a = iu - 32 x0, likewise y0, b, and per channel
    out = ((32-a)(32-b) p(y0,x0) + a (32-b) p(y0,x0+1) + (32-a) b p(y0+1,x0) + a b p(y0+1,x0+1) + 512) >> 10
with a tap outside the image counting as 0."""
import numpy as np

EPS = 1e-12         # the drivers' L3D_EPS: both |k1| and |k2| at or below it -> the pixels pass through


def source_coordinates(width, height, fx, fy, cx, cy, k1, k2):
    """-> (u, v), float64 arrays height x width"""
    j = np.arange(width, dtype=np.float64)[None, :]
    i = np.arange(height, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = (j - cx) / fx + 0.0 * i
        y = (i - cy) / fy + 0.0 * j
        r2 = x * x + y * y
        kr = 1.0 + (k2 * r2 + k1) * r2
        u = fx * (x * kr) + cx
        v = fy * (y * kr) + cy
    return u, v


def quantise(u, v, inside):
    """-> x0, a, y0, b (int64; zero where not inside)"""
    with np.errstate(all="ignore"):
        iu = np.where(inside, np.rint(32.0 * np.where(inside, u, 0.0)), 0.0).astype(np.int64)
        iv = np.where(inside, np.rint(32.0 * np.where(inside, v, 0.0)), 0.0).astype(np.int64)
    x0, y0 = iu // 32, iv // 32             # floor division: a, b in 0..31 for negative iu, iv as well
    return x0, iu - 32 * x0, y0, iv - 32 * y0


def undistort(img, fx, fy, cx, cy, k1, k2):
    """-> dict: image (as img); u, v; masks inside, partial (inside with a tap of non-zero weight off the image), x0_negative (inside, x0 < 0);
    per pixel tie_margin = min(|frac(32u) - 1/2|, |frac(32v) - 1/2|) and limit_distance = the smallest distance of u, v from the four
    limits -1, width, -1, height (both NaN where u or v is)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    h, w = img.shape[:2]
    u, v = source_coordinates(w, h, fx, fy, cx, cy, k1, k2)
    with np.errstate(all="ignore"):
        inside = (u > -1.0) & (u < w) & (v > -1.0) & (v < h)
        tie = np.minimum(np.abs((32.0 * u - np.floor(32.0 * u)) - 0.5), np.abs((32.0 * v - np.floor(32.0 * v)) - 0.5))
        limit = np.minimum(np.minimum(np.abs(u + 1.0), np.abs(u - w)), np.minimum(np.abs(v + 1.0), np.abs(v - h)))
    if abs(k1) <= EPS and abs(k2) <= EPS:
        out = img.copy()
        full = np.ones((h, w), bool)
        return dict(image=out, u=u, v=v, inside=full, partial=~full, x0_negative=~full, tie_margin=tie, limit_distance=limit)
    x0, a, y0, b = quantise(u, v, inside)
    p = np.zeros((h + 2, w + 2) + img.shape[2:], np.int64)         # zero border: index + 1
    p[1:h + 1, 1:w + 1] = img

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        t = p[np.clip(yy, -1, h) + 1, np.clip(xx, -1, w) + 1]
        return t, ok

    ex = (lambda m: m[..., None]) if img.ndim == 3 else (lambda m: m)
    acc = np.zeros(img.shape, np.int64)
    off = np.zeros((h, w), bool)
    for dy, dx, wt in ((0, 0, (32 - a) * (32 - b)), (0, 1, a * (32 - b)), (1, 0, (32 - a) * b), (1, 1, a * b)):
        t, ok = tap(y0 + dy, x0 + dx)
        acc += ex(wt) * t
        off |= ~ok & (wt > 0)
    out = np.where(ex(inside), (acc + 512) >> 10, 0).astype(np.uint8)
    return dict(image=out, u=u, v=v, inside=inside, partial=inside & off, x0_negative=inside & (x0 < 0), tie_margin=tie, limit_distance=limit)


# ---- the cases of tests/test_gpu_undistort.py (kernel against model), checked for their margins by tests/test_undistort_cpu.py:
# (width, height, channels, row padding in bytes, fx, fy, cx, cy, k1, k2)
CASES = [
    (8, 8, 1, 0, 6.0, 6.0, 4.0, 4.0, 0.35, 0.0),                     # taps left of column 0, partial and full outside
    (37, 29, 3, 37, 30.0, 30.0, 18.5, 14.5, -0.4, 0.15),             # pincushion, all inside; padded rows
    (37, 29, 1, 0, 28.0, 31.0, 16.25, 15.75, 0.5, 0.2),              # fx != fy, off-centre
    (96, 80, 3, 0, 70.0, 70.0, 48.0, 40.0, 0.12, 0.0),
    (96, 80, 1, 0, 70.0, 70.0, 48.0, 40.0, -0.3, 0.0),
    (161, 41, 1, 0, 120.0, 120.0, 80.5, 20.5, -0.25, 0.05),          # more than one block per row
    (257, 8, 1, 0, 200.0, 200.0, 128.5, 4.0, 0.3, -0.1),
    (37, 29, 3, 0, 30.0, 30.0, 18.5, 14.5, 0.0, 0.0),                # must return the input bytes
]


def case_image(case, seed=5):
    """the noise image of a case: (array the call gets -- a view into padded rows where the case asks for them --, the same pixels contiguous)"""
    w, h, ch, pad = case[:4]
    rng = np.random.default_rng(seed)
    shape = (h, w) if ch == 1 else (h, w, ch)
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if not pad:
        return img, img
    buf = np.full((h, w * ch + pad), 77, np.uint8)
    buf[:, :w * ch] = img.reshape(h, w * ch)
    view = np.lib.stride_tricks.as_strided(buf, shape=shape, strides=(w * ch + pad,) + ((1,) if ch == 1 else (ch, 1)))
    return view, img
