"""The lens contract of include/line3d_amd.h ("A LENS") in numpy (float64 / int64): what k_det_undistort_lens (l3d_detect.hip) must give byte for byte.

For output pixel (column j, row i), with the OUTPUT camera (fx', fy', cx', cy') and the lens's SOURCE camera (fx, fy, cx, cy; none: the output's):
    x = (j - cx') / fx'      y = (i - cy') / fy'      r2 = x x + y y
    BROWN:    num = 1 + ((k3 r2 + k2) r2 + k1) r2      den = 1 + ((k6 r2 + k5) r2 + k4) r2      kr = num / den
              xd = x kr + ((2 p1) x y + p2 (r2 + 2 (x x)))
              yd = y kr + (p1 (r2 + 2 (y y)) + (2 p2) x y)
    FISHEYE:  r = sqrt(r2)   th = atan(r)   t2 = th th
              td = th (1 + (((k4 t2 + k3) t2 + k2) t2 + k1) t2)
              s = r > 1e-8 ? td / r : 1      xd = x s      yd = y s
    u = fx xd + cx           v = fy yd + cy
then the inside test, the rounding to 1/32 pixel and the four taps of tests/undistort_model.py.  BROWN coefficients come in OpenCV's order
k1 k2 p1 p2 k3 k4 k5 k6, FISHEYE as k1 k2 k3 k4.  A BROWN lens with all coefficients within 1e-12 and equal cameras passes the pixels through."""
import numpy as np

import undistort_model as um

BROWN, FISHEYE = 1, 2
EPS = um.EPS


def source_coordinates(width, height, out_cam, model, src_cam, coeffs):
    """-> (u, v), float64 arrays height x width; out_cam, src_cam: (fx, fy, cx, cy), src_cam None: out_cam; coeffs: up to 8 numbers"""
    ofx, ofy, ocx, ocy = (float(c) for c in out_cam)
    fx, fy, cx, cy = (float(c) for c in (out_cam if src_cam is None else src_cam))
    k = [float(c) for c in coeffs] + [0.0] * (8 - len(coeffs))
    j = np.arange(width, dtype=np.float64)[None, :]
    i = np.arange(height, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = (j - ocx) / ofx + 0.0 * i
        y = (i - ocy) / ofy + 0.0 * j
        r2 = x * x + y * y
        if model == BROWN:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
            den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
            kr = num / den
            xd = x * kr + ((2.0 * p1) * x * y + p2 * (r2 + 2.0 * (x * x)))
            yd = y * kr + (p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * x * y)
        elif model == FISHEYE:
            r = np.sqrt(r2)
            th = np.arctan(r)
            t2 = th * th
            td = th * (1.0 + (((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2)
            s = np.where(r > 1e-8, td / np.where(r > 1e-8, r, 1.0), 1.0)
            xd = x * s
            yd = y * s
        else:
            raise ValueError("model")
        u = fx * xd + cx
        v = fy * yd + cy
    return u, v


def denominator(width, height, out_cam, coeffs):
    """den of a BROWN lens per output pixel"""
    ofx, ofy, ocx, ocy = (float(c) for c in out_cam)
    k = [float(c) for c in coeffs] + [0.0] * (8 - len(coeffs))
    j = np.arange(width, dtype=np.float64)[None, :]
    i = np.arange(height, dtype=np.float64)[:, None]
    x = (j - ocx) / ofx + 0.0 * i
    y = (i - ocy) / ofy + 0.0 * j
    r2 = x * x + y * y
    return 1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2


def is_active(out_cam, model, src_cam, coeffs):
    same = src_cam is None or tuple(float(c) for c in src_cam) == tuple(float(c) for c in out_cam)
    return model == FISHEYE or not same or any(abs(float(c)) > EPS for c in coeffs)


def resample(img, u, v, inside):
    """the four taps of the contract at (u, v) where inside, 0 elsewhere -> (image, partial, x0_negative)"""
    h, w = img.shape[:2]
    x0, a, y0, b = um.quantise(u, v, inside)
    p = np.zeros((h + 2, w + 2) + img.shape[2:], np.int64)         # zero border: index + 1
    p[1:h + 1, 1:w + 1] = img
    ex = (lambda m: m[..., None]) if img.ndim == 3 else (lambda m: m)
    acc = np.zeros(img.shape, np.int64)
    off = np.zeros((h, w), bool)
    for dy, dx, wt in ((0, 0, (32 - a) * (32 - b)), (0, 1, a * (32 - b)), (1, 0, (32 - a) * b), (1, 1, a * b)):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        acc += ex(wt) * p[np.clip(yy, -1, h) + 1, np.clip(xx, -1, w) + 1]
        off |= ~ok & (wt > 0)
    out = np.where(ex(inside), (acc + 512) >> 10, 0).astype(np.uint8)
    return out, inside & off, inside & (x0 < 0)


def undistort(img, out_cam, model, src_cam, coeffs):
    """-> dict as undistort_model.undistort gives: image; u, v; masks inside, partial, x0_negative; per pixel tie_margin = min(|frac(32u) - 1/2|,
    |frac(32v) - 1/2|) (in units of 1/32 pixel) and limit_distance = the smallest distance of u, v from the four limits -1, width, -1, height
    (both NaN where u or v is)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    h, w = img.shape[:2]
    u, v = source_coordinates(w, h, out_cam, model, src_cam, coeffs)
    with np.errstate(all="ignore"):
        inside = (u > -1.0) & (u < w) & (v > -1.0) & (v < h)
        tie = np.minimum(np.abs((32.0 * u - np.floor(32.0 * u)) - 0.5), np.abs((32.0 * v - np.floor(32.0 * v)) - 0.5))
        limit = np.minimum(np.minimum(np.abs(u + 1.0), np.abs(u - w)), np.minimum(np.abs(v + 1.0), np.abs(v - h)))
    if not is_active(out_cam, model, src_cam, coeffs):
        full = np.ones((h, w), bool)
        return dict(image=img.copy(), u=u, v=v, inside=full, partial=~full, x0_negative=~full, tie_margin=tie, limit_distance=limit)
    out, partial, x0neg = resample(img, u, v, inside)
    return dict(image=out, u=u, v=v, inside=inside, partial=partial, x0_negative=x0neg, tie_margin=tie, limit_distance=limit)


# ---- the cases of tests/test_gpu_lens.py (kernel against model), checked for what they claim and for their margins by tests/test_lens_cases_cpu.py.
# The sizes of undistort_model.CASES: (width, height, channels, row padding in bytes, focal length of the base camera)
SIZES = [
    (8, 8, 1, 0, 6.0),
    (37, 29, 3, 37, 24.0),           # padded rows
    (96, 80, 3, 0, 64.0),
    (96, 80, 1, 0, 64.0),
    (161, 41, 1, 0, 110.0),          # more than one block per row
    (257, 8, 1, 0, 170.0),
]
# (name, model, coefficients, claim): the claim is what tests/test_lens_cases_cpu.py holds the case to
LENSES = [
    ("tangential", BROWN, (0.0, 0.0, 0.06, -0.04), "moves"),
    ("k3", BROWN, (0.0, 0.0, 0.0, 0.0, 0.35), "moves"),
    ("rational", BROWN, (0.3, 0.0, 0.0, 0.0, 0.0, 0.12, 0.05, 0.02), "den_not_one"),
    ("all_eight", BROWN, (-0.28, 0.09, 0.011, -0.007, 0.04, 0.06, -0.03, 0.015), "den_not_one"),
    # den = 1 - 4 r2 is exactly 0 at r2 = 1/4: _cases gives this lens an output camera under which a pixel has x = 1/2, y = 0 exactly, so that kr is
    # inf there and the pixel's coordinates are inf and NaN (0 inf) -- they must come out 0
    ("den_crosses_zero", BROWN, (0.1, 0.0, 0.0, 0.0, 0.0, -4.0, 0.0, 0.0), "den_changes_sign"),
    ("fisheye4", FISHEYE, (-0.04, 0.012, -0.005, 0.0015), "moves"),
    ("fisheye0", FISHEYE, (0.0, 0.0, 0.0, 0.0), "moves"),
]


def _cameras(w, h, f, other):
    """the base camera of a size (the output camera; principal point off the centre by fractions that are no multiple of 1/64), and with `other` the
    source camera that goes with it: the output camera is then zoomed out (fx' = 0.6 fx) and shifted"""
    src = (f, f * 1.03125, 0.5 * w + 0.3, 0.5 * h - 0.2)
    if not other:
        return src, None
    out = (0.6 * src[0], 0.64 * src[1], 0.5 * w - 0.45, 0.5 * h + 0.35)
    return out, src


def _cases():
    cases = []
    for w, h, ch, pad, f in SIZES:
        for name, model, coeffs, claim in LENSES:
            for other in (False, True):
                out_cam, src_cam = _cameras(w, h, f, other)
                if name == "den_crosses_zero":      # a power of two as focal length and an integer principal point: x = 1/2 exactly at column cx' + f2 / 2
                    f2 = 2.0 ** np.floor(np.log2(f))
                    out_cam, src_cam = (f2, f2, float(w // 2), float(h // 2)), (_cameras(w, h, f, False)[0] if other else None)
                cases.append(dict(name="%dx%dx%d_%s%s" % (w, h, ch, name, "_newcam" if other else ""), size=(w, h, ch, pad), out_cam=out_cam, model=model,
                                  src_cam=src_cam, coeffs=coeffs, claim=claim, other=other))
    # all coefficients zero, equal cameras: the input bytes
    cases.append(dict(name="37x29x3_brown_zero", size=(37, 29, 3, 0), out_cam=(30.0, 30.0, 18.5, 14.5), model=BROWN, src_cam=None, coeffs=(0.0,) * 8,
                      claim="identity", other=False))
    return cases


CASES = _cases()


def case_image(case, seed=5):
    """as undistort_model.case_image: (array the call gets -- a view into padded rows where the case asks for them --, the same pixels contiguous)"""
    return um.case_image(case["size"], seed)


def case_model(case):
    _, img = case_image(case)
    return undistort(img, case["out_cam"], case["model"], case["src_cam"], case["coeffs"])
