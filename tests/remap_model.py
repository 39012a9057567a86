"""The remap contract of include/line3d_amd.h ("A REMAP") in numpy (float64 / int64), sharing no code with the product:
  * plan()           the planner (l3d_undistort_plan): border points, Newton inversion, the two rectangles, the output camera and size;
  * remap()          the resampling onto another size with its validity plane (k_det_undistort_remap) -- the map is tests/lens_model.py's;
  * defined_plane()  the validity plane carried to the detector's working resolution N x M: a gradient pixel is undefined if any pixel that
                     contributed to its value is invalid (the 2 x 2 taps of the rescale where it rescales, the 7 + 7 taps of the Gaussian sampler
                     with its symmetric boundary, the 2 x 2 stencil of the gradient, clipped at the last row and column)."""
import numpy as np

import lens_model as lm

BROWN, FISHEYE = lm.BROWN, lm.FISHEYE
ITERATIONS, CONVERGED, SIZE_SLACK, RAY_STEPS = 50, 1e-12, 1e-6, 16
MAX_SIDE, MAX_BYTES = 1 << 24, 1 << 31


# ---------------------------------------------------------------------------------------------------------------- the planner
def _forward_brown(k, x, y):
    """BROWN's forward formulas and their Jacobian at (x, y): f, g, fx, fy, gx, gy"""
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    r2 = x * x + y * y
    num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
    dnum = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1
    dden = (3.0 * k6 * r2 + 2.0 * k5) * r2 + k4
    kr = num / den
    dkr = (dnum * den - num * dden) / (den * den)
    f = x * kr + ((2.0 * p1) * x * y + p2 * (r2 + 2.0 * (x * x)))
    g = y * kr + (p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * x * y)
    fx = kr + 2.0 * x * x * dkr + 2.0 * p1 * y + 6.0 * p2 * x
    fy = 2.0 * x * y * dkr + 2.0 * p1 * x + 2.0 * p2 * y
    gy = kr + 2.0 * y * y * dkr + 6.0 * p1 * y + 2.0 * p2 * x
    return f, g, fx, fy, fy, gy


def border_points(model, src_cam, coeffs, width, height, fov_max_deg=120.0):
    """-> dict: j, i (the border pixels, top row then bottom row then left column then right column; corners appear twice), x, y (their undistorted
    positions, clamped where they cannot be used), clamped (bool), edge (0 top, 1 bottom, 2 left, 3 right)"""
    fx, fy, cx, cy = (float(c) for c in src_cam)
    k = [float(c) for c in coeffs] + [0.0] * (8 - len(coeffs))
    cols, rows = np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64)
    j = np.concatenate([cols, cols, np.zeros(height), np.full(height, width - 1.0)])
    i = np.concatenate([np.zeros(width), np.full(width, height - 1.0), rows, rows])
    edge = np.concatenate([np.zeros(width, int), np.ones(width, int), np.full(height, 2), np.full(height, 3)])
    r_max = np.tan(fov_max_deg * (np.pi / 180.0) / 2.0)
    xd, yd = (j - cx) / fx, (i - cy) / fy
    rd = np.sqrt(xd * xd + yd * yd)
    n = len(j)
    active, failed = np.ones(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        if model == FISHEYE:
            th = rd.copy()
            for _ in range(ITERATIONS):
                t2 = th * th
                poly = 1.0 + (((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2
                d = 1.0 + (((9.0 * k[3] * t2 + 7.0 * k[2]) * t2 + 5.0 * k[1]) * t2 + 3.0 * k[0]) * t2
                s = (th * poly - rd) / d
                bad = active & ~np.isfinite(s)
                failed |= bad
                active &= ~bad
                th = np.where(active, th - s, th)
                active &= ~(np.abs(s) <= CONVERGED)
            t2 = th * th
            d = 1.0 + (((9.0 * k[3] * t2 + 7.0 * k[2]) * t2 + 5.0 * k[1]) * t2 + 3.0 * k[0]) * t2
            ok = ~active & ~failed & (d > 0.0) & (th >= 0.0) & (th < np.pi / 2.0)
            for q in range(1, RAY_STEPS):
                t2 = (th * (q / RAY_STEPS)) ** 2
                ok &= 1.0 + (((9.0 * k[3] * t2 + 7.0 * k[2]) * t2 + 5.0 * k[1]) * t2 + 3.0 * k[0]) * t2 > 0.0
            s = np.where(rd > 1e-8, np.tan(th) / np.where(rd > 1e-8, rd, 1.0), 1.0)
            x, y = xd * s, yd * s
        else:
            x, y = xd.copy(), yd.copy()
            for _ in range(ITERATIONS):
                f, g, jfx, jfy, jgx, jgy = _forward_brown(k, x, y)
                f, g = f - xd, g - yd
                det = jfx * jgy - jfy * jgx
                sx, sy = (jgy * f - jfy * g) / det, (jfx * g - jgx * f) / det
                bad = active & ~(np.isfinite(sx) & np.isfinite(sy))
                failed |= bad
                active &= ~bad
                x, y = np.where(active, x - sx, x), np.where(active, y - sy, y)
                active &= ~((np.abs(sx) <= CONVERGED) & (np.abs(sy) <= CONVERGED))
            _, _, jfx, jfy, jgx, jgy = _forward_brown(k, x, y)
            ok = ~active & ~failed & (jfx * jgy - jfy * jgx > 0.0) & (x * xd + y * yd >= 0.0)
            for q in range(1, RAY_STEPS):
                _, _, jfx, jfy, jgx, jgy = _forward_brown(k, x * (q / RAY_STEPS), y * (q / RAY_STEPS))
                ok &= jfx * jgy - jfy * jgx > 0.0
        r = np.sqrt(x * x + y * y)
        usable = ok & np.isfinite(r) & (r <= r_max)
        far = ok & np.isfinite(r) & ~usable
        rs, rds = np.where(far, r, 1.0), np.where(rd > 0.0, rd, 1.0)
        x = np.where(usable, x, np.where(far, x / rs * r_max, np.where(rd > 0.0, xd / rds * r_max, 0.0)))
        y = np.where(usable, y, np.where(far, y / rs * r_max, np.where(rd > 0.0, yd / rds * r_max, 0.0)))
    return dict(j=j, i=i, x=x, y=y, clamped=~usable, edge=edge)


def plan(model, src_cam, coeffs, size, alpha, out_size=None, max_dim=0, fov_max_deg=120.0):
    """-> (K 3 x 3, (width, height)); out_size None: the source size, "keep_focal": the size at which fx' = fx.  ValueError for what the planner refuses"""
    width, height = size
    fx, fy = float(src_cam[0]), float(src_cam[1])
    if model == 0:
        model, coeffs = BROWN, ()
    if model not in (BROWN, FISHEYE) or not np.all(np.isfinite(list(src_cam) + list(coeffs))) or not (fx > 0.0 and fy > 0.0):
        raise ValueError("lens")
    if model == FISHEYE and any(coeffs[4:]):
        raise ValueError("lens")

    def size_ok(w, h):
        return 8 <= w <= MAX_SIDE and 8 <= h <= MAX_SIDE and 3 * w * h <= MAX_BYTES
    if not size_ok(width, height) or not (0.0 <= alpha <= 1.0) or not (0.0 < fov_max_deg < 180.0) or max_dim < 0:
        raise ValueError("argument")
    keep_focal = isinstance(out_size, str) and out_size == "keep_focal"
    if out_size is not None and not keep_focal and not size_ok(*out_size):
        raise ValueError("output size")
    p = border_points(model, src_cam, coeffs, width, height, fov_max_deg)
    x, y, e = p["x"], p["y"], p["edge"]
    out_l, out_r, out_t, out_b = x.min(), x.max(), y.min(), y.max()
    in_l, in_r, in_t, in_b = x[e == 2].max(), x[e == 3].min(), y[e == 0].max(), y[e == 1].min()
    if not (in_r > in_l and in_b > in_t):
        raise ValueError("degenerate rectangle")
    l, r = in_l + alpha * (out_l - in_l), in_r + alpha * (out_r - in_r)
    t, b = in_t + alpha * (out_t - in_t), in_b + alpha * (out_b - in_b)
    aspect = fy / fx
    if keep_focal:
        f2 = fx
        w2 = int(np.floor(f2 * (r - l) + SIZE_SLACK)) + 1
        h2 = int(np.floor(f2 * aspect * (b - t) + SIZE_SLACK)) + 1
        if max_dim > 0 and max(w2, h2) > max_dim:
            f2 = fx * (float(max_dim) / float(max(w2, h2)))
            w2 = int(np.floor(f2 * (r - l) + SIZE_SLACK)) + 1
            h2 = int(np.floor(f2 * aspect * (b - t) + SIZE_SLACK)) + 1
        if not size_ok(w2, h2):
            raise ValueError("planned size")
    else:
        w2, h2 = (width, height) if out_size is None else out_size
        f0 = max((w2 - 1) / (in_r - in_l), (h2 - 1) / (aspect * (in_b - in_t)))
        f1 = min((w2 - 1) / (out_r - out_l), (h2 - 1) / (aspect * (out_b - out_t)))
        f2 = f0 + alpha * (f1 - f0)
    g2 = f2 * aspect
    K = np.array([[f2, 0.0, 0.5 * (w2 - 1) - f2 * (0.5 * (l + r))], [0.0, g2, 0.5 * (h2 - 1) - g2 * (0.5 * (t + b))], [0.0, 0.0, 1.0]])
    return K, (int(w2), int(h2))


# ---------------------------------------------------------------------------------------------------------------- the resampling
def is_pinhole(model, coeffs):
    return model == 0 or (model == BROWN and all(abs(float(c)) <= lm.EPS for c in coeffs))


def remap(img, out_size, out_cam, model, src_cam, coeffs, mask=None, border_mask=True):
    """img: uint8 h x w [x ch] (the source); out_size (w', h') or None; mask: None or h x w, non-zero = valid.  -> dict: image (h' x w' [x ch]),
    valid (h' x w' uint8, 255 / 0), u, v, inside, tie_margin, limit_distance (as lens_model.undistort gives them), resampled (bool)"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    ow, oh = (w, h) if out_size is None else out_size
    mk = None if mask is None else (np.asarray(mask) != 0)
    same_cam = src_cam is None or tuple(float(c) for c in src_cam) == tuple(float(c) for c in out_cam)
    if model is None or (is_pinhole(model, coeffs) and same_cam and (ow, oh) == (w, h)):
        assert (ow, oh) == (w, h)
        valid = np.full((h, w), 255, np.uint8) if mk is None else np.where(mk, 255, 0).astype(np.uint8)
        return dict(image=img.copy(), valid=valid, resampled=False)
    if model == 0:
        model, coeffs = BROWN, ()
    u, v = lm.source_coordinates(ow, oh, out_cam, model, src_cam, coeffs)
    with np.errstate(all="ignore"):
        inside = (u > -1.0) & (u < w) & (v > -1.0) & (v < h)
        tie = np.minimum(np.abs((32.0 * u - np.floor(32.0 * u)) - 0.5), np.abs((32.0 * v - np.floor(32.0 * v)) - 0.5))
        limit = np.minimum(np.minimum(np.abs(u + 1.0), np.abs(u - w)), np.minimum(np.abs(v + 1.0), np.abs(v - h)))
        iu = np.where(inside, np.rint(32.0 * np.where(inside, u, 0.0)), 0.0).astype(np.int64)
        iv = np.where(inside, np.rint(32.0 * np.where(inside, v, 0.0)), 0.0).astype(np.int64)
    x0, y0 = iu // 32, iv // 32
    a, b = iu - 32 * x0, iv - 32 * y0
    p = np.zeros((h + 2, w + 2) + img.shape[2:], np.int64)          # zero border: index + 1
    p[1:h + 1, 1:w + 1] = img
    pm = np.ones((h + 2, w + 2), bool)                               # the caller's plane; a tap off the source has no entry: left to the border rule
    if mk is not None:
        pm[1:h + 1, 1:w + 1] = mk
    ex = (lambda m: m[..., None]) if img.ndim == 3 else (lambda m: m)
    acc = np.zeros((oh, ow) + img.shape[2:], np.int64)
    off = np.zeros((oh, ow), bool)
    masked = np.zeros((oh, ow), bool)
    for dy, dx, wt in ((0, 0, (32 - a) * (32 - b)), (0, 1, a * (32 - b)), (1, 0, (32 - a) * b), (1, 1, a * b)):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        yi, xi = np.clip(yy, -1, h) + 1, np.clip(xx, -1, w) + 1
        acc += ex(wt) * p[yi, xi]
        off |= ~ok & (wt > 0)
        masked |= ok & (wt > 0) & ~pm[yi, xi]
    out = np.where(ex(inside), (acc + 512) >> 10, 0).astype(np.uint8)
    good = ~(inside & masked)
    if border_mask:
        good &= inside & ~off
    return dict(image=out, valid=np.where(good, 255, 0).astype(np.uint8), u=u, v=v, inside=inside, tie_margin=tie, limit_distance=limit, resampled=True)


# ---------------------------------------------------------------------------------------------------------------- validity at N x M
SCALE = 0.8


def _axis_taps(n_out, n_in):
    i = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * i + 1) * n_in - n_out, 0)
    den = 2 * n_out
    i0 = num // den
    a = ((num % den) * 256 + den // 2) // den
    last = i0 >= n_in - 1
    i0 = np.where(last, n_in - 1, i0)
    a = np.where(last, 0, a)
    return i0, np.minimum(i0 + 1, n_in - 1), a


def _sym(j, n):
    j = np.mod(j, 2 * n)
    return np.where(j >= n, 2 * n - 1 - j, j)


def working_size(width, height):
    return int(np.ceil(width * SCALE)), int(np.ceil(height * SCALE))


def defined_plane(valid, new_size=None):
    """valid: h x w, non-zero = valid, in the grid the detector reads (the remap's output).  new_size (nw, nh): the size the detector rescales to
    (None: none).  -> M x N uint8, 255 where the gradient pixel is defined by valid pixels alone, 0 elsewhere"""
    v = np.asarray(valid) != 0
    h, w = v.shape
    nw, nh = (w, h) if new_size is None else new_size
    if (nw, nh) != (w, h):                                           # the rescale: a tap counts iff its weight is not zero
        x0, x1, a = _axis_taps(nw, w)
        y0, y1, b = _axis_taps(nh, h)
        wx = ((256 - a) != 0, a != 0)
        wy = ((256 - b) != 0, b != 0)
        g = np.ones((nh, nw), bool)
        for yi, yw in ((y0, wy[0]), (y1, wy[1])):
            for xi, xw in ((x0, wx[0]), (x1, wx[1])):
                counts = yw[:, None] & xw[None, :]
                g &= ~counts | v[yi[:, None], xi[None, :]]
        v = g
    N, M = working_size(nw, nh)
    xc = np.floor(np.arange(N, dtype=np.float64) / SCALE + 0.5).astype(np.int64)
    yc = np.floor(np.arange(M, dtype=np.float64) / SCALE + 0.5).astype(np.int64)
    gx = np.ones((nh, N), bool)
    for t in range(-3, 4):
        gx &= v[:, _sym(xc + t, nw)]
    gy = np.ones((M, N), bool)
    for t in range(-3, 4):
        gy &= gx[_sym(yc + t, nh), :]
    x1, y1 = np.minimum(np.arange(N) + 1, N - 1), np.minimum(np.arange(M) + 1, M - 1)
    d = gy & gy[:, x1] & gy[y1, :] & gy[y1[:, None], x1[None, :]]
    return np.where(d, 255, 0).astype(np.uint8)


def footprint_distance(size, new_size=None):
    """an upper bound, in pixels of the grid the detector reads, on how far from an invalid pixel a gradient pixel can be undefined: the gradient's
    stencil (1 working pixel) and the two samplers' half width (3 taps of the rescaled grid around a centre rounded by up to 1/2) taken through
    1 / 0.8 and the rescale, plus the rescale's own tap"""
    w, h = size
    nw, nh = size if new_size is None else new_size
    up = max(w / nw, h / nh)
    return ((1.0 / SCALE) + 3.5) * up + up + 1.0


# ---------------------------------------------------------------------------------------------------------------- the cases of tests/test_gpu_remap.py
# (kernel against model), checked for what they claim and for their margins by tests/test_remap_cases_cpu.py.  Source sizes: lens_model.SIZES.  The
# lenses (the pinhole camera is resampled onto a camera of the table's own, the others onto the planner's -- this model's -- at the case's alpha)
LENSES = [
    ("tangential", BROWN, (0.0, 0.0, 0.05, -0.03)),
    ("rational", BROWN, (0.3, 0.0, 0.0, 0.0, 0.0, 0.12, 0.05, 0.02)),
    ("fisheye4", FISHEYE, (-0.04, 0.012, -0.005, 0.0015)),
    ("fisheye0", FISHEYE, ()),
    ("pinhole", 0, ()),
]
OUT_KINDS = ("equal", "smaller", "larger_one", "odd")
ALPHAS = (0.0, 0.5, 1.0)
FOCAL = 0.9             # the source camera's focal length as a share of lens_model's: a stronger lens at the same size
FOCAL_THIN_TANGENTIAL = 1.4     # ... but on the flattest size a tangential lens this strong shears the rows past each other (the planner refuses)


def out_size_of(kind, w, h):
    if kind == "equal":
        return (w, h)
    if kind == "smaller":
        return (max(8, (7 * w) // 10), max(8, (3 * h) // 5))
    if kind == "larger_one":
        return (w + 23, h)
    return (37, 29)


def case_mask(w, h):
    """holes at the image edge (a corner block, half of the last row) and in the middle"""
    m = np.full((h, w), 1, np.uint8)
    m[:max(1, h // 4), :max(1, w // 5)] = 0
    m[h - 1, w // 2:] = 0
    m[h // 2 - 1:h // 2 + 2, w // 2 - 2:w // 2 + 1] = 0
    return m


def _cases():
    cases = []
    for s, (w, h, ch, pad, f) in enumerate(lm.SIZES):
        for l, (name, model, coeffs) in enumerate(LENSES):
            kind, alpha = OUT_KINDS[(s + l) % 4], ALPHAS[(s + 2 * l) % 3]
            share = FOCAL_THIN_TANGENTIAL if name == "tangential" and w > 8 * h else FOCAL
            src = (share * f, share * f * 1.03125, 0.5 * w + 0.3, 0.5 * h - 0.2)
            ow, oh = out_size_of(kind, w, h)
            if model == 0:
                alpha = None
                out = (0.8 * src[0] * ow / w, 0.85 * src[1] * oh / h, 0.5 * ow - 0.45, 0.5 * oh + 0.35)
            else:
                K, _ = plan(model, src, coeffs, (w, h), alpha, (ow, oh))
                out = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
            masked = alpha != 0.0 and (s + l) % 2 == 1 and h > 8        # (on 8 rows the holes would leave little)
            cases.append(dict(name="%dx%dx%d_%s_%s_%s%s" % (w, h, ch, name, kind, "cam" if alpha is None else "a%g" % alpha, "_mask" if masked else ""),
                              size=(w, h, ch, pad), out_size=(ow, oh), kind=kind, alpha=alpha, out_cam=out, model=model, src_cam=src, coeffs=coeffs,
                              masked=masked))
    return cases


CASES = _cases()


def case_image(case, seed=5):
    """(array the call gets -- a view into padded rows where the case asks for them --, the same pixels contiguous, the mask or None)"""
    import undistort_model as um
    view, img = um.case_image(case["size"], seed)
    return view, img, (case_mask(*case["size"][:2]) if case["masked"] else None)


def case_model(case):
    _, img, mask = case_image(case)
    return remap(img, case["out_size"], case["out_cam"], case["model"], case["src_cam"], case["coeffs"], mask=mask)
