"""A float64 model of the device line segment detector, stage by stage, in plain numpy / scipy / mpmath (no GPU).

Written from the definitions in the header comment of line3d_amd/csrc/l3d_detect.hip and DESIGN.md section 4f: what every stage is
DEFINED to compute, evaluated in the most direct way.  Every threshold decision also reports its MARGIN (how far the compared quantity is
from the threshold), so that a test can tell a wrong kernel from a decision that sits on a rounding error.

    pixel_stage(img, new_size)            rescale + grey (detect_metric), Gaussian sub-sampling, 2x2 gradient, level-line angle, buckets
    label(bucket, active)                 8-connected components of equal bucket per partition, sizes, the vote
    region(mod, ang, pixels, min_reg, logNT)   seed, moments, rectangle, density, shrink, rectangle score, retries
    nfa_exact / nfa_float                 the binomial tail exactly (mpmath) / by the detector's stated recipe
    detect(img, ...)                      three rounds with release, then the selection
"""
import math

import numpy as np

import detect_metric as dm

SCALE, SIGMA_SCALE, QUANT, ANG_TH, DENSITY_TH = 0.8, 0.6, 2.0, 22.5, 0.7
NOTDEF = -1024.0
PREC = math.pi * ANG_TH / 180.0
P0 = ANG_TH / 180.0
RHO = QUANT / math.sin(PREC)
TAPS, HALF = 7, 3           # sigma = 0.6 / 0.8: half width ceil(sigma sqrt(2 x 3 ln 10)) = 3
ROUNDS = 3


def scaled_size(nw, nh):
    return int(math.ceil(nw * SCALE)), int(math.ceil(nh * SCALE))


def log_nt(N, M):
    return 5.0 * (math.log10(N) + math.log10(M)) / 2.0 + math.log10(11.0)


def min_region(N, M):
    return max(2, int(-log_nt(N, M) / math.log10(P0)))


# ---------------------------------------------------------------------------------------------------------------- pixel stage
def _sampler_axis(n_out, n_in):
    """-> (index (n_out, 7) into the input axis under the symmetric boundary, weights (n_out, 7))"""
    sigma = SIGMA_SCALE / SCALE
    x = np.arange(n_out, dtype=np.float64) / SCALE
    centre = np.floor(x + 0.5)
    i = np.arange(TAPS, dtype=np.float64)
    w = np.exp(-0.5 * ((i[None, :] - (HALF + x - centre)[:, None]) / sigma) ** 2)
    w /= w.sum(axis=1, keepdims=True)
    j = (centre[:, None] - HALF + i[None, :]).astype(np.int64) % (2 * n_in)         # ... c b a | a b c ... z | z y x ...
    j = np.where(j >= n_in, 2 * n_in - 1 - j, j)
    return j, w


def gaussian_sample(grey):
    """Gaussian sub-sampling by 0.8 of a (h, w) image, x pass then y pass, taps added in ascending order"""
    g = np.asarray(grey, dtype=np.float64)
    h, w = g.shape
    N, M = scaled_size(w, h)
    jx, wx = _sampler_axis(N, w)
    jy, wy = _sampler_axis(M, h)
    aux = np.zeros((h, N))
    for t in range(TAPS):
        aux += g[:, jx[:, t]] * wx[None, :, t]
    out = np.zeros((M, N))
    for t in range(TAPS):
        out += aux[jy[:, t], :] * wy[:, t, None]
    return out


def gradient(img):
    """-> (mod, ang, margin of the modulus against rho); the last row and column carry no gradient: 0 and NOTDEF"""
    M, N = img.shape
    mod, ang = np.zeros((M, N)), np.full((M, N), NOTDEF)
    a, b, c, d = img[:-1, :-1], img[:-1, 1:], img[1:, :-1], img[1:, 1:]
    com1, com2 = d - a, b - c
    gx, gy = com1 + com2, com1 - com2
    m = np.sqrt((gx * gx + gy * gy) / 4.0)
    mod[:-1, :-1] = m
    ang[:-1, :-1] = np.where(m > RHO, np.arctan2(gx, -gy), NOTDEF)
    margin = np.full((M, N), np.inf)
    margin[:-1, :-1] = np.abs(m - RHO)
    return mod, ang, margin


def buckets(ang):
    """angle -> bucket of 45 degrees in partition 0 ([-pi, -pi + pi/4) is bucket 0) and in partition 1 (shifted by 22.5 degrees);
    255 where the angle is not defined.  margin: distance of the angle to the nearest bucket boundary of each partition, in buckets"""
    defined = ang != NOTDEF
    t = (np.where(defined, ang, 0.0) + math.pi) / (math.pi / 4.0)
    b = np.stack([np.floor(t).astype(np.int64) & 7, np.floor(t + 0.5).astype(np.int64) & 7], axis=-1).astype(np.uint8)
    b[~defined] = 255
    margin = np.stack([np.abs(t - np.rint(t)), np.abs(t + 0.5 - np.rint(t + 0.5))], axis=-1)
    margin[~defined] = np.inf
    return b, margin


def pixel_stage(img, new_size=None):
    img = np.asarray(img)
    h, w = img.shape[:2]
    nw, nh = (w, h) if new_size is None else new_size
    grey = dm.grey_u8(dm.rescale_u8(img, nw, nh))
    sampled = gaussian_sample(grey)
    mod, ang, m_rho = gradient(sampled)
    bucket, m_bucket = buckets(ang)
    return {"grey": grey.astype(np.float32), "img": sampled, "mod": mod, "ang": ang, "bucket": bucket,
            "margin_rho": m_rho, "margin_bucket": m_bucket}


# ---------------------------------------------------------------------------------------------------------------- labelling, vote
def label(bucket, active):
    """bucket (M, N, 2), active (M, N) -> parent (2, M, N) int32: the smallest pixel index of the pixel's 8-connected component of equal
    bucket among the active pixels (-1: inactive); size (2, M, N): pixels of that component; key (M, N) uint32: partition x np + root of
    the larger of the pixel's two components (tie: partition 0), 2 np for an inactive pixel"""
    from scipy import ndimage
    bucket = np.asarray(bucket)
    act = np.asarray(active).astype(bool)
    M, N = act.shape
    np_ = M * N
    index = np.arange(np_, dtype=np.int64).reshape(M, N)
    parent = np.full((2, M, N), -1, np.int64)
    size = np.zeros((2, M, N), np.int64)
    for p in range(2):
        for v in np.unique(bucket[..., p][act]):
            lab, n = ndimage.label(act & (bucket[..., p] == v), structure=np.ones((3, 3), int))
            if n == 0:
                continue
            inside = lab > 0
            smallest = ndimage.minimum(index, lab, np.arange(1, n + 1)).astype(np.int64)
            count = np.bincount(lab[inside], minlength=n + 1)
            parent[p][inside] = smallest[lab[inside] - 1]
            size[p][inside] = count[lab[inside]]
    key = np.where(size[1] > size[0], np_ + parent[1], parent[0])
    key = np.where(act, key, 2 * np_).astype(np.uint32)
    return parent.astype(np.int32), size, key


# ---------------------------------------------------------------------------------------------------------------- NFA
def nfa_exact(n, k, p, logNT, digits=80):
    """-log10(NT x B(n, k, p)) with the binomial tail B summed exactly (every term, `digits` decimal digits)"""
    import mpmath as mp
    with mp.workdps(digits):
        n, k = int(n), int(k)
        p = mp.mpf(p)                              # (the double itself: exact)
        if n == 0 or k == 0:
            tail = mp.mpf(1)
        else:
            term = mp.binomial(n, k) * p ** k * (1 - p) ** (n - k)
            ratio = p / (1 - p)
            tail = term
            for i in range(k + 1, n + 1):
                term = term * (n - i + 1) / i * ratio
                tail += term
        return float(-mp.log10(tail) - mp.mpf(logNT))


def _log_gamma(x):
    if x > 15.0:            # Windschitl
        return 0.918938533204673 + (x - 0.5) * math.log(x) - x + 0.5 * x * math.log(x * math.sinh(1.0 / x) + 1.0 / (810.0 * x ** 6.0))
    q = (75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424, 2.50662827511)      # Lanczos
    a = (x + 0.5) * math.log(x + 5.5) - (x + 5.5)
    b = 0.0
    for i in range(7):
        a -= math.log(x + i)
        b += q[i] * x ** i
    return a + math.log(b)


FIRST_TERM_ZERO = 100.0 * 2.220446049250313e-16 * 2.2250738585072014e-308         # the reference's double_equal(term, 0)


DEVICE_ZERO = 100.0 * 2.2250738585072014e-308                                       # the device's: 100 DBL_MIN


def nfa_float(n, k, p, logNT, zero=FIRST_TERM_ZERO):
    """The detector's recipe in doubles: first term through log-gamma (Lanczos up to 15, Windschitl beyond); a first term that is zero
    (<= `zero`) stands for the tail when k > n p, and the tail counts as 1 otherwise; else terms are added until the bound on the rest
    is under a tenth of the result"""
    if n == 0 or k == 0:
        return -logNT
    if n == k:
        return -logNT - n * math.log10(p)
    ratio = p / (1.0 - p)
    log1 = _log_gamma(n + 1.0) - _log_gamma(k + 1.0) - _log_gamma(n - k + 1.0) + k * math.log(p) + (n - k) * math.log(1.0 - p)
    try:
        term = math.exp(log1)
    except OverflowError:
        term = math.inf
    if abs(term) <= zero:
        return -log1 / math.log(10.0) - logNT if k > n * p else -logNT
    tail = term
    for i in range(k + 1, n + 1):
        bin_term = (n - i + 1) * (1.0 / i)
        mult = bin_term * ratio
        term *= mult
        tail += term
        if bin_term < 1.0:
            err = term * ((1.0 - mult ** (n - i + 1)) / (1.0 - mult) - 1.0)
            if err < 0.1 * abs(-math.log10(tail) - logNT) * tail:
                break
    return -math.log10(tail) - logNT


# ---------------------------------------------------------------------------------------------------------------- regions
def _angle_dist(a, b):
    d = (a - b) % (2.0 * math.pi)
    return min(d, 2.0 * math.pi - d)


def rect_from_pixels(mod, ang, px):
    """Rectangle of the pixels px (flat indices): centre = gradient-weighted mean; axis = the inertia axis of the smaller eigenvalue,
    turned by pi when it is further than the tolerance from the mean level-line angle; extents along and across it from the centre (at
    least 0 either way); width at least 1.  -> dict, with the margin of the flip"""
    N = mod.shape[1]
    x, y = (px % N).astype(np.float64), (px // N).astype(np.float64)
    m, t = mod.ravel()[px], ang.ravel()[px]
    w = m.sum()
    cx, cy = (x * m).sum() / w, (y * m).sum() / w
    ixx, iyy, ixy = ((y - cy) ** 2 * m).sum(), ((x - cx) ** 2 * m).sum(), -((x - cx) * (y - cy) * m).sum()
    lam = 0.5 * (ixx + iyy - math.sqrt((ixx - iyy) ** 2 + 4.0 * ixy * ixy))
    theta = math.atan2(lam - ixx, ixy) if abs(ixx) > abs(iyy) else math.atan2(ixy, lam - iyy)
    mean = math.atan2(np.sin(t).sum(), np.cos(t).sum())
    away = _angle_dist(theta, mean)
    if away > PREC:
        theta += math.pi
    dx, dy = math.cos(theta), math.sin(theta)
    along, across = (x - cx) * dx + (y - cy) * dy, -(x - cx) * dy + (y - cy) * dx
    lmin, lmax = min(0.0, along.min()), max(0.0, along.max())
    wmin, wmax = min(0.0, across.min()), max(0.0, across.max())
    r = {"cx": cx, "cy": cy, "theta": theta, "dx": dx, "dy": dy, "x1": cx + lmin * dx, "y1": cy + lmin * dy, "x2": cx + lmax * dx, "y2": cy + lmax * dy,
         "width": max(wmax - wmin, 1.0), "prec": PREC, "p": P0, "reg_angle": mean, "margin_flip": abs(away - PREC)}
    r["length"] = math.hypot(r["x2"] - r["x1"], r["y2"] - r["y1"])
    r["density"] = len(px) / (r["length"] * r["width"])
    return r


def rect_count(r, ang):
    """-> (pts, alg, border margin, alignment margin): the pixels whose centre lies in the rectangle and those whose level-line angle is
    within r['prec'] of its angle; the smallest distance of a pixel centre to the rectangle's border (over the image pixels around it) and
    the smallest distance of an angle difference to the tolerance"""
    M, N = ang.shape
    hw = 0.5 * r["width"]
    length = math.hypot(r["x2"] - r["x1"], r["y2"] - r["y1"])
    cxs = [r["x1"] + s * r["dy"] * hw for s in (-1, 1)] + [r["x2"] + s * r["dy"] * hw for s in (-1, 1)]
    cys = [r["y1"] + s * r["dx"] * hw for s in (-1, 1)] + [r["y2"] + s * r["dx"] * hw for s in (-1, 1)]
    x0, x1 = max(0, int(math.floor(min(cxs))) - 1), min(N - 1, int(math.ceil(max(cxs))) + 1)
    y0, y1 = max(0, int(math.floor(min(cys))) - 1), min(M - 1, int(math.ceil(max(cys))) + 1)
    if x1 < x0 or y1 < y0:
        return 0, 0, math.inf, math.inf
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    ux, uy = xx - r["x1"], yy - r["y1"]
    a, b = ux * r["dx"] + uy * r["dy"], -ux * r["dy"] + uy * r["dx"]
    signed = np.minimum(np.minimum(a, length - a), hw - np.abs(b))          # >= 0 inside
    inside = signed >= 0.0
    t = ang[y0:y1 + 1, x0:x1 + 1]
    d = np.abs(r["theta"] - t)
    d = np.where(d > 1.5 * math.pi, np.abs(d - 2.0 * math.pi), d)
    defined = inside & (t != NOTDEF)
    aligned = defined & (d <= r["prec"])
    m_align = float(np.abs(d - r["prec"])[defined].min()) if defined.any() else math.inf
    return int(inside.sum()), int(aligned.sum()), float(np.abs(signed).min()), m_align


BORDER = 1e-6


def rect_count_bounds(r, ang):
    """The counts of rect_count when every pixel centre within BORDER of a side may fall either way (a rectangle from the moments has the
    region's two extreme pixels ON its end sides, so their membership is a matter of the last bit): -> (pts_lo, pts_hi, alg_lo, alg_hi)"""
    grown, shrunk = dict(r), dict(r)
    for q, e in ((grown, BORDER), (shrunk, -BORDER)):
        q["x1"], q["y1"], q["x2"], q["y2"] = r["x1"] - e * r["dx"], r["y1"] - e * r["dy"], r["x2"] + e * r["dx"], r["y2"] + e * r["dy"]
        q["width"] = r["width"] + 2.0 * e
    hi, lo = rect_count(grown, ang), rect_count(shrunk, ang)
    return lo[0], hi[0], lo[1], hi[1]


def rect_improve(r, ang, logNT, zero=FIRST_TERM_ZERO):
    """The rectangle's value; while it is not positive, the detector's variations in turn: precision halved five times, width cut by
    0.5 five times, one side moved in by 0.25 (width - 0.5) five times, the other side, precision halved five times again.  A stage keeps
    the best rectangle seen so far; the search stops after the stage in which the value turns positive.
    -> (final rectangle, value, pts, alg, {margins}, rectangles visited, the stage after which the value was positive: -1 the first score,
    0 .. 4, or None)"""
    def score(q):
        pts, alg, mb, ma = rect_count(q, ang)
        return nfa_float(pts, alg, q["p"], logNT, zero), pts, alg, mb, ma
    best = dict(r)
    v, pts, alg, mb, ma = score(best)
    margins = {"border": mb, "aligned": ma, "nfa": abs(v), "better": math.inf}
    visited = [dict(best)]
    if v > 0.0:
        return best, v, pts, alg, margins, visited, -1
    for stage in range(5):
        q = dict(best)
        for _ in range(5):
            if stage in (0, 4):
                q["p"] = q["p"] / 2.0
                q["prec"] = q["p"] * math.pi
            else:
                if q["width"] - 0.5 < 0.5:
                    continue
                s = (0.0, 0.25, -0.25)[stage - 1]
                q["x1"] += -q["dy"] * s
                q["y1"] += q["dx"] * s
                q["x2"] += -q["dy"] * s
                q["y2"] += q["dx"] * s
                q["width"] -= 0.5
            nv, npts, nalg, mb, ma = score(q)
            visited.append(dict(q))
            margins["border"], margins["aligned"] = min(margins["border"], mb), min(margins["aligned"], ma)
            if (npts, nalg, q["p"]) != (pts, alg, best["p"]):
                margins["better"] = min(margins["better"], abs(nv - v))
            if nv > v:
                v, pts, alg, best = nv, npts, nalg, dict(q)
        margins["nfa"] = min(margins["nfa"], abs(v))
        if v > 0.0:
            return best, v, pts, alg, margins, visited, stage
    return best, v, pts, alg, margins, visited, None


def region(mod, ang, pixels, min_reg, logNT, zero=FIRST_TERM_ZERO):
    """One region (flat pixel indices) -> record dict, or None for a region of fewer than min_reg pixels.
    The region is taken whole; while its density (pixels over rectangle area) is under 0.7 it is cut to the pixels within a radius of its
    strongest pixel (tie: the smallest index): the distance to the farther end point of the first rectangle, x 0.75 per step."""
    px = np.sort(np.asarray(pixels, dtype=np.int64))
    if len(px) < min_reg:
        return None
    N = mod.shape[1]
    m = mod.ravel()[px]
    seed = int(px[np.flatnonzero(m == m.max())[0]])
    sx, sy = float(seed % N), float(seed // N)
    dist = np.hypot((px % N) - sx, (px // N) - sy)
    rec = {"accepted": False, "scored": False, "seed": seed, "history": [],
           "margins": {"size": math.inf, "density": math.inf, "flip": math.inf, "radius": math.inf, "nfa": math.inf, "border": math.inf, "aligned": math.inf, "better": math.inf}}
    mg = rec["margins"]
    rad = None
    for step in range(64):
        used = px if rad is None else px[dist <= rad]
        if rad is not None:
            mg["radius"] = min(mg["radius"], float(np.abs(dist - rad).min()))
        rec["steps"], rec["n_used"], rec["used"] = step, len(used), used
        mg["size"] = min(mg["size"], abs(len(used) - (min_reg - 0.5)))
        if len(used) < min_reg or len(used) < 2:
            break
        r = rect_from_pixels(mod, ang, used)
        rec["rect"], rec["minpix"] = r, int(used[0])
        rec["history"].append((step, len(used), r["density"]))
        mg["flip"] = min(mg["flip"], r["margin_flip"])
        mg["density"] = min(mg["density"], abs(r["density"] - DENSITY_TH))
        if r["density"] >= DENSITY_TH:
            final, v, pts, alg, m2, visited, stage = rect_improve(r, ang, logNT, zero)
            rec.update(scored=True, final=final, nfa=v, pts=pts, alg=alg, accepted=v > 0.0, visited=visited, stage=stage)
            for k in ("nfa", "border", "aligned", "better"):
                mg[k] = min(mg[k], m2[k])
            # the first score when the pixels on the border may fall either way: lowest with the border's unaligned pixels in and its
            # aligned ones out, highest the other way round (a point more raises the tail, an aligned point more lowers it)
            plo, phi, alo, ahi = rect_count_bounds(r, ang)
            rec.update(first_counts=(plo, phi, alo, ahi), first_lo=nfa_float(phi - (ahi - alo), alo, r["p"], logNT, zero),
                       first_hi=nfa_float(plo + (ahi - alo), ahi, r["p"], logNT, zero))
            break
        if rad is None:
            rad = max(math.hypot(sx - r["x1"], sy - r["y1"]), math.hypot(sx - r["x2"], sy - r["y2"]))
        rad *= 0.75
    return rec


def search_rule(rec, decision=1e-6, aligned=1e-9):
    """How far a scored region's rectangle search can be compared with another implementation of the same definitions:
    'exact'  no pixel centre within BORDER of a side of any rectangle visited, no angle within `aligned` of a tolerance, no value within
             `decision` of 0 or of the value it is compared with: counts, value, acceptance and the final rectangle must coincide;
    'first'  pixels sit on the border (the two extreme pixels of the region always lie ON the end sides of its first rectangle), but the
             first score is positive by more than `decision` whichever way they fall: accepted at once, the rectangle stays the first one,
             the counts lie between the bounds;
    None     neither: the outcome may depend on the last bit"""
    mg = rec["margins"]
    if not rec["scored"] or mg["aligned"] <= aligned:
        return None
    if mg["border"] > BORDER and mg["nfa"] > decision and mg["better"] > decision:
        return "exact"
    return "first" if rec["first_lo"] > decision else None


def regions_of_key(key):
    """key (M, N) of the vote -> list of (key value, ascending flat pixel indices) in ascending key order, 2 np left out"""
    k = np.asarray(key).ravel()
    order = np.argsort(k, kind="stable")
    ks = k[order]
    cut = np.flatnonzero(np.diff(ks)) + 1
    out = []
    for idx in np.split(order, cut):
        if len(idx) and k[idx[0]] < 2 * k.size:
            out.append((int(k[idx[0]]), idx.astype(np.int64)))
    return out


# ---------------------------------------------------------------------------------------------------------------- the whole detector
def detect(img, new_size=None, min_length=None, max_segments=3000, zero=FIRST_TERM_ZERO):
    """-> (segments (n, 4) float32 in pixels of `img`, smallest decision margin by kind; 'undecided': scored regions search_rule leaves open)"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    nw, nh = (w, h) if new_size is None else new_size
    if min_length is None:
        min_length = float(np.float32(0.005) * np.sqrt(np.float32(h * h + w * w)))
    ps = pixel_stage(img, new_size)
    mod, ang, bucket = ps["mod"], ps["ang"], ps["bucket"]
    M, N = mod.shape
    logNT, min_reg = log_nt(N, M), min_region(N, M)
    margins = {"rho": float(ps["margin_rho"].min()), "bucket": float(ps["margin_bucket"].min()), "length": math.inf, "undecided": 0}
    active = ang != NOTDEF
    cands = []
    for _ in range(ROUNDS):
        _, _, key = label(bucket, active)
        for _, px in regions_of_key(key):
            rec = region(mod, ang, px, min_reg, logNT, zero)
            if rec is None:
                margins["size"] = min(margins.get("size", math.inf), abs(len(px) - (min_reg - 0.5)))
                continue
            for k in ("size", "density", "flip", "radius"):
                margins[k] = min(margins.get(k, math.inf), rec["margins"][k])
            if rec["scored"]:
                how = search_rule(rec)
                margins["undecided"] += how is None
                margins["aligned"] = min(margins.get("aligned", math.inf), rec["margins"]["aligned"])
                margins["search"] = min(margins.get("search", math.inf), rec["first_lo"] if how == "first" else min(rec["margins"]["nfa"], rec["margins"]["better"]))
            if rec["accepted"]:
                f = rec["final"]
                cands.append(((f["x1"] + 0.5) / SCALE, (f["y1"] + 0.5) / SCALE, (f["x2"] + 0.5) / SCALE, (f["y2"] + 0.5) / SCALE, rec["minpix"]))
                active.ravel()[rec["used"]] = False
    up = dm.upscale_factor(w, h, nw, nh)
    out = []
    for x1, y1, x2, y2, minpix in cands:
        s = np.array([x1, y1, x2, y2]).astype(np.float32) * np.float32(up)
        dx, dy = s[0] - s[2], s[1] - s[3]
        length = np.sqrt(dx * dx + dy * dy)
        margins["length"] = min(margins["length"], abs(float(length) - min_length))
        if length > np.float32(min_length):
            out.append((-float(length), minpix, s))
    out.sort(key=lambda t: (t[0], t[1]))
    segs = np.array([t[2] for t in out[:max_segments]], np.float32).reshape(-1, 4)
    return segs, margins
