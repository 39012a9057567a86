"""Agreement measure between two sets of 2-D line segments (the detector against the reference detector, and the reference
against itself under redrawn noise).  The parameters are fixed: the same for every comparison.

cover(A, B): every segment of A is sampled every STEP px; a sample is covered when some segment b of B
  * lies within ANGLE_DEG of the sample's segment (as undirected lines),
  * has the sample within PERP px perpendicular distance, and
  * has the sample within [-ALONG, len_b + ALONG] along it.
The result is the covered share of A's total length.  Pooled figures weight the images by that length."""
import numpy as np

STEP = 0.5
ANGLE_DEG = 5.0
PERP = 1.5          # half of the narrower rectangles the reference reports on the golden images
ALONG = 1.5


def _xy(S):
    S = np.asarray(S, dtype=np.float64)
    return S.reshape(-1, S.shape[-1])[:, :4] if S.size else np.zeros((0, 4))


def cover_lengths(A, B):
    """-> (covered length of A, total length of A)"""
    A, B = _xy(A), _xy(B)
    la = np.hypot(A[:, 2] - A[:, 0], A[:, 3] - A[:, 1])
    total = 0.0
    for l in la:                # (the same order of additions as `covered` below: a fully covered set gives exactly 1)
        total += float(l)
    if len(A) == 0 or len(B) == 0:
        return 0.0, total
    lb = np.hypot(B[:, 2] - B[:, 0], B[:, 3] - B[:, 1])
    okb = lb > 0
    B, lb = B[okb], lb[okb]
    if len(B) == 0:
        return 0.0, total
    db = (B[:, 2:4] - B[:, 0:2]) / lb[:, None]
    cos_min = np.cos(np.deg2rad(ANGLE_DEG))
    covered = 0.0
    for a, l in zip(A, la):
        if l <= 0:
            continue
        da = (a[2:4] - a[0:2]) / l
        cand = np.abs(db @ da) >= cos_min
        if not cand.any():
            continue
        t = np.arange(0.0, l + 1e-9, STEP)
        P = a[0:2][None, :] + t[:, None] * da[None, :]                    # m x 2
        rel = P[:, None, :] - B[cand][None, :, 0:2]                       # m x k x 2
        d = db[cand]
        along = rel[..., 0] * d[None, :, 0] + rel[..., 1] * d[None, :, 1]
        perp = np.abs(rel[..., 0] * d[None, :, 1] - rel[..., 1] * d[None, :, 0])
        hit = (perp <= PERP) & (along >= -ALONG) & (along <= lb[cand][None, :] + ALONG)
        covered += float(l) * float(hit.any(axis=1).mean())
    return covered, total


def cover(A, B):
    c, t = cover_lengths(A, B)
    return c / t if t > 0 else 0.0


def pooled(pairs):
    """pairs of (A, B) -> length-weighted cover over the images"""
    c = t = 0.0
    for A, B in pairs:
        ci, ti = cover_lengths(A, B)
        c += ci
        t += ti
    return c / t if t > 0 else 0.0


def reference_floor(refs_a, refs_b):
    """worst single-image repeatability of the reference against itself, both directions"""
    return min(min(cover(a, b), cover(b, a)) for a, b in zip(refs_a, refs_b))


# ---- the stated integer formulas of the rescale + grey stage (include/line3d_amd.h), in numpy: what the generator feeds the reference ----
def _axis(n_out, n_in):
    i = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * i + 1) * n_in - n_out, 0)
    den = 2 * n_out
    i0 = num // den
    a = ((num % den) * 256 + den // 2) // den
    last = i0 >= n_in - 1
    i0 = np.where(last, n_in - 1, i0)
    a = np.where(last, 0, a)
    return i0, np.minimum(i0 + 1, n_in - 1), a


def rescale_u8(img, new_w, new_h):
    img = np.asarray(img)
    h, w = img.shape[:2]
    if (new_w, new_h) == (w, h):
        return img.copy()
    x0, x1, a = _axis(new_w, w)
    y0, y1, b = _axis(new_h, h)
    p = img.astype(np.int64).reshape(h, w, -1)
    a = a[None, :, None]
    b = b[:, None, None]
    v = ((256 - a) * (256 - b) * p[y0][:, x0] + a * (256 - b) * p[y0][:, x1] + (256 - a) * b * p[y1][:, x0] + a * b * p[y1][:, x1] + 32768) >> 16
    return v.astype(np.uint8).reshape((new_h, new_w) + img.shape[2:])


def grey_u8(img):
    img = np.asarray(img)
    if img.ndim == 2:
        return img.copy()
    p = img.astype(np.int64)
    return ((299 * p[..., 0] + 587 * p[..., 1] + 114 * p[..., 2] + 500) // 1000).astype(np.uint8)


def upscale_factor(w, h, new_w, new_h):
    if (new_w, new_h) == (w, h):
        return np.float32(1.0)
    wd = np.float32(new_w) / np.float32(w)
    hd = np.float32(new_h) / np.float32(h)
    return np.float32(1.0) / (np.float32(0.5) * (wd + hd))
