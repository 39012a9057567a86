"""The segment-mask contract of include/line3d_amd.h ("A SEGMENT MASK") in numpy (float64 / int64): what l3d_mask_segments and
l3d_test_mask_segments_host must give bit for bit.  Written from the header's words:

    dx = x2 - x1, dy = y2 - y1, m = max(|dx|, |dy|), n = floor(m) + 1; sample k = 0..n: t = k / n, px = x1 + t dx, py = y1 + t dy
    no lens: the sample reads mask pixel (floor(px + 0.5), floor(py + 0.5)); outside the mask: invalid; valid iff byte >= threshold (0 reads as 1)
    a lens:  (px, py) through the formulas of A LENS with j = px, i = py -> (u, v), the pixel is (floor(u + 0.5), floor(v + 0.5)); not finite: invalid
    always dropped: a coordinate that is not finite, dx == dy == 0, m >= 65536
    DROP:   V valid samples, kept iff V 1000 >= keep_permille (n + 1); a kept segment keeps its bits
    CLIP / SPLIT: a run of at most max_gap invalid samples strictly between two valid samples counts as valid; a run [a, b] is a maximal run of
            valid samples with a < b; it passes iff (s s) L2 >= min_length min_length, s = (b - a) / n, L2 = dx dx + dy dy.  CLIP: the run with the
            largest b - a (the first on a tie) if it passes; SPLIT: every passing run in ascending a.  End points: the sample rounded to f32, the
            input's bits where a == 0 (x1, y1) and where b == n (x2, y2)
    output: input order, runs in order along the segment, src_index per output segment

Every product and sum is one numpy operation on float64 arrays or scalars: nothing is fused.  The lens formulas are those of tests/lens_model.py
(source_coordinates), which evaluates them on the integer pixel grid only; lens_point below is the same sequence of operations at any position, and
tests/test_segmask_cases_cpu.py holds the two against each other on the grid."""
import numpy as np

import lens_model as lm

DROP, CLIP, SPLIT = 0, 1, 2
BROWN, FISHEYE = lm.BROWN, lm.FISHEYE


def lens_point(px, py, out_cam, model, src_cam, coeffs):
    """A LENS at positions (px, py) (float64 arrays): -> (u, v).  out_cam: the segments' camera; src_cam: the lens's (None: out_cam)"""
    ofx, ofy, ocx, ocy = (np.float64(c) for c in out_cam)
    fx, fy, cx, cy = (np.float64(c) for c in (out_cam if src_cam is None else src_cam))
    k = [np.float64(c) for c in coeffs] + [np.float64(0.0)] * (8 - len(coeffs))
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    with np.errstate(all="ignore"):
        x = (px - ocx) / ofx
        y = (py - ocy) / ofy
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


def samples(seg):
    """-> None for a segment that is always dropped, else (n, px, py, dx, dy): px, py float64 arrays of n + 1 samples"""
    x1, y1, x2, y2 = (np.float64(v) for v in np.asarray(seg, np.float32))
    if not (np.isfinite(x1) and np.isfinite(y1) and np.isfinite(x2) and np.isfinite(y2)):
        return None
    dx, dy = x2 - x1, y2 - y1
    m = max(abs(dx), abs(dy))
    if (dx == 0.0 and dy == 0.0) or m >= 65536.0:
        return None
    n = int(np.floor(m)) + 1
    t = np.arange(n + 1, dtype=np.float64) / np.float64(n)
    return n, x1 + t * dx, y1 + t * dy, dx, dy


def mask_positions(px, py, lens):
    """where the samples read the mask: (u, v) float64; lens: None, or dict(out_cam, model, src_cam, coeffs) -- an inactive lens is no lens"""
    if lens is None or not lm.is_active(lens["out_cam"], lens["model"], lens["src_cam"], lens["coeffs"]):
        return px, py
    return lens_point(px, py, lens["out_cam"], lens["model"], lens["src_cam"], lens["coeffs"])


def validity(seg, mask, threshold=1, lens=None):
    """-> None (always dropped) or (n, bool array of n + 1 samples)"""
    sm = samples(seg)
    if sm is None:
        return None
    n, px, py = sm[:3]
    u, v = mask_positions(px, py, lens)
    mask = np.asarray(mask).view(np.uint8) if np.asarray(mask).dtype == np.bool_ else np.asarray(mask)
    h, w = mask.shape
    thr = 1 if threshold == 0 else int(threshold)
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = np.isfinite(u) & np.isfinite(v) & (fu >= 0) & (fu < w) & (fv >= 0) & (fv < h)
    iu = np.where(inside, fu, 0).astype(np.int64)
    iv = np.where(inside, fv, 0).astype(np.int64)
    return n, inside & (mask[iv, iu].astype(np.int64) >= thr)


def bridge(valid, max_gap):
    """a run of at most max_gap invalid samples strictly between two valid samples counts as valid"""
    out = valid.copy()
    idx = np.flatnonzero(valid)
    for a, b in zip(idx[:-1], idx[1:]):
        if 0 < b - a - 1 <= max_gap:
            out[a + 1:b] = True
    return out


def runs(valid):
    """maximal runs [a, b] of valid samples with a < b, ascending"""
    out, k, n1 = [], 0, len(valid)
    while k < n1:
        if not valid[k]:
            k += 1
            continue
        a = k
        while k + 1 < n1 and valid[k + 1]:
            k += 1
        if a < k:
            out.append((a, k))
        k += 1
    return out


def filter_segments(segments, mask, mode=DROP, threshold=1, keep_permille=500, max_gap=0, min_length=0.0, lens=None):
    """-> (segments (k, 4) float32, src_index (k,) int32)"""
    segments = np.asarray(segments, np.float32).reshape(-1, 4)
    out, src = [], []
    for i, seg in enumerate(segments):
        val = validity(seg, mask, threshold, lens)
        if val is None:
            continue
        n, valid = val
        if mode == DROP:
            V = int(np.count_nonzero(valid))
            if V * 1000 >= int(keep_permille) * (n + 1):
                out.append(seg.copy())
                src.append(i)
            continue
        _, px, py, dx, dy = samples(seg)
        L2 = dx * dx + dy * dy
        ml2 = np.float64(min_length) * np.float64(min_length)

        def passes(a, b):
            s = np.float64(b - a) / np.float64(n)
            return (s * s) * L2 >= ml2

        def emit(a, b):
            o = np.array([px[a], py[a], px[b], py[b]], np.float64).astype(np.float32)
            if a == 0:
                o[0:2] = seg[0:2]
            if b == n:
                o[2:4] = seg[2:4]
            out.append(o)
            src.append(i)

        rr = runs(bridge(valid, int(max_gap)))
        if mode == SPLIT:
            for a, b in rr:
                if passes(a, b):
                    emit(a, b)
        elif mode == CLIP:
            if rr:
                best = rr[0]
                for a, b in rr[1:]:
                    if b - a > best[1] - best[0]:
                        best = (a, b)
                if passes(*best):
                    emit(*best)
        else:
            raise ValueError("mode")
    segs = np.array(out, np.float32).reshape(-1, 4)
    return segs, np.array(src, np.int32)
