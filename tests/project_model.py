"""The projection rules of include/line3d_amd.h ("PROJECTION AND OVERLAYS", 1) in numpy float64 scalars: camera frame, near plane, pixel map, the
rectangle rule (Liang-Barsky, edges left, right, top, bottom) and the output.  Every product, sum and quotient is one numpy operation, so each is
rounded on its own.  Shares no code with the product."""
import numpy as np

F = np.float64


def rect(width, height, margin):
    m = F(margin)
    return F(-0.5) - m, (F(width) - F(0.5)) + m, F(-0.5) - m, (F(height) - F(0.5)) + m


def clip(uP, vP, du, dv, r):
    """the rectangle rule -> (t0, t1) when kept, None when dropped; `trace` of the last call: t0, t1 as they stood when the rule ended"""
    xmin, xmax, ymin, ymax = r
    t0, t1 = F(0.0), F(1.0)
    clip.trace = None
    for p, q in ((-du, uP - xmin), (du, xmax - uP), (-dv, vP - ymin), (dv, ymax - vP)):
        if p == 0:
            if q < 0:
                return None
            continue
        rr = q / p
        if p < 0:
            if rr > t1:
                return None
            t0 = max(t0, rr)
        else:
            if rr < t0:
                return None
            t1 = min(t1, rr)
    clip.trace = (t0, t1)
    return (t0, t1) if t0 < t1 else None


clip.trace = None


def camera_frame(R, t, X):
    R, t, X = np.asarray(R, F).reshape(3, 3), np.asarray(t, F).reshape(3), np.asarray(X, F).reshape(3)
    return [((R[r, 0] * X[0] + R[r, 1] * X[1]) + R[r, 2] * X[2]) + t[r] for r in range(3)]


def pair(cam, seg, near, margin):
    """one (camera, segment) pair -> None (dropped) or (4 float32, flags); cam = (K, R, t, width, height)"""
    K, R, t, width, height = cam
    K = np.asarray(K, F).reshape(9)
    near = F(near)
    with np.errstate(all="ignore"):
        P, Q = camera_frame(R, t, seg[:3]), camera_frame(R, t, seg[3:])
        if not all(np.isfinite(v) for v in P + Q):
            return None
        movedP = movedQ = False
        if P[2] < near and Q[2] < near:
            return None
        if P[2] < near:
            s = (near - P[2]) / (Q[2] - P[2])
            P = [P[0] + s * (Q[0] - P[0]), P[1] + s * (Q[1] - P[1]), near]
            movedP = True
        elif Q[2] < near:
            s = (near - Q[2]) / (P[2] - Q[2])
            Q = [Q[0] + s * (P[0] - Q[0]), Q[1] + s * (P[1] - Q[1]), near]
            movedQ = True

        def pix(p):
            xn, yn = p[0] / p[2], p[1] / p[2]
            return (K[0] * xn + K[1] * yn) + K[2], (K[3] * xn + K[4] * yn) + K[5]

        (uP, vP), (uQ, vQ) = pix(P), pix(Q)
        du, dv = uQ - uP, vQ - vP
        if not all(np.isfinite(v) for v in (uP, vP, uQ, vQ, du, dv)):
            return None
        if du == 0 and dv == 0:
            return None
        tt = clip(uP, vP, du, dv, rect(width, height, margin))
        if tt is None:
            return None
        t0, t1 = tt
        a = (uP, vP) if t0 == 0 else (uP + t0 * du, vP + t0 * dv)
        b = (uQ, vQ) if t1 == 1 else (uP + t1 * du, vP + t1 * dv)
        flags = (1 if (movedP or t0 > 0) else 0) | (2 if (movedQ or t1 < 1) else 0)
        return np.array([a[0], a[1], b[0], b[1]], F).astype(np.float32), flags


def project(seg3d, cams, near=1e-6, margin=0.0):
    """-> (seg2d (k, 4) float32, src_index (k,) int32, flags (k,) uint8, cam_start (m + 1,) int64): camera-major, input order within a camera"""
    seg3d = np.asarray(seg3d, F).reshape(-1, 6)
    segs, src, fl, start = [], [], [], [0]
    for cam in cams:
        for i, s in enumerate(seg3d):
            got = pair(cam, s, near, margin)
            if got is not None:
                segs.append(got[0]); src.append(i); fl.append(got[1])
        start.append(len(src))
    return (np.array(segs, np.float32).reshape(-1, 4), np.array(src, np.int32), np.array(fl, np.uint8), np.array(start, np.int64))
