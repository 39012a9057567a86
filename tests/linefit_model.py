"""The line fit of processClusteredSegments (line3D.cc:1392-1597: getLineEquation3D + projectToLine) restated in plain numpy float64 --
the reference the device fit (l3d_linefit.hip) is tested against.  It shares nothing with l3d_linefit.hpp: the direction comes
from numpy.linalg.eigh of the scatter of the CENTRED points (the product runs its own Jacobi iteration, the oracle's align() an SVD of the
uncentred product), only the conventions are the same -- the component of largest magnitude of the direction is positive, the float32
distance from the projected end point farthest against the direction is the sort key, the order is stable.

What the model returns is the STRUCTURE of a cluster's fit: which input points the sweep emits.  Points are numbered 2 * member + {0: P1, 1: P2}.
The sweep emits input points, not projected ones, so a fit is right exactly when its end points ARE those input points.

linefit_conditions() measures how far a cluster is from the inputs on which two correct implementations may legitimately differ
(two points whose float32 distances could swap, a scatter without a clear first axis, a direction whose sign rule could flip)."""
import numpy as np

K_FIT_LDS = 128          # l3d_linefit.hip: members whose sweep state fits the per-wave LDS arrays
K_REG_CAMS = 64          # ... and cameras the register sweep has lanes for


def inverse_transform(P, Rinv, scale_inv, tneg):
    """Line3D::inverseTransform (line3D.cc:1782-1786) on rows of P, float64"""
    P = np.asarray(P, np.float64)
    return (np.asarray(Rinv, np.float64) @ (P * float(scale_inv) + np.asarray(tneg, np.float64)).T).T


def line_of_points(pts):
    """-> (Pc, direction, min_point, eigenvalues ascending)"""
    pts = np.asarray(pts, np.float64)
    n2 = len(pts)
    Pc = np.zeros(3)
    for p in pts:
        Pc = Pc + p
    Pc = Pc / float(n2)
    D = pts - Pc
    w, V = np.linalg.eigh(D.T @ D)
    d = V[:, int(np.argmax(w))].copy()
    d = d / np.linalg.norm(d)
    if d[int(np.argmax(np.abs(d)))] < 0:
        d = -d
    dn2 = float(np.linalg.norm(d)) * float(np.linalg.norm(d))
    min_point, min_length = np.zeros(3), 0.0
    for p in pts:
        proj = Pc + (float(d @ (p - Pc)) / dn2) * d
        loc = float(d @ (Pc - proj))
        if loc <= min_length:
            min_length, min_point = loc, proj
    return Pc, d, min_point, w


def sweep(order, cams):
    """projectToLine's sweep (:1543-1594) over the points in `order`; cams[member] -> list of (start point, end point),
    the number of distinct cameras met up to each step is of no concern here"""
    open_lines, open_cams = set(), {}
    opened, start, out = False, -1, []
    for p in order:
        p = int(p)
        member = p >> 1
        cam = int(cams[member])
        if member not in open_lines:
            open_lines.add(member)
            open_cams[cam] = open_cams.get(cam, 0) + 1
        else:
            open_lines.discard(member)
            open_cams[cam] -= 1
            if open_cams[cam] == 0:
                del open_cams[cam]
        if opened and len(open_cams) < 3:
            out.append((start, p))
            opened = False
        elif not opened and len(open_cams) >= 3:
            start, opened = p, True
    return out


def fit_cluster(pts, cams):
    """pts (2 * members, 3): the inverse-transformed end points in member order; cams (members,) -> dict:
    structure [(start point index, end point index)], order (the sweep order), dist64, dist32, w (eigenvalues), dir"""
    pts = np.asarray(pts, np.float64)
    if len(pts) == 0:
        return {"structure": [], "order": np.zeros(0, np.int64), "dist64": np.zeros(0), "dist32": np.zeros(0, np.float32), "w": np.zeros(3), "dir": np.zeros(3)}
    _Pc, d, min_point, w = line_of_points(pts)
    dist64 = np.sqrt(((pts - min_point) ** 2).sum(axis=1))
    dist32 = dist64.astype(np.float32)
    order = np.argsort(dist32, kind="stable")
    return {"structure": sweep(order, cams), "order": order, "dist64": dist64, "dist32": dist32, "w": w, "dir": d}


def path_of(members, cams):
    """Which of k_fit_clusters' four paths a cluster takes: 'lo' (<= 64 members, register sweep, one mask), 'hi' (65-128 members, both
    masks), 'overflow' (<= 128 members, a 65th distinct camera turns up in the sweep) or 'global' (> 128 members)."""
    if members > K_FIT_LDS:
        return "global"
    if len({int(c) for c in cams}) > K_REG_CAMS:           # (every member's first point registers its camera: all cameras are met)
        return "overflow"
    return "lo" if members <= 64 else "hi"


def overflow_step(cams, order):
    """the sweep step (index into order) at which the 65th distinct camera is met, or -1"""
    seen = set()
    for k, p in enumerate(order):
        seen.add(int(cams[int(p) >> 1]))
        if len(seen) > K_REG_CAMS:
            return k
    return -1


def linefit_conditions(pts, fit):
    """-> dict of the three margins of the issue's conditions:
    gap_ulps: the smallest difference of neighbouring float64 distances (bit-identical points excepted) in float32 ulps of the largest distance,
    eig_ratio: largest / second eigenvalue of the scatter, dir_gap: |largest| - |second| component of the direction"""
    pts = np.asarray(pts, np.float64)
    d = fit["dist64"]
    o = np.argsort(d, kind="stable")
    ulp = float(np.spacing(np.float32(d.max()))) if d.max() > 0 else 0.0
    gap = np.inf
    for a, b in zip(o[:-1], o[1:]):
        if pts[a].tobytes() == pts[b].tobytes():
            continue
        gap = min(gap, (d[b] - d[a]) / ulp if ulp else np.inf)
    w = np.sort(fit["w"])
    comp = np.sort(np.abs(fit["dir"]))
    return {"gap_ulps": float(gap), "eig_ratio": float(w[2] / w[1]) if w[1] > 0 else np.inf, "dir_gap": float(comp[2] - comp[1]),
            "all_identical": bool(all(p.tobytes() == pts[0].tobytes() for p in pts))}
