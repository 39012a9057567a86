"""numpy float64 model of the line refinement, written from the header comment of line3d_amd/csrc/l3d_refine.hpp -- it shares no code with the
product.  Every sum runs sequentially over the members (numpy's own order), NOT in the product's 64 lane-strided partial sums with their xor tree:
the model is deliberately not bit-comparable with the product; tests/golden/make_golden_refine.py measures what a change of order may cost."""
import numpy as np

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-12, 1e12
N2_MIN, DEC_REL, PARALLEL = 1e-300, 1e-14, 1e-12


def camera_parts(P):
    """P (3, 4) -> M, p4, Minv, C = -Minv p4"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    M, p4 = P[:, :3], P[:, 3]
    with np.errstate(all="ignore"):
        Minv = np.linalg.inv(M) if abs(np.linalg.det(M)) > 0 else np.full((3, 3), np.nan)
    return M, p4, Minv, -Minv @ p4


def sign_rule(d):
    """the component of largest magnitude (first on ties) positive"""
    k = int(np.argmax(np.abs(d)))
    return -d if d[k] < 0 else d


def line_of_points(pts):
    """centre and principal direction of the points (the start of the refinement)"""
    Pc = pts.mean(axis=0)
    q = pts - Pc
    w, V = np.linalg.eigh(q.T @ q)
    d = V[:, int(np.argmax(w))]
    return Pc, sign_rule(d / np.linalg.norm(d))


def basis(d):
    k = int(np.argmin(np.abs(d)))                  # first on ties
    e = np.zeros(3)
    e[k] = 1.0
    u = np.cross(d, e)
    u = u / np.linalg.norm(u)
    return u, np.cross(d, u)


def member_lines(cams, member_cam, A, d):
    """per member: l = p x g, n2, and whether the n2 rule drops it"""
    out = []
    for c in member_cam:
        M, p4 = cams[c][0], cams[c][1]
        p, g = M @ A + p4, M @ d
        l = np.cross(p, g)
        n2 = l[0] * l[0] + l[1] * l[1]
        out.append((p, g, l, n2, (not np.isfinite(n2)) or n2 < N2_MIN))
    return out


def residuals(cams, member_cam, seg, A, d):
    """(r (n, 2) with NaN for dropped members, dropped (n,) bool)"""
    n = len(member_cam)
    r, dropped = np.full((n, 2), np.nan), np.zeros(n, bool)
    for m, (p, g, l, n2, drop) in enumerate(member_lines(cams, member_cam, A, d)):
        dropped[m] = drop
        if drop:
            continue
        for j in range(2):
            r[m, j] = (l[0] * seg[m, 2 * j] + l[1] * seg[m, 2 * j + 1] + l[2]) / np.sqrt(n2)
    return r, dropped


def jacobian(cams, member_cam, seg, A, d):
    """analytic d r / d (a, b, c', e') at 0: (n, 2, 4), NaN rows for dropped members"""
    u, v = basis(d)
    J = np.full((len(member_cam), 2, 4), np.nan)
    for m, (p, g, l, n2, drop) in enumerate(member_lines(cams, member_cam, A, d)):
        if drop:
            continue
        M = cams[member_cam[m]][0]
        n = np.sqrt(n2)
        dl = [np.cross(M @ u, g), np.cross(M @ v, g), np.cross(p, M @ u), np.cross(p, M @ v)]
        for j in range(2):
            x = np.array([seg[m, 2 * j], seg[m, 2 * j + 1], 1.0])
            s = l @ x
            for i in range(4):
                J[m, j, i] = (dl[i] @ x) / n - s * (l[0] * dl[i][0] + l[1] * dl[i][1]) / n ** 3
    return J


def apply(A, d, delta, Pc0=None):
    """the local parameters applied to a state; Pc0 given: re-centred"""
    u, v = basis(d)
    A1 = A + delta[0] * u + delta[1] * v
    d1 = d + delta[2] * u + delta[3] * v
    d1 = d1 / np.linalg.norm(d1)
    if Pc0 is not None:
        A1 = A1 + ((Pc0 - A1) @ d1) * d1
    return A1, d1


def evaluate(cams, member_cam, seg, A, d, hub):
    r, dropped = residuals(cams, member_cam, seg, A, d)
    J = jacobian(cams, member_cam, seg, A, d)
    keep = ~dropped
    rr, JJ = r[keep].reshape(-1), J[keep].reshape(-1, 4)
    ar = np.abs(rr)
    with np.errstate(all="ignore"):
        lin = (ar > hub) & (hub != 0.0)
        w = np.where(lin, hub / np.where(ar > 0, ar, 1.0), 1.0)
        rho = np.where(lin, 2.0 * hub * ar - hub * hub, rr * rr)
    H = (JJ * w[:, None]).T @ JJ
    b = (JJ * w[:, None]).T @ rr
    return {"H": H, "b": b, "cost": float(rho.sum()), "sumsq": float((rr * rr).sum()), "count": int(len(rr)), "dropped": int(dropped.sum())}


def rms_of(S):
    return float(np.sqrt(S["sumsq"] / S["count"])) if S["count"] > 0 else 0.0


def solve(H, b, lam):
    a = H + lam * np.diag(np.diag(H))
    L = np.zeros((4, 4))
    for j in range(4):
        s = a[j, j] - L[j, :j] @ L[j, :j]
        if not (s > 0.0) or not np.isfinite(s):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 4):
            L[i, j] = (a[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(4)
    for i in range(4):
        y[i] = (-b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(4)
    for i in range(3, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def point_t(cam, x, y, X, A, d, by_ray):
    """(t, whether the ray formula was used, den / (q.q))"""
    _, _, Minv, C = cam
    with np.errstate(all="ignore"):
        q = Minv @ np.array([x, y, 1.0])
        w = C - A
        qq, dq = q @ q, d @ q
        den = qq - dq * dq
        if by_ray and den > PARALLEL * qq:
            return float((qq * (d @ w) - dq * (q @ w)) / den), True, float(den / qq)
        return float(d @ (X - A)), False, float(den / qq) if qq > 0 else float("nan")


def sweep(order, t, A, d, member_cam):
    """fit::sweep_line: a stretch exists while segments of at least three cameras are open"""
    open_m, cam_open, opened, start, out = set(), {}, False, None, []
    for p in order:
        m = p >> 1
        c = int(member_cam[m])
        if m not in open_m:
            open_m.add(m)
            cam_open[c] = cam_open.get(c, 0) + 1
        else:
            open_m.discard(m)
            cam_open[c] -= 1
        n_open = sum(1 for k in cam_open.values() if k > 0)
        P = A + t[p] * d
        if opened and n_open < 3:
            out.append(np.concatenate([start, P]))
            opened = False
        elif not opened and n_open >= 3:
            start, opened = P, True
    return np.array(out).reshape(-1, 6)


def refine_group(member_cam, seg, pts, cameras, max_iterations=20, huber_px=2.0):
    """one group -> dict (line, rms_before, rms_after, iterations, status, segs (k, 6), t (2n,), by_ray (2n,), den_rel (2n,), dropped_start, cost trace)"""
    member_cam = np.asarray(member_cam, np.int64)
    seg = np.asarray(seg, np.float32).astype(np.float64).reshape(-1, 4)
    pts = np.asarray(pts, np.float64).reshape(-1, 6)
    n = len(member_cam)
    nan = float("nan")
    if n == 0 or not (np.all(np.isfinite(pts)) and np.all(np.isfinite(seg))):
        return {"line": np.full(6, nan), "rms_before": nan, "rms_after": nan, "iterations": 0, "status": 2, "segs": np.zeros((0, 6)), "t": np.full(2 * n, nan),
                "by_ray": np.zeros(2 * n, bool), "den_rel": np.full(2 * n, nan), "dropped_start": 0, "costs": []}
    cams = [camera_parts(P) for P in np.asarray(cameras, np.float64).reshape(-1, 3, 4)]
    Pc0, d = line_of_points(pts.reshape(-1, 3))
    A = Pc0.copy()
    S = evaluate(cams, member_cam, seg, A, d, huber_px)
    rms0, costs = rms_of(S), [S["cost"]]
    status, it, dropped_start = 1, 0, S["dropped"]
    if n - S["dropped"] < 2:
        status = 2
    else:
        lam = LAMBDA0
        while it < max_iterations and S["cost"] != 0.0:
            delta = solve(S["H"], S["b"], lam)
            it += 1
            accepted = small = False
            if delta is not None:
                A1, d1 = apply(A, d, delta, Pc0)
                T = evaluate(cams, member_cam, seg, A1, d1, huber_px)
                if T["cost"] < S["cost"]:
                    accepted, small = True, S["cost"] - T["cost"] <= DEC_REL * S["cost"]
                    A, d, S = A1, d1, T
                    costs.append(S["cost"])
            if accepted:
                status, lam = 0, max(lam / 10.0, LAMBDA_MIN)
                if small:
                    break
            else:
                lam = min(10.0 * lam, LAMBDA_MAX)
                if lam >= LAMBDA_MAX:
                    break
    d = sign_rule(d)
    t, by_ray, den_rel = np.zeros(2 * n), np.zeros(2 * n, bool), np.zeros(2 * n)
    for i in range(2 * n):
        m, j = i >> 1, i & 1
        t[i], by_ray[i], den_rel[i] = point_t(cams[member_cam[m]], seg[m, 2 * j], seg[m, 2 * j + 1], pts[m, 3 * j:3 * j + 3], A, d, status != 2)
    key = np.where(np.isnan(t), np.inf, t)
    order = sorted(range(2 * n), key=lambda i: (key[i], i))
    return {"line": np.concatenate([A, d]), "rms_before": rms0, "rms_after": rms_of(S), "iterations": it, "status": status, "segs": sweep(order, t, A, d, member_cam),
            "t": t, "by_ray": by_ray, "den_rel": den_rel, "dropped_start": dropped_start, "costs": costs}


def refine(group_start, member_cam, member_seg, member_pts, cameras, max_iterations=20, huber_px=2.0):
    """all groups -> list of refine_group results"""
    gs = np.asarray(group_start)
    seg, pts = np.asarray(member_seg).reshape(-1, 4), np.asarray(member_pts).reshape(-1, 6)
    return [refine_group(member_cam[gs[g]:gs[g + 1]], seg[gs[g]:gs[g + 1]], pts[gs[g]:gs[g + 1]], cameras, max_iterations, huber_px) for g in range(len(gs) - 1)]
