"""The rules of include/line3d_amd.h, "SUPPORT OF 3-D LINES", in numpy float64 scalars: a row (one 3-D segment in one camera: the projection's pair
through the rectangle rule, its ends kept in f64), a column (one 2-D segment), the pair test, the records in (camera, k, j) order, the best row of
every column and the four counts; and gather(), the same on the lines of a result ("ON THE OBJECT").  Every product, sum, quotient and square root is one numpy operation, so each is rounded on its own; no BLAS call.
The camera frame, the rectangle and the rectangle rule are the projection model's (tests/project_model.py).  Shares no code with the product."""
import numpy as np

import project_model as pm

F = np.float64
RECORD = np.dtype([("seg3d", np.int32), ("seg2d", np.int32), ("dist", np.float32), ("overlap", np.float32)])


def mx(a, b):
    return b if a < b else a


def mn(a, b):
    return b if b < a else a


def row(cam, seg, near, margin):
    """one (camera, 3-D segment) -> None (no row) or dict(A, B, da, La) in f64; cam = (K, R, t, width, height)"""
    K, R, t, width, height = cam
    K = np.asarray(K, F).reshape(9)
    near = F(near)
    seg = np.asarray(seg, F)
    with np.errstate(all="ignore"):
        P, Q = pm.camera_frame(R, t, seg[:3]), pm.camera_frame(R, t, seg[3:])
        if not all(np.isfinite(v) for v in P + Q):
            return None
        if P[2] < near and Q[2] < near:
            return None
        if P[2] < near:
            s = (near - P[2]) / (Q[2] - P[2])
            P = [P[0] + s * (Q[0] - P[0]), P[1] + s * (Q[1] - P[1]), near]
        elif Q[2] < near:
            s = (near - Q[2]) / (P[2] - Q[2])
            Q = [Q[0] + s * (P[0] - Q[0]), Q[1] + s * (P[1] - Q[1]), near]

        def pix(p):
            xn, yn = p[0] / p[2], p[1] / p[2]
            return (K[0] * xn + K[1] * yn) + K[2], (K[3] * xn + K[4] * yn) + K[5]

        (uP, vP), (uQ, vQ) = pix(P), pix(Q)
        du, dv = uQ - uP, vQ - vP
        if not all(np.isfinite(v) for v in (uP, vP, uQ, vQ, du, dv)):
            return None
        if du == 0 and dv == 0:
            return None
        tt = pm.clip(uP, vP, du, dv, pm.rect(width, height, margin))
        if tt is None:
            return None
        t0, t1 = tt
        A = (uP, vP) if t0 == 0 else (uP + t0 * du, vP + t0 * dv)
        B = (uQ, vQ) if t1 == 1 else (uP + t1 * du, vP + t1 * dv)
        ax, ay = B[0] - A[0], B[1] - A[1]
        La = np.sqrt((ax * ax) + (ay * ay))
        if not (np.isfinite(La) and La > 0):
            return None
        return dict(A=A, B=B, da=(ax / La, ay / La), La=La, t=(t0, t1))


def column(g):
    """x1, y1, x2, y2 (float32) -> None (not eligible) or dict(U, V, db, Lb)"""
    g = np.asarray(g, np.float32).astype(F)
    with np.errstate(all="ignore"):
        U, V = (g[0], g[1]), (g[2], g[3])
        bx, by = V[0] - U[0], V[1] - U[1]
        Lb = np.sqrt((bx * bx) + (by * by))
        if not (all(np.isfinite(v) for v in g) and np.isfinite(Lb) and Lb > 0):
            return None
        return dict(U=U, V=V, db=(bx / Lb, by / Lb), Lb=Lb)


def pair_terms(r, c):
    """|cos|, eU, eV, ov, min(La, Lb) of a row and an eligible column"""
    with np.errstate(all="ignore"):
        A, (dax, day) = r["A"], r["da"]
        cs = abs((dax * c["db"][0]) + (day * c["db"][1]))
        e, s = [], []
        for X in (c["U"], c["V"]):
            wx, wy = X[0] - A[0], X[1] - A[1]
            e.append(abs((wx * day) - (wy * dax)))
            s.append((wx * dax) + (wy * day))
        ov = mn(mx(s[0], s[1]), r["La"]) - mx(mn(s[0], s[1]), F(0.0))
        return cs, e[0], e[1], ov, mn(r["La"], c["Lb"])


def pair_test(r, c, dist_px, cos_min, min_overlap):
    """-> None, or (dist, overlap) as float32"""
    with np.errstate(all="ignore"):
        cs, eU, eV, ov, Lm = pair_terms(r, c)
        if not cs >= F(cos_min):
            return None
        if not (eU <= F(dist_px) and eV <= F(dist_px)):
            return None
        if not ov >= F(min_overlap) * Lm:
            return None
        return np.float32(mx(eU, eV)), np.float32(ov / Lm)


def columns(segs):
    """the column table of one camera as arrays over j: (ok, Ux, Uy, Vx, Vy, dbx, dby, Lb); the same operations as column(), one numpy operation each"""
    g = np.asarray(segs, np.float32).reshape(-1, 4).astype(F)
    with np.errstate(all="ignore"):
        Ux, Uy, Vx, Vy = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
        bx, by = Vx - Ux, Vy - Uy
        Lb = np.sqrt((bx * bx) + (by * by))
        ok = np.isfinite(Ux) & np.isfinite(Uy) & np.isfinite(Vx) & np.isfinite(Vy) & np.isfinite(Lb) & (Lb > 0)
        return ok, Ux, Uy, Vx, Vy, bx / Lb, by / Lb, Lb


def row_against_columns(r, cols, dist_px, cos_min, min_overlap):
    """the pair test of one row against all columns of its camera -> (pass mask, dist float32, overlap float32) over j"""
    ok, Ux, Uy, Vx, Vy, dbx, dby, Lb = cols
    A, (dax, day), La = r["A"], r["da"], r["La"]
    amx = lambda a, b: np.where(a < b, b, a)
    amn = lambda a, b: np.where(b < a, b, a)
    with np.errstate(all="ignore"):
        cs = np.abs((dax * dbx) + (day * dby))
        wUx, wUy, wVx, wVy = Ux - A[0], Uy - A[1], Vx - A[0], Vy - A[1]
        eU, eV = np.abs((wUx * day) - (wUy * dax)), np.abs((wVx * day) - (wVy * dax))
        sU, sV = (wUx * dax) + (wUy * day), (wVx * dax) + (wVy * day)
        ov = amn(amx(sU, sV), La) - amx(amn(sU, sV), F(0.0))
        Lm = amn(La, Lb)
        good = ok & (cs >= F(cos_min)) & (eU <= F(dist_px)) & (eV <= F(dist_px)) & (ov >= F(min_overlap) * Lm)
        return good, amx(eU, eV).astype(np.float32), (ov / Lm).astype(np.float32)


def support(seg3d, cams, segments_per_camera, dist_px, cos_min, min_overlap, near, margin):
    """-> dict(records, cam_start (m + 1,) int64, best (all 2-D segments,) int32, counts (4,) int64)"""
    seg3d = np.asarray(seg3d, F).reshape(-1, 6)
    per = [np.asarray(s, np.float32).reshape(-1, 4) for s in segments_per_camera]
    assert len(per) == len(cams)
    T = sum(len(s) for s in per)
    best = np.full(T, -1, np.int32)
    counts = np.zeros(4, np.int64)
    if len(seg3d) == 0 or len(cams) == 0:
        return dict(records=np.zeros(0, RECORD), cam_start=np.zeros(len(cams) + 1, np.int64), best=best, counts=counts)
    parts, start, off, total = [], [0], 0, 0
    for cam, segs in zip(cams, per):
        cols = columns(segs)
        counts[1] += int(cols[0].sum())
        bd = np.full(len(segs), np.inf, F)              # the smallest dist (as float32) so far; ascending k: the first k that reaches it stays
        for k, s in enumerate(seg3d):
            r = row(cam, s, near, margin)
            if r is None:
                continue
            counts[0] += 1
            if len(segs) == 0:
                continue
            good, dist, ov = row_against_columns(r, cols, dist_px, cos_min, min_overlap)
            j = np.nonzero(good)[0]
            if len(j) == 0:
                continue
            rec = np.zeros(len(j), RECORD)
            rec["seg3d"], rec["seg2d"], rec["dist"], rec["overlap"] = k, j, dist[j], ov[j]
            parts.append(rec)
            total += len(j)
            better = (best[off + j] < 0) | (dist[j].astype(F) < bd[j])
            bd[j[better]] = dist[j][better].astype(F)
            best[off + j[better]] = k
        off += len(segs)
        start.append(total)
    counts[2] = total
    counts[3] = int((best >= 0).sum())
    return dict(records=np.concatenate(parts) if parts else np.zeros(0, RECORD), cam_start=np.array(start, np.int64), best=best, counts=counts)


LINE_RECORD = np.dtype([("view_id", np.uint32), ("seg", np.uint32), ("seg3d", np.int32), ("dist", np.float32), ("overlap", np.float32), ("flags", np.uint32)])


def gather(lines, views, dist_px, cos_min, min_overlap, near, margin):
    """"ON THE OBJECT": lines = [(members [(view id, segment)], 3-D segments (k, 6))] in the result's order, views = {id: (camera, segments)} ->
    dict(records (LINE_RECORD, ordered by (line, view id, segment)), line_start, line_views (lines, 2), counts (4,) int64, added: per line the
    (view id, segment) pairs a finish with the support on appends)"""
    ids = sorted(views)
    seg3d = np.array([s for _, s3 in lines for s in np.asarray(s3, F).reshape(-1, 6)], F).reshape(-1, 6)
    line_of = [li for li, (_, s3) in enumerate(lines) for _ in range(len(np.asarray(s3, F).reshape(-1, 6)))]
    out = support(seg3d, [views[i][0] for i in ids], [views[i][1] for i in ids], dist_px, cos_min, min_overlap, near, margin)
    seg_off = np.concatenate([[0], np.cumsum([len(views[i][1]) for i in ids])])
    member = {}
    for li, (m, _) in enumerate(lines):
        for key in m:
            member.setdefault((int(key[0]), int(key[1])), set()).add(li)
    entry = {}                                              # (line, view id, segment) -> (dist, seg3d, overlap): the smallest (dist, seg3d)
    for c, vid in enumerate(ids):
        for r in out["records"][out["cam_start"][c]:out["cam_start"][c + 1]]:
            key = (line_of[int(r["seg3d"])], vid, int(r["seg2d"]))
            val = (float(r["dist"]), int(r["seg3d"]), r["overlap"], r["dist"])
            if key not in entry or val[:2] < entry[key][:2]:
                entry[key] = val
    recs, start, views_of, added = [], [0], [], [[] for _ in lines]
    found = 0
    on_a_line = set()
    for li, (m, _) in enumerate(lines):
        mine = sorted(k for k in entry if k[0] == li)
        for _, vid, j in mine:
            d, k3, ov, d32 = entry[(li, vid, j)]
            where = member.get((vid, j), set())
            b = out["best"][seg_off[ids.index(vid)] + j]
            flags = (1 if li in where else 0) | (2 if where - {li} else 0) | (4 if b >= 0 and line_of[b] == li else 0)
            recs.append((vid, j, k3, d32, ov, flags))
            found += flags & 1
            on_a_line.add((vid, j))
            if flags == 4:
                added[li].append((vid, j))
        start.append(len(recs))
        views_of.append((len({int(c) for c, _ in m}), len({vid for _, vid, _ in mine})))
    n_members = sum(len(m) for m, _ in lines)
    counts = np.array([len(recs), found, n_members - found, sum(1 for k in on_a_line if k not in member)], np.int64)
    return dict(records=np.array(recs, LINE_RECORD) if recs else np.zeros(0, LINE_RECORD), line_start=np.array(start, np.int64),
                line_views=np.array(views_of, np.int32).reshape(-1, 2), counts=counts, added=added)
