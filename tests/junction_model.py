"""The rules of include/line3d_amd.h ("JUNCTIONS OF 3-D LINES") in numpy float64 scalars: a line of the table, the pair test with its closest points,
where on a line a junction lies, the kinds, the records, the vertices with their star rule, the attachments and the counts, and the tolerance and
extension of a line on the pipeline object.  Every product, sum, quotient and root is one numpy operation, so each is rounded on its own; dot products
are ((x x) + (y y)) + (z z).  Shares no code with the product."""
import numpy as np

F = np.float64
END_P, END_Q, INTERIOR = 0, 1, 2
KIND_L, KIND_T, KIND_X = 0, 1, 2

RECORD = np.dtype([("i", np.int32), ("j", np.int32), ("where_i", np.int32), ("where_j", np.int32), ("s", np.float64), ("t", np.float64),
                   ("gap", np.float64), ("X", np.float64, (3,))])
VERTEX = np.dtype([("X", np.float64, (3,)), ("first_node", np.int32), ("degree", np.int32)])


def dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def prepare(line, tol, ext):
    """dict(P, d, L, tol, ext) of an eligible line, or None"""
    with np.errstate(all="ignore"):
        P = [F(v) for v in line[:3]]
        Q = [F(v) for v in line[3:6]]
        v = [Q[k] - P[k] for k in range(3)]
        L = np.sqrt(dot(v, v))
        if not (all(np.isfinite(x) for x in P + Q) and np.isfinite(F(tol)) and np.isfinite(F(ext)) and np.isfinite(L) and L > 0):
            return None
        return dict(P=P, d=[v[k] / L for k in range(3)], L=L, tol=F(tol), ext=F(ext))


def where_on(s, L, ext):
    if s + s <= L:
        return END_P if s <= ext else INTERIOR
    return END_Q if L - s <= ext else INTERIOR


def pair_terms(li, lj):
    """every number of the pair test of eligible lines i < j, whatever it decides: dict(b, den, s, t, g, X, Ci, Cj)"""
    with np.errstate(all="ignore"):
        b = dot(li["d"], lj["d"])
        w = [li["P"][k] - lj["P"][k] for k in range(3)]
        p, q = dot(li["d"], w), dot(lj["d"], w)
        den = F(1.0) - (b * b)
        s = ((b * q) - p) / den
        t = (q - (b * p)) / den
        Ci = [li["P"][k] + (s * li["d"][k]) for k in range(3)]
        Cj = [lj["P"][k] + (t * lj["d"][k]) for k in range(3)]
        r = [Ci[k] - Cj[k] for k in range(3)]
        g = np.sqrt(dot(r, r))
        X = [(Ci[k] + Cj[k]) * F(0.5) for k in range(3)]
        return dict(b=b, den=den, s=s, t=t, g=g, X=X, Ci=Ci, Cj=Cj)


def pair_eval(li, lj, cos_max):
    """None, or dict(s, t, g, X, wi, wj, kind) of the pair that passes"""
    m = pair_terms(li, lj)
    if not abs(m["b"]) <= F(cos_max):
        return None
    if not m["den"] > 0:
        return None
    s, t = m["s"], m["t"]
    if not (-li["ext"] <= s and s <= li["L"] + li["ext"]):
        return None
    if not (-lj["ext"] <= t and t <= lj["L"] + lj["ext"]):
        return None
    tol = lj["tol"] if li["tol"] < lj["tol"] else li["tol"]
    if not m["g"] <= tol:
        return None
    wi, wj = where_on(s, li["L"], li["ext"]), where_on(t, lj["L"], lj["ext"])
    ends = (wi != INTERIOR) + (wj != INTERIOR)
    return dict(s=s, t=t, g=m["g"], X=m["X"], wi=wi, wj=wj, kind=(KIND_X, KIND_T, KIND_L)[ends])


def spoke(tab, node, rep, cos_max):
    """the star rule for a node that is not the representative: the pair's values, or None"""
    a, r = node >> 1, rep >> 1
    if a == r:
        return None
    lo = a < r
    e = pair_eval(tab[a if lo else r], tab[r if lo else a], cos_max)
    if e is None:
        return None
    wa, wr = (e["wi"], e["wj"]) if lo else (e["wj"], e["wi"])
    return e if (wa == (node & 1) and wr == (rep & 1)) else None


def junctions(lines, tol, ext, cos_max, crossings=0):
    """-> dict(records, node_vertex (2 n,), vertices, node_attach (2 n,), counts (8,), comp, rep, stay: per node)"""
    lines = np.asarray(lines, F).reshape(-1, 6)
    n = len(lines)
    nn = 2 * n
    tab = [prepare(lines[i], tol[i], ext[i]) for i in range(n)]
    # condition 1 over all pairs at once narrows the candidates (the same products and sums, elementwise); the scalar test decides
    D = np.array([t["d"] if t else [np.nan] * 3 for t in tab], F).reshape(n, 3)
    rec = []
    parent = list(range(nn))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(n):
        if tab[i] is None:
            continue
        with np.errstate(all="ignore"):
            c = np.abs(((D[i, 0] * D[i + 1:, 0]) + (D[i, 1] * D[i + 1:, 1])) + (D[i, 2] * D[i + 1:, 2]))
        for j in (np.nonzero(c <= F(cos_max))[0] + i + 1).tolist():
            if tab[j] is None:
                continue
            e = pair_eval(tab[i], tab[j], cos_max)
            if e is None or (e["kind"] == KIND_X and not crossings):
                continue
            rec.append((i, j, e["wi"], e["wj"], e["s"], e["t"], e["g"], e["X"]))
            if e["kind"] == KIND_L:
                a, b = find(2 * i + e["wi"]), find(2 * j + e["wj"])
                if a != b:
                    parent[max(a, b)] = min(a, b)
    records = np.array(rec, RECORD) if rec else np.zeros(0, RECORD)
    comp = [find(v) for v in range(nn)]
    members = {}
    for v in range(nn):
        if tab[v >> 1] is not None:
            members.setdefault(comp[v], []).append(v)
    rep = [-1] * nn
    stay = [0] * nn
    node_vertex = [-1] * nn
    counts = [sum(t is not None for t in tab)] + [int((kinds_of(records) == k).sum()) for k in (KIND_L, KIND_T, KIND_X)] + [0, 0, 0, 0]
    found = []                                        # (lowest staying node, position, degree, staying nodes)
    for c, mem in members.items():
        r = mem[0]
        for v in mem[1:]:
            if tab[v >> 1]["L"] > tab[r >> 1]["L"]:
                r = v
        spokes = {v: spoke(tab, v, r, cos_max) for v in mem if v != r}
        stays = [v for v in mem if v == r or spokes[v] is not None]
        for v in mem:
            rep[v] = r
        for v in stays:
            stay[v] = 1
        if len(mem) >= 2:
            counts[4] += 1
            counts[6] += len(mem) - len(stays)
        if len(stays) >= 2:
            S = [F(0.0), F(0.0), F(0.0)]
            for v in stays:
                if v != r:
                    S = [S[k] + spokes[v]["X"][k] for k in range(3)]
            m = F(len(stays) - 1)
            found.append((stays[0], [S[k] / m for k in range(3)], len(stays), stays))
    found.sort(key=lambda f: f[0])
    vertices = np.zeros(len(found), VERTEX)
    for k, (first, X, degree, stays) in enumerate(found):
        vertices[k] = (X, first, degree)
        for v in stays:
            node_vertex[v] = k
    counts[5] = len(found)
    node_attach = [-1] * nn
    for k in range(len(records)):
        wi, wj = int(records["where_i"][k]), int(records["where_j"][k])
        if (wi != INTERIOR) + (wj != INTERIOR) != 1:
            continue
        v = 2 * int(records["i"][k]) + wi if wi != INTERIOR else 2 * int(records["j"][k]) + wj
        if node_vertex[v] >= 0:
            continue
        if node_attach[v] < 0 or records["gap"][k] < records["gap"][node_attach[v]]:
            node_attach[v] = k
    counts[7] = sum(a >= 0 for a in node_attach)
    return dict(records=records, node_vertex=np.array(node_vertex, np.int32), vertices=vertices, node_attach=np.array(node_attach, np.int32),
                counts=np.array(counts, np.int32), comp=np.array(comp, np.int32), rep=np.array(rep, np.int32), stay=np.array(stay, np.int32))


def kinds_of(records):
    ends = (records["where_i"] != INTERIOR).astype(np.int32) + (records["where_j"] != INTERIOR).astype(np.int32)
    return np.array([KIND_X, KIND_T, KIND_L], np.int32)[ends]


def line_sigma(P, Q, members, views):
    """sigma of a line on the pipeline object, as step 1 of the merging defines it: the mean over the members, in their stored order, of z / f -- z = R[2] .
    M + t[2] at M = (P + Q) / 2, f = (|K00| + |K11|) / 2 of the member's view.  Members with z <= 0 or a term that is not finite are skipped; none left:
    0.  members: (camera, segment); views: id -> dict(K, R, t)"""
    M = [(F(P[k]) + F(Q[k])) / F(2.0) for k in range(3)]
    total, cnt = F(0.0), 0
    with np.errstate(all="ignore"):
        for cam, _ in members:
            v = views[int(cam)]
            K, R, t = np.asarray(v["K"], F).reshape(3, 3), np.asarray(v["R"], F).reshape(3, 3), np.asarray(v["t"], F).reshape(3)
            z = dot(R[2], M) + t[2]
            f = (abs(K[0, 0]) + abs(K[1, 1])) / F(2.0)
            q = z / f
            if not (z > 0 and np.isfinite(q)):
                continue
            total = total + q
            cnt += 1
    return total / F(cnt) if cnt else F(0.0)


def line_tol_ext(P, Q, members, views, dist_px=4.0, ext_px=12.0, max_ext_rel=0.25):
    """(tol, ext) of a line on the pipeline object: tol = dist_px x sigma, ext = min(ext_px x sigma, max_ext_rel x L)"""
    with np.errstate(all="ignore"):
        sigma = line_sigma(P, Q, members, views)
        v = [F(Q[k]) - F(P[k]) for k in range(3)]
        L = np.sqrt(dot(v, v))
        a, b = F(ext_px) * sigma, F(max_ext_rel) * L
        tol, ext = F(dist_px) * sigma, (b if b < a else a)
    return (tol if tol >= 0 else F(0.0)), (ext if ext >= 0 else F(0.0))


def result_table(result, views, dist_px=4.0, ext_px=12.0, max_ext_rel=0.25):
    """a result list [(members [(cam, seg)...], segs3d (k, 6))...] -> lines (n, 6): the start of the first 3-D segment and the end of the last, tol, ext"""
    n = len(result)
    lines = np.array([list(np.asarray(s, F).reshape(-1, 6)[0, :3]) + list(np.asarray(s, F).reshape(-1, 6)[-1, 3:]) for _, s in result], F).reshape(n, 6)
    te = [line_tol_ext(lines[k, :3], lines[k, 3:], result[k][0], views, dist_px, ext_px, max_ext_rel) for k in range(n)]
    return lines, np.array([t for t, _ in te], F).reshape(n), np.array([e for _, e in te], F).reshape(n)


def snap_result(result, lines, out):
    """the ends moved as l3d_line3d_set_junctions(snap) moves them -> (the new result list, ends moved, moves skipped)"""
    moved = skipped = 0
    new = [(m, np.array(s, F).reshape(-1, 6).copy()) for m, s in result]
    for l in range(len(result)):
        P = [F(x) for x in lines[l, :3]]
        v = [F(lines[l, 3 + k]) - P[k] for k in range(3)]
        L = np.sqrt(dot(v, v))
        d = [v[k] / L for k in range(3)]
        for e in (0, 1):
            node = 2 * l + e
            if out["node_vertex"][node] >= 0:
                X = out["vertices"]["X"][out["node_vertex"][node]]
                s = dot([X[k] - P[k] for k in range(3)], d)
            elif out["node_attach"][node] >= 0:
                r = out["records"][out["node_attach"][node]]
                s = r["s"] if r["i"] == l else r["t"]
            else:
                continue
            to = [P[k] + (s * d[k]) for k in range(3)]
            seg = new[l][1][0] if e == 0 else new[l][1][-1]
            far, old = (seg[3:6], seg[0:3]) if e == 0 else (seg[0:3], seg[3:6])
            if not dot([far[k] - to[k] for k in range(3)], [far[k] - old[k] for k in range(3)]) > 0:
                skipped += 1
                continue
            seg[0 + 3 * e:3 + 3 * e] = to
            moved += 1
    return new, moved, skipped


def corner_recall(scene, result, views, lines, tol, ext, node_vertex):
    """Recall of the true corners of a make_scene_boxes scene.  A corner is COVERED when at least two reconstructed lines that show edges of that corner
    (majority ground truth of their members) have an end within their tol + ext of it; it is RECALLED when one vertex holds such ends of at least two of
    these lines -> (covered corners, recalled corners, the box of every line)"""
    edge_of = [int(np.bincount([int(views[c]["gt"][s]) for c, s in m]).argmax()) for m, _ in result]
    covered, recalled = [], []
    for c, X in enumerate(scene.corners):
        ends = []                                    # nodes of lines of this corner's edges that reach it
        for l, e in enumerate(edge_of):
            if e not in scene.corner_edges[c]:
                continue
            for end in (0, 1):
                if np.linalg.norm(lines[l, 3 * end:3 * end + 3] - X) <= tol[l] + ext[l]:
                    ends.append(2 * l + end)
        if len({v >> 1 for v in ends}) < 2:
            continue
        covered.append(c)
        vs = [node_vertex[v] for v in ends if node_vertex[v] >= 0]
        if vs and max(np.bincount(vs)) >= 2:
            recalled.append(c)
    return covered, recalled, np.array([e // 12 for e in edge_of], np.int32)
