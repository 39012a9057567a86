"""The rules of include/line3d_amd.h ("PLANES OF 3-D LINES") in numpy float64: a line of the table, a hypothesis from a seed pair, the lies-in test, the
hypothesis pair test, the components with their star rule, the parameters of a candidate, its frame, members and extent, the counts, and the tolerance
of a line on the pipeline object.  Every product, sum, quotient and root is one numpy operation, so each is rounded on its own; dot products are
((x x) + (y y)) + (z z).  The all-pairs search and the membership run one row against arrays -- the same operations elementwise -- so that tables of
thousands of seeds stay quick; the scalar functions state the rule and the tests compare the two.  Shares no code with the product."""
import numpy as np

F = np.float64
SEED = 1

PLANE = np.dtype([("N", np.float64, (3,)), ("c", np.float64), ("u", np.float64, (3,)), ("v", np.float64, (3,)), ("rect", np.float64, (4,)), ("rep", np.int32),
                  ("first_hyp", np.int32), ("n_hyp", np.int32), ("n_lines", np.int32)])
MEMBER = np.dtype([("plane", np.int32), ("line", np.int32), ("flags", np.int32), ("pad", np.int32)])


def dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def cross(a, b):
    return [(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])]


def prepare(line, tol):
    """dict(P, Q, d, L, tol) of an eligible line, or None"""
    with np.errstate(all="ignore"):
        P = [F(v) for v in line[:3]]
        Q = [F(v) for v in line[3:6]]
        v = [Q[k] - P[k] for k in range(3)]
        L = np.sqrt(dot(v, v))
        if not (all(np.isfinite(x) for x in P + Q) and np.isfinite(F(tol)) and np.isfinite(L) and L > 0):
            return None
        return dict(P=P, Q=Q, d=[v[k] / L for k in range(3)], L=L, tol=F(tol))


def hypothesis_terms(li, lj):
    """every number of the hypothesis of two eligible lines, whatever is decided: dict(b, den, mm, N, X, c, A)"""
    with np.errstate(all="ignore"):
        b = dot(li["d"], lj["d"])
        den = F(1.0) - (b * b)
        cr = cross(li["d"], lj["d"])
        mm = np.sqrt(dot(cr, cr))
        w = [li["P"][k] - lj["P"][k] for k in range(3)]
        p, q = dot(li["d"], w), dot(lj["d"], w)
        s = ((b * q) - p) / den
        t = (q - (b * p)) / den
        Ci = [li["P"][k] + (s * li["d"][k]) for k in range(3)]
        Cj = [lj["P"][k] + (t * lj["d"][k]) for k in range(3)]
        X = [(Ci[k] + Cj[k]) * F(0.5) for k in range(3)]
        N = [cr[k] / mm for k in range(3)]
        return dict(b=b, den=den, mm=mm, N=N, X=X, c=dot(N, X), A=(li["L"] * lj["L"]) * mm)


def hypothesis(tab, i, j, cos_max):
    """dict(N, c, X, A, i, j) of the eligible hypothesis of seed (i, j), or None"""
    if i == j or tab[i] is None or tab[j] is None:
        return None
    t = hypothesis_terms(tab[i], tab[j])
    if not abs(t["b"]) <= F(cos_max):
        return None
    if not t["den"] > 0:
        return None
    if not t["mm"] > 0:
        return None
    return dict(N=t["N"], c=t["c"], X=t["X"], A=t["A"], i=int(i), j=int(j))


def plane_distance(P, N, c):
    """|(N . P) - c|"""
    with np.errstate(all="ignore"):
        return abs(dot(N, P) - c)


def lies_in(line, N, c):
    return bool(plane_distance(line["P"], N, c) <= line["tol"] and plane_distance(line["Q"], N, c) <= line["tol"])


def pair_test(tab, h, g, cos_min):
    """the hypothesis pair test of two eligible hypotheses (dicts)"""
    with np.errstate(all="ignore"):
        if not abs(dot(h["N"], g["N"])) >= F(cos_min):
            return False
    if not (lies_in(tab[g["i"]], h["N"], h["c"]) and lies_in(tab[g["j"]], h["N"], h["c"])):
        return False
    return lies_in(tab[h["i"]], g["N"], g["c"]) and lies_in(tab[h["j"]], g["N"], g["c"])


def parameters(tab, hyp, stays, rep):
    """dict(N, c, u, v, ok, ns, W, lu) of the candidate whose staying hypotheses are `stays` (ascending)"""
    with np.errstate(all="ignore"):
        S = [F(0.0)] * 3
        W = F(0.0)
        for h in stays:
            sg = F(-1.0) if dot(hyp[h]["N"], hyp[rep]["N"]) < 0 else F(1.0)
            a = hyp[h]["A"] * sg
            S = [S[k] + (a * hyp[h]["N"][k]) for k in range(3)]
            W = W + hyp[h]["A"]
        ns = np.sqrt(dot(S, S))
        N = [S[k] / ns for k in range(3)]
        T = F(0.0)
        for h in stays:
            T = T + (hyp[h]["A"] * dot(N, hyp[h]["X"]))
        c = T / W
        d = tab[hyp[rep]["i"]]["d"]
        dn = dot(d, N)
        up = [d[k] - (dn * N[k]) for k in range(3)]
        lu = np.sqrt(dot(up, up))
        u = [up[k] / lu for k in range(3)]
        v = cross(N, u)
        ok = bool(np.isfinite(ns) and ns > 0 and np.isfinite(W) and W > 0 and np.isfinite(lu) and lu > 0)
        return dict(N=N, c=c, u=u, v=v, ok=ok, ns=ns, W=W, lu=lu)


def frame_coordinates(p, X):
    """(a, b) of the point X in the frame of the plane p"""
    with np.errstate(all="ignore"):
        r = [X[k] - (p["c"] * p["N"][k]) for k in range(3)]
        return dot(p["u"], r), dot(p["v"], r)


def planes(lines, tol, seeds, cos_max, cos_min, min_lines):
    """-> dict(planes, members, hyp_plane (m,), counts (8,), comp, rep, stay: per hypothesis, hyp: the hypotheses or None, tab, cand: the candidates'
    parameters in their order with their member counts)"""
    lines = np.asarray(lines, F).reshape(-1, 6)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    n, m = len(lines), len(seeds)
    counts = [0] * 8
    if n == 0 or m == 0:
        return dict(planes=np.zeros(0, PLANE), members=np.zeros(0, MEMBER), hyp_plane=np.full(m, -1, np.int32), counts=np.array(counts, np.int32), comp=list(range(m)),
                    rep=[-1] * m, stay=[0] * m, hyp=[None] * m, tab=[None] * n, cand=[])
    tab = [prepare(lines[i], tol[i]) for i in range(n)]
    hyp = [hypothesis(tab, int(i), int(j), cos_max) for i, j in seeds]
    counts[0] = sum(t is not None for t in tab)
    counts[1] = sum(h is not None for h in hyp)
    elig = np.array([h is not None for h in hyp])
    HN = np.array([h["N"] if h else [np.nan] * 3 for h in hyp], F).reshape(m, 3)
    Hc = np.array([h["c"] if h else np.nan for h in hyp], F)
    E = np.zeros((m, 4, 3), F)
    T = np.zeros((m, 4), F)
    for k, h in enumerate(hyp):
        if h:
            li, lj = tab[h["i"]], tab[h["j"]]
            E[k] = [li["P"], li["Q"], lj["P"], lj["Q"]]
            T[k] = [li["tol"], li["tol"], lj["tol"], lj["tol"]]
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def row_test(h, cols):
        """the pair test of hypothesis h against the hypotheses `cols` (an index array), elementwise"""
        with np.errstate(all="ignore"):
            ok = elig[cols] & (np.abs(((HN[h, 0] * HN[cols, 0]) + (HN[h, 1] * HN[cols, 1])) + (HN[h, 2] * HN[cols, 2])) >= F(cos_min))
            for k in range(4):
                ok &= np.abs((((HN[h, 0] * E[cols, k, 0]) + (HN[h, 1] * E[cols, k, 1])) + (HN[h, 2] * E[cols, k, 2])) - Hc[h]) <= T[cols, k]
                ok &= np.abs((((HN[cols, 0] * E[h, k, 0]) + (HN[cols, 1] * E[h, k, 1])) + (HN[cols, 2] * E[h, k, 2])) - Hc[cols]) <= T[h, k]
        return ok

    for h in range(m):
        if hyp[h] is None or h + 1 == m:
            continue
        cols = np.arange(h + 1, m)
        for g in cols[row_test(h, cols)].tolist():
            counts[2] += 1
            a, b = find(h), find(g)
            if a != b:
                parent[max(a, b)] = min(a, b)
    comp = [find(h) for h in range(m)]
    groups = {}
    for h in range(m):
        if hyp[h] is not None:
            groups.setdefault(comp[h], []).append(h)
    rep, stay = [-1] * m, [0] * m
    cands = []                                        # (lowest staying hypothesis, staying hypotheses, representative)
    for c, mem in groups.items():
        r = mem[0]
        for h in mem[1:]:
            if hyp[h]["A"] > hyp[r]["A"]:
                r = h
        others = np.array([h for h in mem if h != r], np.int64)
        passes = set(others[row_test(r, others)].tolist()) if len(others) else set()
        stays = [h for h in mem if h == r or h in passes]
        for h in mem:
            rep[h] = r
        for h in stays:
            stay[h] = 1
        counts[4] += len(mem) - len(stays)
        cands.append((stays[0], stays, r))
    cands.sort()
    counts[3] = len(cands)
    ok_line = np.array([t is not None for t in tab])
    LP = np.array([t["P"] if t else [0.0] * 3 for t in tab], F).reshape(n, 3)
    LQ = np.array([t["Q"] if t else [0.0] * 3 for t in tab], F).reshape(n, 3)
    LT = np.array([t["tol"] if t else 0.0 for t in tab], F)
    out_planes, out_members, cand_info = [], [], []
    hyp_plane = np.full(m, -1, np.int32)
    for _, stays, r in cands:
        p = parameters(tab, hyp, stays, r)
        mem = []
        if p["ok"]:
            N, c = p["N"], p["c"]
            with np.errstate(all="ignore"):
                dp = np.abs((((N[0] * LP[:, 0]) + (N[1] * LP[:, 1])) + (N[2] * LP[:, 2])) - c)
                dq = np.abs((((N[0] * LQ[:, 0]) + (N[1] * LQ[:, 1])) + (N[2] * LQ[:, 2])) - c)
            mem = np.nonzero(ok_line & (dp <= LT) & (dq <= LT))[0].tolist()
        kept = p["ok"] and len(mem) >= min_lines
        cand_info.append(dict(p, stays=stays, rep=r, members=mem, kept=kept))
        if not kept:
            counts[5] += 1
            continue
        seed_lines = set()
        for h in stays:
            seed_lines.update((hyp[h]["i"], hyp[h]["j"]))
        rect = None
        for k in mem:
            for X in (tab[k]["P"], tab[k]["Q"]):
                a, b = frame_coordinates(p, X)
                if rect is None:
                    rect = [a, a, b, b]
                else:
                    rect = [a if a < rect[0] else rect[0], a if rect[1] < a else rect[1], b if b < rect[2] else rect[2], b if rect[3] < b else rect[3]]
            out_members.append((len(out_planes), k, SEED if k in seed_lines else 0, 0))
        for h in stays:
            hyp_plane[h] = len(out_planes)
        out_planes.append((p["N"], p["c"], p["u"], p["v"], rect, r, stays[0], len(stays), len(mem)))
    counts[6], counts[7] = len(out_planes), len(out_members)
    return dict(planes=np.array(out_planes, PLANE) if out_planes else np.zeros(0, PLANE), members=np.array(out_members, MEMBER) if out_members else np.zeros(0, MEMBER),
                hyp_plane=hyp_plane, counts=np.array(counts, np.int32), comp=comp, rep=rep, stay=stay, hyp=hyp, tab=tab, cand=cand_info)


def line_tolerance(dist_px, sigma):
    """tol of a line on the object: dist_px x the junctions' sigma; 0 where that is not a number >= 0"""
    with np.errstate(all="ignore"):
        t = F(dist_px) * F(sigma)
    return t if t >= 0 else F(0.0)


def box_faces(corner_edges):
    """the faces of a make_scene_boxes scene from its corner_edges (8 per box: corner 8 b + c has sign bit k of c on axis k): face 6 b + 2 k + s holds the
    corners of box b whose bit k is s -> list of (corner indices, the 4 edges that join two of them)"""
    faces = []
    for b in range(len(corner_edges) // 8):
        for k in range(3):
            for s in (0, 1):
                cs = [8 * b + c for c in range(8) if ((c >> k) & 1) == s]
                seen = np.concatenate([np.asarray(corner_edges[c]) for c in cs]).tolist()
                faces.append((cs, sorted(e for e in set(seen) if seen.count(e) == 2)))
    return faces


def face_recall(corners, corner_edges, edge_of, line_box, tol, out):
    """Recall of the true faces of a make_scene_boxes scene by the planes `out` (a result of planes(), of the host twin or of the device) over lines whose
    majority ground-truth edges are edge_of.  A face is COVERED when at least 3 of its 4 edges have a line; it is RECALLED when one plane has members on
    at least 3 of its edges (its plane: the one with members on the most edges, the lowest at a tie).  -> dict(covered, recalled: face indices,
    plane_of: per recalled face its plane, mixed: the planes whose SEED lines belong to more than one box, unmatched: the planes that recall no face,
    corner_ratio: the largest distance of a true corner of a recalled face from its plane, in units of that plane's largest member tolerance)"""
    planes_, mem = out["planes"], out["members"]
    edge_of = np.asarray(edge_of)
    lines_of = [mem["line"][mem["plane"] == k] for k in range(len(planes_))]
    have = set(edge_of.tolist())
    covered, recalled, plane_of, ratio = [], [], [], 0.0
    for f, (cs, edges) in enumerate(box_faces(corner_edges)):
        if sum(e in have for e in edges) < 3:
            continue
        covered.append(f)
        hits = [len(set(edge_of[ls].tolist()) & set(edges)) for ls in lines_of]
        if not hits or max(hits) < 3:
            continue
        k = int(np.argmax(hits))
        recalled.append(f)
        plane_of.append(k)
        p = planes_[k]
        worst = max(abs(float(np.dot(p["N"], corners[c])) - float(p["c"])) for c in cs)
        ratio = max(ratio, worst / float(np.max(np.asarray(tol)[lines_of[k]])))
    mixed = []
    for k in range(len(planes_)):
        seeds = mem["line"][(mem["plane"] == k) & ((mem["flags"] & SEED) != 0)]
        if len(set(np.asarray(line_box)[seeds].tolist())) > 1:
            mixed.append(k)
    return dict(covered=covered, recalled=recalled, plane_of=plane_of, mixed=mixed, unmatched=sorted(set(range(len(planes_))) - set(plane_of)), corner_ratio=ratio)
