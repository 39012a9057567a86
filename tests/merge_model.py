"""The rules of include/line3d_amd.h ("MERGING DUPLICATE LINES") in numpy float64 scalars: a line of the table, the pair test, the components, the
representative, the star rule, the tolerance of a line on the pipeline object and the round loop.  Every product, sum, quotient and root is one numpy
operation, so each is rounded on its own; dot products are ((x x) + (y y)) + (z z).  Shares no code with the product; the refit is passed in."""
import numpy as np

F = np.float64


def dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def prepare(line, tol):
    """(P, Q, d, L, tol) of an eligible line, or None"""
    with np.errstate(all="ignore"):
        P = [F(v) for v in line[:3]]
        Q = [F(v) for v in line[3:6]]
        v = [Q[k] - P[k] for k in range(3)]
        L = np.sqrt(dot(v, v))
        if not (all(np.isfinite(x) for x in P + Q) and np.isfinite(F(tol)) and np.isfinite(L) and L > 0):
            return None
        return P, Q, [v[k] / L for k in range(3)], L, F(tol)


def along_across(a, X):
    P, _, d, _, _ = a
    v = [X[k] - P[k] for k in range(3)]
    s = dot(v, d)
    r = [v[k] - s * d[k] for k in range(3)]
    return s, np.sqrt(dot(r, r))


def pair_terms(a, b):
    """|d_a . d_b|, e_P, e_Q, the overlap of conditions 1 to 3 (a: the longer line)"""
    with np.errstate(all="ignore"):
        sP, eP = along_across(a, b[0])
        sQ, eQ = along_across(a, b[1])
        hi = min(max(sP, sQ), a[3])
        lo = max(min(sP, sQ), F(0.0))
        return abs(dot(a[2], b[2])), eP, eQ, hi - lo


def pair_test(ti, tj, cos_min, max_gap):
    """eligible table entries of lines i < j"""
    a, b = (ti, tj) if ti[3] >= tj[3] else (tj, ti)
    c, eP, eQ, ov = pair_terms(a, b)
    if not c >= F(cos_min):
        return False
    tol = max(a[4], b[4])
    if not (eP <= tol and eQ <= tol):
        return False
    return bool(ov >= -(F(max_gap) * b[3]))


def group_lines(lines, tol, cos_min, max_gap):
    """-> dict(group (n,) int32, pairs (k, 2) int32, counts (4,) int32, comp, rep: per line its component's label and representative)"""
    lines = np.asarray(lines, F).reshape(-1, 6)
    n = len(lines)
    tab = [prepare(lines[i], tol[i]) for i in range(n)]
    # condition 1 over all pairs at once narrows the candidates (the same products and sums, elementwise); the scalar test decides
    D = np.array([t[2] if t else [np.nan] * 3 for t in tab], F).reshape(n, 3)
    pairs = []
    parent = list(range(n))

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
        for j in (np.nonzero(c >= F(cos_min))[0] + i + 1).tolist():
            if tab[j] is not None and pair_test(tab[i], tab[j], cos_min, max_gap):
                pairs.append((i, j))
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    comp = [find(i) for i in range(n)]
    members = {}
    for i in range(n):
        if tab[i] is not None:
            members.setdefault(comp[i], []).append(i)
    group = list(range(n))
    rep = [-1] * n
    counts = [sum(t is not None for t in tab), 0, 0, 0]
    for c, mem in members.items():
        r = mem[0]
        for i in mem[1:]:
            if tab[i][3] > tab[r][3]:
                r = i
        stays = [i for i in mem if i == r or pair_test(tab[min(i, r)], tab[max(i, r)], cos_min, max_gap)]
        for i in mem:
            rep[i] = r
        for i in stays:
            group[i] = stays[0]
        if len(mem) >= 2:
            counts[1] += 1
            counts[2] += len(mem) - len(stays)
            counts[3] += len(stays) >= 2
    return dict(group=np.array(group, np.int32), pairs=np.array(pairs, np.int32).reshape(-1, 2), counts=np.array(counts, np.int32),
                comp=np.array(comp, np.int32), rep=np.array(rep, np.int32))


def line_tol(P, Q, members, views, dist_px):
    """tol = dist_px x the mean over the members, in their stored order, of z / f: z = R[2] . M + t[2] at M = (P + Q) / 2, f = (|K00| + |K11|) / 2 of the
    member's view.  Members with z <= 0 or a term that is not finite are skipped; none left: 0.  members: (camera, segment); views: id -> dict(K, R, t)"""
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
    return F(dist_px) * (total / F(cnt)) if cnt else F(0.0)


def merge_rounds(result, views, refit, dist_px=4.0, angle_deg=5.0, max_gap=0.0, max_rounds=3):
    """The round loop on a result list [(members [(cam, seg)...] in key order, segs3d (k, 6))...].  refit(members) -> segs3d (k, 6), k may be 0.
    -> (merged result, rounds: per round dict(n_before, pairs, group, n_after, merged, released, empty_refits, result: the list after the round),
    final_index per line of the input, n_sources per final line)"""
    cos_min = np.cos(F(angle_deg) * F(np.pi) / F(180.0))
    result = [(list(m), np.asarray(s, F).reshape(-1, 6)) for m, s in result]
    src = [[k] for k in range(len(result))]
    rounds = []
    for _ in range(max_rounds):
        n = len(result)
        lines = np.array([list(s[0, :3]) + list(s[-1, 3:]) for _, s in result], F).reshape(n, 6)
        tol = [line_tol(lines[k, :3], lines[k, 3:], result[k][0], views, dist_px) for k in range(n)]
        g = group_lines(lines, tol, cos_min, max_gap)
        rec = dict(n_before=n, pairs=g["pairs"], group=g["group"], merged=0, released=int(g["counts"][2]), empty_refits=0)
        if len(g["pairs"]) == 0:
            rec["n_after"] = n
            rec["result"] = list(result)
            rounds.append(rec)
            break
        out, out_src, unmerged = [], [], set()
        for k in range(n):
            gk = int(g["group"][k])
            if gk != k and gk not in unmerged:
                continue                                    # merged into the line at position gk
            mem = [i for i in range(n) if g["group"][i] == k] if gk == k else []
            if len(mem) >= 2:
                union = sorted(set((int(c), int(s)) for i in mem for c, s in result[i][0]))
                segs = np.asarray(refit(union), F).reshape(-1, 6)
                if len(segs):
                    out.append((union, segs))
                    out_src.append(sorted(x for i in mem for x in src[i]))
                    rec["merged"] += 1
                    continue
                rec["empty_refits"] += 1                    # the group's lines stay as they were
                unmerged.add(k)
            out.append(result[k])
            out_src.append(src[k])
        result, src = out, out_src
        rec["n_after"] = len(result)
        rec["result"] = list(result)
        rounds.append(rec)
    final_index = np.zeros(sum(len(s) for s in src), np.int32)
    for k, s in enumerate(src):
        final_index[s] = k
    return result, rounds, final_index, np.array([len(s) for s in src], np.int32)
