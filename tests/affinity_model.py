"""The affinity fill of Line3D::clusterSegments2D (line3D.cc:968-1221) as a plain model over the flat tables of l3d_affinity_input (dense segment ids,
CSR potential correspondences and collinearities, best, hyp_dense): the reference's rule applied literally with a set of `used` pairs, as
oracle/l3d_oracle_pipeline.py: cluster_segments_2D does on its maps.  Beside the candidate list it records what the device fill (l3d_affinity.hip)
leaves behind on the way: one byte per potential-correspondence entry (k_aff_groups), needs_prev and the launch schedule, weights, first-touch
numbering, a part's passed list and minima, and the verdict of the table check.  Nothing here is shaped like the kernels: no groups, no passes, no
words -- a table is walked source by source, entry by entry."""
import numpy as np

F32 = np.float32
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)

WHAT = ["", "a CSR range is out of bounds", "a potential correspondence is out of range, in the source's own view, or out of order",
        "a collinearity entry is out of range, in another view, a self entry, or out of order", "best[] and hyp_dense[] disagree",
        "hypotheses are not numbered in dense order"]
HOST_CSR0 = "affinity fill: CSR tables must start at 0"
HOST_ASCEND = "affinity fill: view tables must ascend"
HOST_COVER = "affinity fill: view tables do not cover the hypotheses"
HOST_ARG = "bad argument"

TABLE_KEYS = ("seg_base", "view_hyp_begin", "hyp", "score", "hyp_dense", "best", "pot_start", "pot_tgt", "coll_start", "coll_other", "coll_w")


def dview_of(t):
    sb = np.asarray(t["seg_base"])
    return np.repeat(np.arange(len(sb) - 1), np.diff(sb)).astype(np.int32)


def enumerate_candidates(t):
    """-> dict(items: list of (a, b, family, cw) in the reference's order, src_count: candidates per source hypothesis, flags: uint8 per potential
    correspondence entry -- bit 0 marked as a target, bit 1 expanded (marked and with a hypothesis), bit 2 m-used (the target's EARLIER hypothesis marked
    the source while it was the source); entries of segments without a hypothesis stay 0)."""
    nh = len(t["hyp_dense"])
    best, ps, pt, cs, co, cw = t["best"], t["pot_start"], t["pot_tgt"], t["coll_start"], t["coll_other"], t["coll_w"]
    flags = np.zeros(len(pt), np.uint8)
    used = set()
    items, src_count = [], np.zeros(nh, np.int64)
    for si in range(nh):
        d = int(t["hyp_dense"][si])
        n0 = len(items)
        for e in range(int(ps[d]), int(ps[d + 1])):          # what the earlier iterations left: read before this one marks anything
            if (d, int(pt[e])) in used:
                flags[e] |= 4

        def meet(x):
            if (d, x) in used:
                return False
            used.add((d, x))
            used.add((x, d))
            return True
        for e in range(int(ps[d]), int(ps[d + 1])):          # line3D.cc:996-1138
            x = int(pt[e])
            if not meet(x):
                continue
            flags[e] |= 1
            if best[x] < 0:
                continue
            flags[e] |= 2
            items.append((si, int(best[x]), 0, F32(0)))
            for q in range(int(cs[x]), int(cs[x + 1])):      # :1065-1136
                c = int(co[q])
                if meet(c) and best[c] >= 0:
                    items.append((si, int(best[c]), 1, F32(0)))
        for q in range(int(cs[d]), int(cs[d + 1])):          # :1141-1214
            x = int(co[q])
            if meet(x) and best[x] >= 0:
                items.append((si, int(best[x]), 2, F32(cw[q])))
        src_count[si] = len(items) - n0
    return dict(items=items, src_count=src_count, flags=flags)


def replay_flags(t, flags):
    """The candidate list again, from the byte flags alone: family 0 <=> bit 1; a family-1 entry c of an expanded target is a candidate unless it is a
    target of the source at or before the expanded one's group position, an earlier expanded target of the same view lists it, or its own earlier
    hypothesis marked the source (found from that hypothesis' flags); family 2: x is skipped <=> its hypothesis is earlier and x lists the source."""
    nh = len(t["hyp_dense"])
    best, ps, pt, cs, co, cw = t["best"], t["pot_start"], t["pot_tgt"], t["coll_start"], t["coll_other"], t["coll_w"]
    dv = dview_of(t)
    coll = lambda x: [int(v) for v in co[int(cs[x]):int(cs[x + 1])]]

    def marked_by(hb, d):       # did hypothesis hb's iteration mark segment d of another view?
        x = int(t["hyp_dense"][hb])
        for e in range(int(ps[x]), int(ps[x + 1])):
            tt = int(pt[e])
            if tt == d or (dv[tt] == dv[d] and (flags[e] & 2) and d in coll(tt)):
                return True
        return False
    items = []
    for si in range(nh):
        d = int(t["hyp_dense"][si])
        ent = list(range(int(ps[d]), int(ps[d + 1])))
        for k, e in enumerate(ent):
            if not flags[e] & 2:
                continue
            x = int(pt[e])
            items.append((si, int(best[x]), 0, F32(0)))
            group_before = [f for f in ent[:k] if dv[int(pt[f])] == dv[x]]
            for c in coll(x):
                if c in [int(pt[f]) for f in group_before]:
                    continue
                if any((flags[f] & 2) and c in coll(int(pt[f])) for f in group_before):
                    continue
                hb = int(best[c])
                if hb < 0 or (hb < si and marked_by(hb, d)):
                    continue
                items.append((si, hb, 1, F32(0)))
        for q in range(int(cs[d]), int(cs[d + 1])):
            x = int(co[q])
            hb = int(best[x])
            if hb >= 0 and not (hb < si and d in coll(x)):
                items.append((si, hb, 2, F32(cw[q])))
    return items


def needs_prev(t, assume_symmetric=False):
    """needs_prev[v] = 1: a source of view v has a target with an EARLIER hypothesis that does not list the source (its m-used test reads bits of the
    views before v).  assume_symmetric: the caller vouches for the reverse records, nothing is looked up."""
    V = len(t["seg_base"]) - 1
    out = np.zeros(V, np.int32)
    if assume_symmetric:
        return out
    dv = dview_of(t)
    ps, pt, best = t["pot_start"], t["pot_tgt"], t["best"]
    for si, d in enumerate(t["hyp_dense"]):
        for e in range(int(ps[d]), int(ps[d + 1])):
            x = int(pt[e])
            if 0 <= best[x] < si and int(d) not in [int(v) for v in pt[int(ps[x]):int(ps[x + 1])]]:
                out[dv[d]] = 1
    return out


def group_launches(t, per_view=False, assume_symmetric=False):
    """launches of k_aff_groups: runs of views, cut in front of a view with needs_prev; only runs that hold a hypothesis count"""
    V = len(t["seg_base"]) - 1
    vhb = t["view_hyp_begin"]
    cut = needs_prev(t, assume_symmetric)
    n, v0 = 0, 0
    while v0 < V:
        v1 = v0 + 1
        while v1 < V and not cut[v1] and not per_view:
            v1 += 1
        if vhb[v1] > vhb[v0]:
            n += 1
        v0 = v1
    return n


def weights(t, items, sim):
    """float32 operation order of line3D.cc:1014 / :1085 / :1163 -> (w float32, passed bool)"""
    sc = np.asarray(t["score"], F32)
    n = len(items)
    a = np.array([i[0] for i in items], np.int64).reshape(n)
    b = np.array([i[1] for i in items], np.int64).reshape(n)
    fam = np.array([i[2] for i in items], np.int64).reshape(n)
    cw = np.array([i[3] for i in items], F32).reshape(n)
    sim = np.asarray(sim, F32).reshape(n)
    half = F32(0.5)
    ssum = (sc[a] + sc[b]).astype(F32)
    w01 = ((half * ssum).astype(F32) * sim).astype(F32)
    w2 = (((cw * half).astype(F32) * ssum).astype(F32) * sim).astype(F32)
    w = np.where(fam == 2, w2, w01).astype(F32)
    passed = w > np.where(fam == 0, F32(0.25), F32(0.01))
    return w, passed


def edge_list(t, items, sim, edge_dtype):
    """first-touch node numbering (source before target, passed candidates only) -> (edges (a,b,w), (b,a,w); node_hyp)"""
    w, passed = weights(t, items, sim)
    node, node_hyp = {}, []
    A = np.zeros(2 * int(passed.sum()), edge_dtype)
    k = 0
    for it, wv, ok in zip(items, w, passed):
        if not ok:
            continue
        for h in it[:2]:
            if h not in node:
                node[h] = len(node_hyp)
                node_hyp.append(h)
        A[k] = (node[it[0]], node[it[1]], wv)
        A[k + 1] = (node[it[1]], node[it[0]], wv)
        k += 2
    return A, np.array(node_hyp, np.int32).reshape(len(node_hyp))


def part(t, items, sim, h0, h1, pos_base=0, loc2glob=None):
    """A rank's part: the candidates of the sources [h0, h1) -> dict(pairs int32 (n, 2) of the passed ones, in global numbers; w; first: per LOCAL
    hypothesis 2 * (pos_base + position) + side as a minimum, ~0 = never touched -- position counts ALL candidates of the part, failed ones too;
    n_candidates)"""
    nh = len(t["hyp_dense"])
    w, passed = weights(t, items, sim)
    first = np.full(nh, NONE64, np.uint64)
    pairs, ws, pos = [], [], 0
    for it, wv, ok in zip(items, w, passed):
        if not h0 <= it[0] < h1:
            continue
        if ok:
            for side, h in enumerate(it[:2]):
                first[h] = min(first[h], np.uint64(2 * (int(pos_base) + pos) + side))
            pairs.append([it[0], it[1]] if loc2glob is None else [int(loc2glob[it[0]]), int(loc2glob[it[1]])])
            ws.append(wv)
        pos += 1
    return dict(pairs=np.array(pairs, np.int32).reshape(len(pairs), 2), w=np.array(ws, F32).reshape(len(ws)), first=first, n_candidates=pos)


def merge_parts(parts, loc2glob, n_hyp_global, edge_dtype):
    """the parts' passed lists in rank order + the element-wise minimum of their minima (scattered to global numbers) -> (edges, node_hyp), numbered by
    ascending first position"""
    first = np.full(n_hyp_global, NONE64, np.uint64)
    for p in parts:
        g = np.arange(len(p["first"])) if loc2glob is None else np.asarray(loc2glob)
        first[g] = np.minimum(first[g], p["first"])
    touched = np.flatnonzero(first != NONE64)
    order = touched[np.argsort(first[touched], kind="stable")]
    node = np.full(n_hyp_global, -1, np.int64)
    node[order] = np.arange(len(order))
    pairs = np.concatenate([p["pairs"] for p in parts]) if parts else np.zeros((0, 2), np.int32)
    w = np.concatenate([p["w"] for p in parts]) if parts else np.zeros(0, F32)
    A = np.zeros(2 * len(pairs), edge_dtype)
    A["i"][0::2], A["j"][0::2], A["w"][0::2] = node[pairs[:, 0]], node[pairs[:, 1]], w
    A["i"][1::2], A["j"][1::2], A["w"][1::2] = node[pairs[:, 1]], node[pairs[:, 0]], w
    return A, order.astype(np.int32)


def validate(t):
    """-> (codes, message, symmetric).  codes: what the table check must answer -- () for a valid table; ("host", message) for what l3d_affinity_fill
    refuses before anything is launched; otherwise the codes k_aff_validate's threads raise (one thread per dense id and per hypothesis, each stopping
    at its first finding; where several codes are raised any one of them may come back -- every crafted table raises exactly one).  symmetric: the
    collinearity table holds every entry both ways (only meaningful for a valid table)."""
    sb, vhb = [int(v) for v in t["seg_base"]], [int(v) for v in t["view_hyp_begin"]]
    V, nh = len(sb) - 1, len(t["hyp_dense"])
    ps, pt, cs, co, best, hd = t["pot_start"], t["pot_tgt"], t["coll_start"], t["coll_other"], t["best"], t["hyp_dense"]
    if nh == 0:
        return (), "", True
    nd = sb[V]
    if nd <= 0:
        return ("host", HOST_ARG), HOST_ARG, False
    if ps[0] != 0 or cs[0] != 0:
        return ("host", HOST_CSR0), HOST_CSR0, False
    for v in range(V):
        if sb[v + 1] < sb[v] or vhb[v + 1] < vhb[v]:
            return ("host", HOST_ASCEND), HOST_ASCEND, False
    if sb[0] != 0 or vhb[0] != 0 or vhb[V] != nh:
        return ("host", HOST_COVER), HOST_COVER, False
    n_pot, n_coll = int(ps[nd]), int(cs[nd])
    if n_pot < 0 or n_coll < 0:
        return ("host", HOST_ARG), HOST_ARG, False
    dv = np.repeat(np.arange(V), np.diff(sb))
    codes, sym = set(), True

    def seg_thread(i):
        nonlocal sym
        pb, pe, cb, ce = int(ps[i]), int(ps[i + 1]), int(cs[i]), int(cs[i + 1])
        if pb < 0 or pe < pb or pe > n_pot or cb < 0 or ce < cb or ce > n_coll:
            return codes.add(1)
        v = dv[i]
        for e in range(pb, pe):
            x = int(pt[e])
            if x < 0 or x >= nd or dv[x] == v or (e > pb and pt[e - 1] >= x):
                return codes.add(2)
        for q in range(cb, ce):
            x = int(co[q])
            if x < 0 or x >= nd or dv[x] != v or x == i or (q > cb and co[q - 1] >= x):
                return codes.add(3)
        for q in range(cb, ce):
            x = int(co[q])
            xb, xe = int(cs[x]), int(cs[x + 1])
            if xb < 0 or xe < xb or xe > n_coll:
                break
            if i not in [int(u) for u in co[xb:xe]]:
                sym = False
                break
        hb = int(best[i])
        if hb < -1 or hb >= nh or (hb >= 0 and hd[hb] != i):
            codes.add(4)
    for i in range(nd):
        seg_thread(i)
    for h in range(nh):
        d = int(hd[h])
        if d < 0 or d >= nd or best[d] != h or (h > 0 and hd[h - 1] >= d):
            codes.add(5)
    codes = tuple(sorted(codes))
    return codes, ("affinity fill: " + WHAT[codes[0]]) if codes else "", sym and not codes
