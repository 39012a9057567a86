"""Crafted tables for the affinity fill (l3d_affinity.hip): every case is a dict with the flat tables of l3d_affinity_input (key "t"), a `why`, the
option sets that matter for it (`sets`, names of tests/test_gpu_affinity_paths.py: OPTION_SETS) and a `reach` predicate over the model's output
(affinity_model.py; run_model below) that proves the case reaches the branch it was built for.

Hypotheses lie on one of two 3-D lines through the origin, the x-axis ("x") or the y-axis ("y"), all with depth_p1 = depth_p2 = median_depth = 1,
k_lower = 0.1, k_upper = 0.2: two of one class have similarity exactly 1 (distance 0 is below the lower bound, acos(1) = 0), two of different classes
exactly 0 (the point-to-line distance 1 is far outside the upper bound and the angular term at 90 degrees far below the 0.01 cut).  Every weight is
therefore an exact float32 product of scores and collinearity weights, chosen per case; no expf accuracy enters.  The one table with generic lines
("real_geometry") takes its similarities from the similarity seam call (pinned to the oracle elsewhere)."""
import numpy as np

import affinity_model as am

F32 = np.float32
HYP_DTYPE = np.dtype([("P1", "<f8", (3,)), ("P2", "<f8", (3,)), ("dir", "<f8", (3,)), ("depth_p1", "<f4"), ("depth_p2", "<f4"),
                      ("k_lower", "<f4"), ("k_upper", "<f4"), ("median_depth", "<f4"), ("pad", "<u4")])
SIGMA_A = 10.0
C25, C01 = F32(0.25), F32(0.01)
UP = lambda x: np.nextafter(F32(x), F32(np.inf))


def hyp_record(cls):
    h = np.zeros((), HYP_DTYPE)
    if cls == "x":
        h["P1"], h["P2"], h["dir"] = (1, 0, 0), (2, 0, 0), (1, 0, 0)
    else:
        h["P1"], h["P2"], h["dir"] = (0, 1, 0), (0, 2, 0), (0, 1, 0)
    h["depth_p1"] = h["depth_p2"] = h["median_depth"] = 1.0
    h["k_lower"], h["k_upper"] = 0.1, 0.2
    return h


class Build:
    """sizes: segments per view.  seg(v, k) = dense id.  hyp(d, cls, score); link(a, b) a potential correspondence (both ways unless one_way: a lists b
    only); col(a, b, w) a collinearity (both ways unless one_way: a lists b only)."""

    def __init__(self, sizes):
        self.seg_base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.nd = int(self.seg_base[-1])
        self.hyps, self.pot, self.coll = {}, {}, {}

    def seg(self, v, k):
        assert 0 <= k < self.seg_base[v + 1] - self.seg_base[v]
        return int(self.seg_base[v]) + k

    def view(self, d):
        return int(np.searchsorted(self.seg_base, d, side="right") - 1)

    def hyp(self, d, cls="x", score=1.0):
        self.hyps[d] = (cls, F32(score))
        return d

    def all_hyp(self, cls="x", score=1.0, skip=()):
        for d in range(self.nd):
            if d not in skip:
                self.hyp(d, cls, score)

    def link(self, a, b, one_way=False):
        assert self.view(a) != self.view(b)
        self.pot.setdefault(a, set()).add(b)
        if not one_way:
            self.pot.setdefault(b, set()).add(a)

    def col(self, a, b, w=1.0, one_way=False):
        assert self.view(a) == self.view(b) and a != b
        self.coll.setdefault(a, {})[b] = F32(w)
        if not one_way:
            self.coll.setdefault(b, {})[a] = F32(w)

    def table(self):
        nd = self.nd
        hd = np.array(sorted(self.hyps), np.int32).reshape(len(self.hyps))
        best = np.full(nd, -1, np.int32)
        best[hd] = np.arange(len(hd))
        hyp = np.zeros(len(hd), HYP_DTYPE)
        score = np.zeros(len(hd), F32)
        for h, d in enumerate(hd):
            hyp[h], score[h] = hyp_record(self.hyps[int(d)][0]), self.hyps[int(d)][1]
        vhb = np.searchsorted(hd, self.seg_base).astype(np.int32)
        ps, cs = np.zeros(nd + 1, np.int64), np.zeros(nd + 1, np.int64)
        pt, co, cw = [], [], []
        for d in range(nd):
            pt += sorted(self.pot.get(d, ()))
            ps[d + 1] = len(pt)
            for x in sorted(self.coll.get(d, {})):
                co.append(x)
                cw.append(self.coll[d][x])
            cs[d + 1] = len(co)
        return dict(seg_base=self.seg_base.copy(), view_hyp_begin=vhb, hyp=hyp, score=score, hyp_dense=hd, best=best, pot_start=ps,
                    pot_tgt=np.array(pt, np.int32).reshape(len(pt)), coll_start=cs, coll_other=np.array(co, np.int32).reshape(len(co)),
                    coll_w=np.array(cw, F32).reshape(len(cw)), sigma_a=SIGMA_A)


def exact_sim(t, items):
    """1 for two hypotheses of one class, 0 for two of different classes (see the module's docstring)"""
    d = t["hyp"]["dir"]
    return np.array([1.0 if (d[a] == d[b]).all() else 0.0 for a, b, _, _ in items], F32).reshape(len(items))


def two_way(t):
    ps, pt = t["pot_start"], t["pot_tgt"]
    lists = [set(int(x) for x in pt[int(ps[d]):int(ps[d + 1])]) for d in range(len(ps) - 1)]
    return all(d in lists[x] for d in range(len(lists)) for x in lists[d])


def run_model(t, sim=None):
    """everything the tests compare, from the model: candidates, flags, schedule, table verdict and (with similarities) weights and the edge list"""
    m = am.enumerate_candidates(t)
    m["needs_prev"] = am.needs_prev(t)
    m["launches"] = am.group_launches(t)
    m["launches_per_view"] = am.group_launches(t, per_view=True)
    m["codes"], m["message"], m["sym"] = am.validate(t)
    m["two_way"] = two_way(t)
    if sim is None and t.get("sim", "exact") == "exact":
        sim = exact_sim(t, m["items"])
    if sim is not None:
        m["sim"] = sim
        m["w"], m["passed"] = am.weights(t, m["items"], sim)
        m["edges"], m["node_hyp"] = am.edge_list(t, m["items"], sim, np.dtype([("i", "<i4"), ("j", "<i4"), ("w", "<f4")]))
    return m


# ---- helpers for the predicates ----------------------------------------------------------------------------------------------------------------------
def entry(t, d, x):
    """index of the potential-correspondence entry (source segment d, target x)"""
    ps, pt = t["pot_start"], t["pot_tgt"]
    for e in range(int(ps[d]), int(ps[d + 1])):
        if pt[e] == x:
            return e
    raise KeyError((d, x))


def flag(m, t, d, x):
    return int(m["flags"][entry(t, d, x)])


def has_item(m, t, d, x, fam):
    return (int(t["best"][d]), int(t["best"][x]), fam) in {(a, b, f) for a, b, f, _ in m["items"]}


def n_items(m, t, d, x):
    return sum(1 for a, b, _, _ in m["items"] if a == t["best"][d] and b == t["best"][x])


def pass_T(t, m, d, chunk=64):
    """flattened entry counts T of the passes of source segment d: every expanded target contributes itself and its collinear list"""
    ps, pt, cs = t["pot_start"], t["pot_tgt"], t["coll_start"]
    out = []
    for c0 in range(int(ps[d]), int(ps[d + 1]), chunk):
        out.append(sum(1 + int(cs[pt[e] + 1] - cs[pt[e]]) for e in range(c0, min(c0 + chunk, int(ps[d + 1]))) if m["flags"][e] & 2))
    return out


CASES = {}
BASIC = ("default", "sym0", "chunk5")
CHUNKS = ("default", "sym0", "chunk1", "chunk2", "chunk5", "chunk63", "mixed_a", "mixed_b")


def case(name, b, why, reach, sets=BASIC, **kw):
    assert name not in CASES
    t = b.table() if isinstance(b, Build) else b
    CASES[name] = dict(t=t, why=why, reach=reach, sets=tuple(sets), **kw)


# ---- groups (k_aff_groups) ---------------------------------------------------------------------------------------------------------------------------
def star(counts, pad=1):
    """segment 0 of view 0 lists counts[v] targets of view v + 1 (its first segments; `pad` more segments behind them)"""
    b = Build([1] + [c + pad for c in counts])
    for v, c in enumerate(counts):
        for k in range(c):
            b.link(0, b.seg(v + 1, k))
    return b


for n in (1, 2, 63, 64, 65, 128, 129):
    b = star([n])
    b.all_hyp()
    case("group_%d" % n, b, "one group of %d targets of one view, no collinearity: every target marked and expanded; T = targets per pass" % n,
         lambda m, t, n=n: int((m["flags"][:n] == 3).sum()) == n and m["src_count"][0] == n and pass_T(t, m, 0)[0] == min(n, 64),
         sets=CHUNKS if n in (65, 129) else BASIC)

b = star([63, 3])
b.all_hyp()
for k in range(2):
    b.col(b.seg(2, k), b.seg(2, k + 1))
case("group_starts_in_lane_63", b, "63 targets of view 1, then 3 collinear targets of view 2: the second group starts in lane 63 and goes on in the next pass",
     lambda m, t: [flag(m, t, 0, t["seg_base"][2] + k) for k in range(3)] == [3, 0, 3] and t["pot_start"][1] == 66, sets=CHUNKS)

b = star([60, 4])
b.all_hyp()
b.col(b.seg(2, 0), b.seg(2, 3))
case("group_ends_in_lane_63", b, "60 targets of view 1, then 4 of view 2 whose first lists the last: lane 63 belongs to the group that starts in lane 60 -- a lane 63 that "
     "took the whole pass for its group would test the head of view 1's group where the head of its own lists it (general path: sym0)",
     lambda m, t: [flag(m, t, 0, t["seg_base"][2] + k) for k in range(4)] == [3, 3, 3, 0] and t["pot_start"][1] == 64, sets=CHUNKS)

b = star([3, 3, 3])
b.all_hyp()
for v in (1, 2, 3):
    b.col(b.seg(v, 0), b.seg(v, 1))
case("three_views_one_pass", b, "three groups in one pass, each with a collinear pair at its head",
     lambda m, t: [flag(m, t, 0, x) for x in t["pot_tgt"][:9]] == [3, 0, 3] * 3)

b = star([5])
b.all_hyp(skip=(2, 4))
b.col(2, 3)
b.col(4, 5)
case("no_hypothesis_mid_group", b, "targets without a hypothesis in mid-group: marked, not expanded, so their collinear segments behind them are still marked",
     lambda m, t: [flag(m, t, 0, x) for x in (1, 2, 3, 4, 5)] == [3, 1, 3, 1, 3])


# ---- collinear chains among the targets of one group -------------------------------------------------------------------------------------------------
def chain(n, no_hyp_every=0):
    b = star([n])
    b.all_hyp(skip=[1 + k for k in range(n) if no_hyp_every and k % no_hyp_every == 2])
    for k in range(n - 1):
        b.col(1 + k, 2 + k)
    return b


def chain_flags(m, t, n):
    return [flag(m, t, 0, 1 + k) for k in range(n)]


case("chain_64", chain(64), "t_k lists t_k+-1, all with hypotheses: marked targets alternate -- 64 resolution rounds in the symmetric variant",
     lambda m, t: chain_flags(m, t, 64) == [3, 0] * 32, sets=CHUNKS)
case("chain_64_every_third_without_hypothesis", chain(64, 3), "the chain with every third target lacking a hypothesis: a marked, unexpanded target frees its successor",
     lambda m, t: chain_flags(m, t, 6) == [3, 0, 1, 3, 0, 1] and 1 in chain_flags(m, t, 64)[60:], sets=CHUNKS)
case("chain_70", chain(70), "the chain of 70 targets crosses the pass boundary at chunk 64 (the gs < c0 read-back of both variants) and every boundary at chunk 5",
     lambda m, t: chain_flags(m, t, 70) == [3, 0] * 35 and flag(m, t, 0, 64) == 0 and flag(m, t, 0, 65) == 3, sets=CHUNKS)
case("chain_130_straddles_every_pass", chain(130), "one group of 130 chained targets: it straddles every pass at chunks 1, 2, 5, 63 and 64",
     lambda m, t: chain_flags(m, t, 130) == [3, 0] * 65, sets=CHUNKS)

b = star([65])
b.all_hyp()
for k in range(1, 65):
    b.col(1, 1 + k)
case("fan_65", b, "t0 lists all others: the general path's two-iteration case; the targets of the second pass find t0's bit by read-back",
     lambda m, t: chain_flags(m, t, 65) == [3] + [0] * 64 and m["src_count"][0] == 65, sets=CHUNKS)

b = star([5, 5])
b.all_hyp()
for v in (1, 2):
    for k in range(4):
        b.col(b.seg(v, k), b.seg(v, k + 1))
case("two_chains_two_groups", b, "two disjoint chains in two groups of one pass",
     lambda m, t: [flag(m, t, 0, x) for x in t["pot_tgt"][:10]] == [3, 0, 3, 0, 3] * 2)

# ---- asymmetric collinearity ----------------------------------------------------------------------------------------------------------------------------
b = star([2])
b.all_hyp()
b.col(1, 2, one_way=True)
case("asym_t0_lists_t1", b, "t0 lists t1 only: t1 is met as t0's collinear segment (family 1) and not marked as a target; coll_sym must come back 0",
     lambda m, t: not m["sym"] and chain_flags(m, t, 2) == [3, 0] and has_item(m, t, 0, 2, 1))
b = star([2])
b.all_hyp()
b.col(2, 1, one_way=True)
case("asym_t1_lists_t0", b, "t1 lists t0 only: t1 is marked and expanded, t0 in its list is no second candidate",
     lambda m, t: not m["sym"] and chain_flags(m, t, 2) == [3, 3] and n_items(m, t, 0, 1) == 1 and not has_item(m, t, 0, 1, 1))
b = star([2], pad=2)
b.all_hyp()
b.col(1, 2)
b.col(4, 3, one_way=True)
case("asym_on_last_dense_segment", b, "the one asymmetric entry sits on the last dense segment (the last thread of k_aff_validate that holds a list)",
     lambda m, t: not m["sym"] and t["coll_start"][-1] - t["coll_start"][-2] == 1 and chain_flags(m, t, 2) == [3, 0])
b = star([3])
b.all_hyp(skip=(3,))
b.col(1, 2)
b.col(3, 1, one_way=True)
case("asym_on_segment_without_hypothesis", b, "the one asymmetric entry sits on a segment without a hypothesis: its list is never walked, the general path still has to be taken",
     lambda m, t: not m["sym"] and chain_flags(m, t, 3) == [3, 0, 1])
b = Build([1, 3, 2])
b.all_hyp()
b.link(0, 1), b.link(0, 2)
b.col(1, 2)
b.col(4, 5, one_way=True)
case("asym_in_view_nobody_targets", b, "the one asymmetric entry sits in a view that holds no target of anyone: it changes no decision except a family-2 one, but the table is not symmetric",
     lambda m, t: not m["sym"] and chain_flags(m, t, 2) == [3, 0] and has_item(m, t, 4, 5, 2) and has_item(m, t, 5, 4, 2) is False)

# ---- family 1 decisions: one sub-case per skip -------------------------------------------------------------------------------------------------------
b = star([2])
b.all_hyp(skip=(1,))
b.col(1, 2)
case("f1_c_is_earlier_target", b, "c is an earlier target of the group (marked, without a hypothesis): t1's list names it, no candidate",
     lambda m, t: chain_flags(m, t, 2) == [1, 3] and m["src_count"][0] == 1)
b = star([2])
b.all_hyp()
b.col(1, 2)
case("f1_c_is_later_target", b, "c is a LATER target of the group: a candidate of family 1, and that target is then not marked",
     lambda m, t: chain_flags(m, t, 2) == [3, 0] and has_item(m, t, 0, 2, 1) and not has_item(m, t, 0, 2, 0))
b = star([2], pad=1)
b.all_hyp()
b.col(1, 3), b.col(2, 3)
case("f1_c_listed_by_earlier_expanded", b, "c is listed by an earlier expanded target: one candidate, from the first",
     lambda m, t: chain_flags(m, t, 2) == [3, 3] and n_items(m, t, 0, 3) == 1 and m["src_count"][0] == 3)
b = star([2], pad=1)
b.all_hyp(skip=(1,))
b.col(1, 3), b.col(2, 3)
case("f1_c_listed_by_earlier_unexpanded", b, "c is listed by an earlier target that is marked but not expanded: its list was never walked, c is t1's candidate",
     lambda m, t: chain_flags(m, t, 2) == [1, 3] and n_items(m, t, 0, 3) == 1)
b = Build([2, 1])
b.all_hyp()
b.col(0, 1)
b.link(2, 0, one_way=True)
b.link(1, 2)
case("f1_c_mused_source_is_its_target", b, "c has an earlier hypothesis and the source is one of c's targets: c, met in t's list, is m-used (met_by's first arm); t itself comes by a one-way record",
     lambda m, t: flag(m, t, 2, 0) == 3 and not has_item(m, t, 2, 1, 1) and not has_item(m, t, 2, 1, 0) and has_item(m, t, 2, 0, 0) and flag(m, t, 2, 1) == 4,
     sets=BASIC + ("per_view",))
b = Build([2, 2])
b.all_hyp()
b.col(0, 1), b.col(2, 3)
b.link(1, 2)
b.link(3, 0, one_way=True)
case("f1_c_mused_through_collinear_of_expanded", b, "c has an earlier hypothesis and an expanded target of c lists the source as collinear (met_by's second arm)",
     lambda m, t: flag(m, t, 3, 0) == 3 and has_item(m, t, 1, 3, 1) and not has_item(m, t, 3, 1, 1) and has_item(m, t, 3, 0, 0), sets=BASIC + ("per_view",))
b = star([1], pad=1)
b.all_hyp(skip=(2,))
b.col(1, 2)
case("f1_c_without_hypothesis", b, "c has no hypothesis: marked, no candidate", lambda m, t: flag(m, t, 0, 1) == 3 and m["src_count"][0] == 1)

# ---- one-way potential records -------------------------------------------------------------------------------------------------------------------------
b = Build([1, 2])
b.all_hyp()
b.link(0, 1)
b.col(1, 2)
b.link(2, 0, one_way=True)
case("one_way_marked_through_collinear", b, "d lists t, t has an earlier hypothesis and does not list d, but t's iteration marked d through the list of its expanded target: d finds t m-used without the reverse record",
     lambda m, t: list(m["needs_prev"]) == [0, 1] and flag(m, t, 2, 0) == 4 and m["src_count"][2] == 0 and m["launches"] == 2, sets=BASIC + ("per_view",))
b = Build([1, 1])
b.all_hyp()
b.link(1, 0, one_way=True)
case("one_way_not_marked", b, "d lists t, t has an earlier hypothesis and never met d: t is not m-used, a candidate",
     lambda m, t: list(m["needs_prev"]) == [0, 1] and flag(m, t, 1, 0) == 3 and has_item(m, t, 1, 0, 0) and m["launches"] == 2, sets=BASIC + ("per_view",))


def one_way_views(V, where):
    b = Build([2] * V)
    b.all_hyp()
    for v in range(V - 1):
        b.link(b.seg(v, 0), b.seg(v + 1, 0))
    for v in where:
        b.link(b.seg(v, 1), b.seg(v - 1, 1), one_way=True)
    return b


case("one_way_in_view_1", one_way_views(3, [1]), "the one-way record in view 1 of three: launches {0}, {1, 2}",
     lambda m, t: list(m["needs_prev"]) == [0, 1, 0] and m["launches"] == 2 and m["launches_per_view"] == 3, sets=BASIC + ("per_view",))
case("one_way_in_last_view", one_way_views(3, [2]), "the one-way record in the last view: launches {0, 1}, {2}",
     lambda m, t: list(m["needs_prev"]) == [0, 0, 1] and m["launches"] == 2, sets=BASIC + ("per_view",))
case("one_way_in_two_views_of_five", one_way_views(5, [1, 3]), "one-way records in two non-adjacent views of five: launches {0}, {1, 2}, {3, 4}",
     lambda m, t: list(m["needs_prev"]) == [0, 1, 0, 1, 0] and m["launches"] == 3 and m["launches_per_view"] == 5, sets=BASIC + ("per_view",))
b = Build([2, 2, 2])
for d in (0, 1, 4, 5):
    b.hyp(d)
b.link(0, 2), b.link(0, 4)
b.link(5, 1, one_way=True)
case("view_without_hypothesis_before_cut", b, "a view with no hypothesis in front of a cut: launches {0, 1}, {2}; one launch per view makes 2 as well",
     lambda m, t: list(m["needs_prev"]) == [0, 0, 1] and m["launches"] == 2 and m["launches_per_view"] == 2 and flag(m, t, 0, 2) == 1, sets=BASIC + ("per_view",))
b = Build([1, 1])
b.all_hyp()
b.link(0, 1, one_way=True)
case("one_way_to_later_hypothesis", b, "d lists t, t has a LATER hypothesis and no reverse record: nothing to wait for, no cut",
     lambda m, t: list(m["needs_prev"]) == [0, 0] and m["launches"] == 1 and has_item(m, t, 0, 1, 0) and not m["two_way"], sets=BASIC + ("per_view",))

# ---- family 2 ------------------------------------------------------------------------------------------------------------------------------------------
b = Build([3, 1])
b.all_hyp(skip=(2,))
b.col(0, 1), b.col(1, 2)
case("f2_earlier_lists_source_and_without_hypothesis", b, "x earlier and lists the source: skipped; x later: a candidate; x without a hypothesis: none",
     lambda m, t: [(a, bb, f) for a, bb, f, _ in m["items"]] == [(0, 1, 2)])
b = Build([2, 1])
b.all_hyp()
b.col(1, 0, one_way=True)
case("f2_earlier_does_not_list_source", b, "x earlier and does NOT list the source: a candidate (the table is asymmetric)",
     lambda m, t: [(a, bb, f) for a, bb, f, _ in m["items"]] == [(1, 0, 2)] and not m["sym"])
for n in (0, 1, 63, 64, 65, 130):
    b = Build([n + 1, 1])
    b.all_hyp()
    for k in range(n):
        b.col(0, 1 + k, w=0.5)
    case("f2_list_%d" % n, b, "a family-2 list of %d entries: %d decision word(s); the listed segments find the source earlier and listing them" % (n, (n + 63) // 64),
         lambda m, t, n=n: m["src_count"][0] == n and len(m["items"]) == n and all(it[3] == F32(0.5) for it in m["items"]),
         sets=BASIC + (("block32", "wblock1") if n >= 64 else ()))


# ---- word boundaries -----------------------------------------------------------------------------------------------------------------------------------
def words_case(n_targets, lists):
    """n_targets targets of view 1; lists: {target index: length of its collinear list}, the listed segments are non-targets behind the targets"""
    extra = sum(lists.values())
    b = star([n_targets], pad=extra)
    b.all_hyp()
    u = 1 + n_targets
    for k, n in sorted(lists.items()):
        for _ in range(n):
            b.col(1 + k, u)
            u += 1
    return b


for T, (n, lists) in {1: (1, {}), 63: (60, {59: 3}), 64: (64, {}), 65: (64, {63: 1}), 128: (64, {k: 1 for k in range(64)}),
                      129: (64, {k: 2 if k == 7 else 1 for k in range(64)})}.items():
    case("words_T_%d" % T, words_case(n, lists), "a pass whose flattened count T is %d" % T,
         lambda m, t, T=T: pass_T(t, m, 0)[0] == T and m["src_count"][0] == T, sets=BASIC + ("block1", "wblock1", "wblock3"))
case("words_target_is_last_bit", words_case(64, {63: 3}), "an expanded target whose own entry is bit 63 of a word and whose list starts the next",
     lambda m, t: pass_T(t, m, 0) == [67] and m["src_count"][0] == 67, sets=BASIC + ("block7", "wblock1"))
case("words_list_spans_three", words_case(11, {10: 130}), "a collinear list of 130 behind 11 entries: it spans three words",
     lambda m, t: pass_T(t, m, 0) == [141] and m["src_count"][0] == 141, sets=BASIC + ("block7", "wblock1", "mixed_b"))


# ---- thresholds and numbering ----------------------------------------------------------------------------------------------------------------------------
def weight_is(m, t, d, x, fam, w, passed):
    for (a, bb, f, _), wv, ok in zip(m["items"], m["w"], m["passed"]):
        if (a, bb, f) == (int(t["best"][d]), int(t["best"][x]), fam):
            return wv.tobytes() == F32(w).tobytes() and bool(ok) == passed
    return False


def threshold_pairs(fam, thr, s_at, s_up, cw_at=1.0, cw_up=1.0):
    """two sources, each with one candidate of the family: the first weighs exactly thr (not kept), the second the next float above (kept)"""
    if fam == 0:
        b = Build([2, 2])
        b.link(0, 2, one_way=True), b.link(1, 3, one_way=True)
    elif fam == 1:
        b = Build([2, 4])
        b.link(0, 2, one_way=True), b.link(1, 4, one_way=True)
        b.col(2, 3), b.col(4, 5)
    else:
        b = Build([4, 1])
        b.col(0, 1, w=cw_at), b.col(2, 3, w=cw_up)
    return b


SA25, SB25 = F32(0.25), F32(0.25) + F32(2.0 ** -24)                 # 0.5 * (sa + sb) = 0.25 + 2^-25 = the float above 0.25, every step exact
ULP01 = UP(C01) - C01
SB01 = F32(C01 + F32(2) * ULP01)                                     # 0.5 * (c + (c + 2 ulp)) = c + ulp, every step exact

b = threshold_pairs(0, C25, None, None)
b.hyp(0, "x", SA25), b.hyp(2, "x", SA25), b.hyp(1, "x", SA25), b.hyp(3, "x", SB25)
case("threshold_family_0", b, "a family-0 weight exactly 0.25f is not kept, the next float above is",
     lambda m, t: weight_is(m, t, 0, 2, 0, C25, False) and weight_is(m, t, 1, 3, 0, UP(C25), True) and len(m["edges"]) == 2)
b = threshold_pairs(1, C01, None, None)
b.hyp(0, "x", C01), b.hyp(2, "y", 1.0), b.hyp(3, "x", C01), b.hyp(1, "x", C01), b.hyp(4, "y", 1.0), b.hyp(5, "x", SB01)
case("threshold_family_1", b, "a family-1 weight exactly 0.01f is not kept, the next float above is (the targets themselves are of the other class: weight 0)",
     lambda m, t: weight_is(m, t, 0, 3, 1, C01, False) and weight_is(m, t, 1, 5, 1, UP(C01), True) and weight_is(m, t, 0, 2, 0, 0.0, False) and len(m["edges"]) == 2)
b = threshold_pairs(2, C01, None, None, cw_at=C01, cw_up=UP(C01))
b.all_hyp("x", 1.0, skip=(4,))
case("threshold_family_2_through_cw", b, "family 2 at 0.01f through the collinearity weight alone (scores 1: the weight IS cw)",
     lambda m, t: weight_is(m, t, 0, 1, 2, C01, False) and weight_is(m, t, 2, 3, 2, UP(C01), True) and len(m["edges"]) == 2)
b = threshold_pairs(2, C01, None, None)
b.hyp(0, "x", C01), b.hyp(1, "x", C01), b.hyp(2, "x", C01), b.hyp(3, "x", SB01)
case("threshold_family_2_through_scores", b, "family 2 at 0.01f through the scores alone (cw = 1)",
     lambda m, t: weight_is(m, t, 0, 1, 2, C01, False) and weight_is(m, t, 2, 3, 2, UP(C01), True) and len(m["edges"]) == 2)

b = Build([2, 2])
b.hyp(0, "x"), b.hyp(1, "y"), b.hyp(2, "y"), b.hyp(3, "x")
b.link(0, 2, one_way=True), b.link(0, 3, one_way=True), b.link(1, 2, one_way=True)
case("failing_candidate_before_passing_one", b, "a failing candidate names a hypothesis in front of the passing one that does: the node number comes from the passing one",
     lambda m, t: list(m["passed"]) == [False, True, True] and list(m["node_hyp"]) == [0, 3, 1, 2])
b = Build([1, 1, 1])
b.all_hyp()
b.link(0, 1), b.link(1, 2)
case("first_touched_as_target_then_source", b, "a hypothesis first touched as a target, then used as a source; all hypotheses touched",
     lambda m, t: list(m["node_hyp"]) == [0, 1, 2] and [(a, bb) for a, bb, _, _ in m["items"]] == [(0, 1), (1, 2)])
b = Build([3, 3, 2])
b.all_hyp()
b.link(1, 4), b.link(4, 6, one_way=True)
case("untouched_hypotheses_front_middle_end", b, "hypotheses never touched at the front, in the middle and at the end: they take no node, the others keep first-touch order",
     lambda m, t: list(m["node_hyp"]) == [1, 4, 6] and len(t["hyp_dense"]) == 8)
# (a family-1 candidate closes a triangle source - target - collinear segment, and of three hypotheses two share a class: families 0 and 2 only)
b = Build([2, 3])
b.hyp(0, "y"), b.hyp(1, "x"), b.hyp(2, "x"), b.hyp(3, "x"), b.hyp(4, "y")
b.link(0, 2), b.link(0, 3), b.link(1, 4)
b.col(0, 1)
case("nothing_passes", b, "every pair mixes the x and y classes: candidates, but an empty list and 0 nodes",
     lambda m, t: len(m["items"]) == 4 and not m["passed"].any() and len(m["edges"]) == 0 and len(m["node_hyp"]) == 0)
for nh in (1, 255, 256, 257):
    b = Build([(nh + 1) // 2 + 1, nh // 2 + 1])
    for k in range((nh + 1) // 2):
        b.hyp(b.seg(0, k))
    for k in range(nh // 2):
        b.hyp(b.seg(1, k))
        b.link(b.seg(0, k), b.seg(1, k))
    case("n_hyp_%d" % nh, b, "%d hypotheses: the block edge of the per-hypothesis kernels (k_aff_fill64, k_aff_node_keys, k_aff_nodes at 256 threads)" % nh,
         lambda m, t, nh=nh: len(t["hyp_dense"]) == nh and len(m["node_hyp"]) == 2 * (nh // 2) and len(m["items"]) == nh // 2)

# ---- blocks ----------------------------------------------------------------------------------------------------------------------------------------------
b = Build([46, 40])
b.all_hyp()
for i in list(range(2, 20)) + list(range(22, 44)):
    for k in range(40):
        b.link(b.seg(0, i), b.seg(1, k))
case("blocks_40_by_40", b, "40 sources x 40 passing candidates (1600 passed pairs), sources with no candidate at the start, between and at the end: with "
     "L3D_AFF_BLOCK 32 on a fresh context the pass lists are grown and kept several times from their first small size",
     lambda m, t: int(m["passed"].sum()) == 1600 and list(m["src_count"][[0, 1, 20, 21, 44, 45]]) == [0] * 6 and not m["src_count"][46:].any(),
     sets=("default", "block1", "block7", "block32", "wblock1", "wblock3", "mixed_a", "mixed_b"), fresh_context="block32")


# ---- random tables (the CPU test's few hundred; one of them with generic 3-D lines) ----------------------------------------------------------------
def random_table(seed, V=4, S=6, one_way=False, asym=False, p_hyp=0.8, p_pot=0.25, p_coll=0.25):
    rng = np.random.default_rng(seed)
    b = Build([S] * V)
    for d in range(b.nd):
        if rng.random() < p_hyp:
            b.hyp(d, "x" if rng.random() < 0.7 else "y", rng.choice([0.25, 0.5, 1.0]))
    for a in range(b.nd):
        for c in range(a + 1, b.nd):
            if b.view(a) != b.view(c):
                if rng.random() < p_pot:
                    r = rng.random()
                    if one_way and r < 0.3:
                        b.link(a, c, one_way=True) if r < 0.15 else b.link(c, a, one_way=True)
                    else:
                        b.link(a, c)
            elif rng.random() < p_coll:
                w = rng.choice([0.25, 0.5, 1.0])
                r = rng.random()
                if asym and r < 0.3:
                    b.col(a, c, w, one_way=True) if r < 0.15 else b.col(c, a, w, one_way=True)
                else:
                    b.col(a, c, w)
    if not b.hyps:
        b.hyp(0)
    return b.table()


def _real_geometry():
    t = random_table(77, V=5, S=10, one_way=True, asym=True, p_pot=0.2, p_coll=0.2)
    rng = np.random.default_rng(78)
    nh = len(t["hyp_dense"])
    # generic lines: a few bundles of nearly parallel, nearby lines (similarities strictly between 0 and 1) and strays
    base_p, base_d = rng.uniform(-1, 1, (4, 3)), rng.normal(size=(4, 3))
    for h in range(nh):
        k = int(rng.integers(0, 4))
        dd = base_d[k] + rng.normal(scale=0.03, size=3)
        dd /= np.linalg.norm(dd)
        p = base_p[k] + rng.normal(scale=0.02, size=3)
        t["hyp"][h]["P1"], t["hyp"][h]["P2"], t["hyp"][h]["dir"] = p, p + dd * rng.uniform(0.5, 1.5), dd
        t["hyp"][h]["depth_p1"], t["hyp"][h]["depth_p2"] = rng.uniform(0.8, 1.5, 2)
        t["hyp"][h]["median_depth"] = 1.2
        t["score"][h] = F32(rng.uniform(0.3, 1.0))
    t["sim"] = "device"
    return t


case("real_geometry", _real_geometry(), "about 40 hypotheses with generic 3-D lines and scores, one-way records and an asymmetric table: the only place expf matters; "
     "similarities from similarity_coll3D_batch", lambda m, t: 35 <= len(t["hyp_dense"]) <= 50 and len(m["items"]) > 40 and not m["sym"] and not m["two_way"],
     sets=BASIC + ("per_view", "block7", "mixed_a"))


# ---- invalid tables: a valid base made wrong in exactly one place ----------------------------------------------------------------------------------------
def _base():
    # (segments 4 and 9 have no list at all: a row start lowered by one behind them makes ONE thread's range descend and nothing else wrong)
    b = Build([5, 5, 4])
    b.all_hyp(skip=(3, 8, 12))
    for a, c in ((0, 6), (0, 7), (0, 10), (1, 7), (1, 11), (2, 8), (3, 10), (5, 11), (5, 12), (6, 12), (7, 13)):
        b.link(a, c)
    for a, c in ((0, 1), (1, 2), (0, 2), (5, 6), (6, 7), (10, 11), (11, 12)):
        b.col(a, c, 0.5)
    return b.table()


BASE = _base()
INVALID = {}


def copy_table(t):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def invalid(name, want, candidates, places=1):
    """the first of `candidates` ((table key, index, value) lists) after which the table check raises exactly `want` and nothing else"""
    for change in candidates:
        t = copy_table(BASE)
        for key, i, val in change:
            t[key][i] = val
        codes, message, _ = am.validate(t)
        if codes == want:
            INVALID[name] = dict(t=t, codes=codes, message=message, change=change, places=places)
            return
    raise AssertionError("no table for " + name)


def _all(key, values, lo=0, hi=None):
    n = len(BASE[key])
    return [[(key, i, v(i) if callable(v) else v)] for i in range(lo, n if hi is None else hi) for v in values]


ND, NH = int(BASE["seg_base"][-1]), len(BASE["hyp_dense"])
NPOT, NCOLL = len(BASE["pot_tgt"]), len(BASE["coll_other"])
_dv = am.dview_of(BASE)
for key, total in (("pot_start", NPOT), ("coll_start", NCOLL)):
    invalid(key + "_descends_mid_table", (1,), [[(key, i, v)] for i in range(2, ND) for v in range(int(BASE[key][i - 1]) - 1, -1, -1)])
    invalid(key + "_past_the_total", (1,), _all(key, [total + 1], 2, ND))
invalid("pot_target_out_of_range", (2,), _all("pot_tgt", [ND, ND + 1000]))
invalid("pot_target_negative", (2,), _all("pot_tgt", [-1]))
invalid("pot_target_in_own_view", (2,), [[("pot_tgt", e, x)] for e in range(NPOT - 1, -1, -1) for x in range(ND)
                                         if x > BASE["pot_tgt"][e] and _dv[x] == _dv[np.searchsorted(BASE["pot_start"], e, side="right") - 1]])
invalid("pot_target_repeated", (2,), [[("pot_tgt", e, BASE["pot_tgt"][e - 1])] for e in range(1, NPOT) if e not in BASE["pot_start"]])
invalid("pot_target_descending", (2,), [[("pot_tgt", e, BASE["pot_tgt"][e - 1] - 1)] for e in range(1, NPOT)
                                        if e not in BASE["pot_start"] and BASE["pot_tgt"][e - 1] - 1 >= 0 and _dv[BASE["pot_tgt"][e - 1] - 1] == _dv[BASE["pot_tgt"][e]]])
invalid("coll_entry_out_of_range", (3,), _all("coll_other", [ND]))
invalid("coll_entry_negative", (3,), _all("coll_other", [-1]))
invalid("coll_entry_in_another_view", (3,), [[("coll_other", q, x)] for q in range(NCOLL - 1, -1, -1) for x in range(ND - 1, -1, -1)
                                             if x > BASE["coll_other"][q] and _dv[x] != _dv[BASE["coll_other"][q]]])
invalid("coll_self_entry", (3,), [[("coll_other", q, int(np.searchsorted(BASE["coll_start"], q, side="right") - 1))] for q in range(NCOLL)])
invalid("coll_entry_repeated", (3,), [[("coll_other", q, BASE["coll_other"][q - 1])] for q in range(1, NCOLL) if q not in BASE["coll_start"]])
invalid("coll_entry_descending", (3,), [[("coll_other", q, BASE["coll_other"][q - 1] - 1)] for q in range(1, NCOLL)
                                        if q not in BASE["coll_start"] and BASE["coll_other"][q - 1] - 1 >= int(BASE["seg_base"][_dv[BASE["coll_other"][q]]])])
_free = [d for d in range(ND) if BASE["best"][d] < 0]
invalid("best_not_below_n_hyp", (4,), [[("best", d, NH)] for d in _free])
invalid("best_below_minus_one", (4,), [[("best", d, -2)] for d in _free])
invalid("best_and_hyp_dense_disagree", (4,), [[("best", d, 0)] for d in _free])
# (one hypothesis pair numbered against the dense order, consistently in both tables: two entries of each -- a single changed entry of hyp_dense also
# disagrees with best[], and which of the two findings comes back is then a race)
invalid("hyp_dense_not_ascending", (5,), [[("hyp_dense", 1, BASE["hyp_dense"][2]), ("hyp_dense", 2, BASE["hyp_dense"][1]),
                                           ("best", BASE["hyp_dense"][1], 2), ("best", BASE["hyp_dense"][2], 1)]], places=4)
invalid("pot_csr_not_starting_at_0", ("host", am.HOST_CSR0), [[("pot_start", 0, 1)]])
invalid("coll_csr_not_starting_at_0", ("host", am.HOST_CSR0), [[("coll_start", 0, 1)]])
invalid("seg_base_descends", ("host", am.HOST_ASCEND), [[("seg_base", 1, BASE["seg_base"][2] + 1)]])
invalid("view_hyp_begin_descends", ("host", am.HOST_ASCEND), [[("view_hyp_begin", 1, BASE["view_hyp_begin"][2] + 1)]])
invalid("view_hyp_begin_does_not_end_at_n_hyp", ("host", am.HOST_COVER), [[("view_hyp_begin", 3, NH + 1)]])


def no_hypotheses():
    """n_hyp = 0: the fill returns OK and empty"""
    t = copy_table(BASE)
    t["hyp"], t["score"], t["hyp_dense"] = t["hyp"][:0], t["score"][:0], t["hyp_dense"][:0]
    t["best"][:] = -1
    t["view_hyp_begin"][:] = 0
    return t


def arrays(t):
    """the tables in the order of capi.Context.affinity_fill's arguments"""
    return [t[k] for k in am.TABLE_KEYS] + [t["sigma_a"]]
