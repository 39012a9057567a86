"""Crafted kept lists for the builder of matchViews' products (l3d_products.hip), one case per branch of its three build strategies.  Every case is
made from the parameters of the rule it is for (the 64 entries of a short row, the 32768 entries above which a pair is scattered in two levels, the
LDS image `cap`, the 16000 segments of the widest view, ...), seeded, never from device output.  tests/test_products_cases_cpu.py checks that each
case is what its name claims; tests/test_gpu_products_paths.py runs them on every variant of the build.

A case: name, view_ids / S (the dense map), chain (the chain views: what Context.test_products takes), rows (None or (dv0, dv1)), held (None or one
flag per chain view), expect (what the hook must report), and the numbers the CPU checks hold it to (row, entries, ...).
Lists are in (segment, local camera, target) order unless the case is about disorder."""
import numpy as np

from products_model import MATCH_DTYPE

SHORT_ROW = 64              # entries a row may have (before the duplicates go) on the short path; slot 63 of a staged row is its marker
PAIR_TWO_LEVEL = 32768      # a pair of more entries is scattered in two levels
WIDEST_VIEW = 16000         # segments of the widest view the transposed build takes
LDS_BYTES = 64 * 1024


def cap_rule(max_S):
    """the LDS image of the two-level scatter beside the block's widest view: from 12288 entries down in steps of 1024, 0 when not even 1024 fit"""
    cap = 12288
    while cap > 1024 and (max_S + 2 + 2 * cap) * 4 > LDS_BYTES:
        cap -= 1024
    return cap if (max_S + 2 + 2 * cap) * 4 <= LDS_BYTES else 0


def staging_rule(records, rows):
    """short rows are staged by the counting pass when the block's lists average at most 48 entries per row"""
    return 2 * records <= 48 * rows


def aliases(case):
    """(early-return view, the view its source's local camera number names) for every source pair whose alias is in the map"""
    out = []
    for k, v in enumerate(case["chain"]):
        if v["n_tbm"] == 0:
            out += [(v["id"], cam) for cam, si in zip(v["source_cam"], v["source_index"]) if cam in case["S"] and case["chain"][si]["n_tbm"] > 0]
    return out


def touched_views(case, x):
    """the views a row of view x can name: its chain view's neighbours, the views it is a neighbour of, the early-return aliases"""
    T = set()
    for v in case["chain"]:
        if v["n_tbm"] == 0:
            continue
        for g in v["l2g"]:
            if g in case["S"]:
                if v["id"] == x:
                    T.add(g)
                if g == x:
                    T.add(v["id"])
    for a, b in aliases(case):
        if a == x:
            T.add(b)
        if b == x:
            T.add(a)
    return T


def plan_blocks(case, budget, sort):
    """The blocks of consecutive dense views a build cuts the table into: a block takes the next view while the lists that touch it (a chain view's own
    view and its neighbours; an early-return pair's view and its alias) stay within `budget` -- records for the transposed build, two key slots per
    record for the sort (two per record of an early-return pair's source in both); its first view always.  budget 0: the builds' own (2^30, 2^28).
    -> per block: x0, x1 (views of the map), records (of its chain views' lists), rows, max_S, pairs (the (chain view, camera) pairs that target it)"""
    ids, chain = case["view_ids"], case["chain"]
    at = {vid: i for i, vid in enumerate(ids)}
    dv0, dv1 = case["rows"] or (0, len(ids))
    n_kept = [len(v["kept"]) if v["n_tbm"] > 0 else 0 for v in chain]
    touch_view, touch_src, pairs = [[] for _ in ids], [[] for _ in ids], [0] * len(ids)
    for k, v in enumerate(chain):
        if n_kept[k] == 0:
            continue
        touch_view[at[v["id"]]].append(k)
        for g in v["l2g"]:
            if g in at:
                pairs[at[g]] += 1
                if g != v["id"]:
                    touch_view[at[g]].append(k)
        if sort:                # (the sort also reads a list in the blocks of the views its records name without their being neighbours)
            touch_view_named = sorted({int(c) for c in np.unique(v["kept"]["camID2"]) if int(c) in at and int(c) not in v["l2g"]})
            for g in touch_view_named:
                touch_view[at[g]].append(k)
    src = []
    for k, v in enumerate(chain):
        if v["n_tbm"] == 0:
            src += [(k, si, at.get(cam)) for cam, si in zip(v["source_cam"], v["source_index"]) if 0 <= si < k and chain[si]["n_tbm"] > 0]
    for q, (k, si, av) in enumerate(src):
        if n_kept[si]:
            touch_src[at[chain[k]["id"]]].append(q)
            if av is not None and av != at[chain[k]["id"]]:
                touch_src[av].append(q)
    per = 2 if sort else 1
    budget = budget or ((1 << 28) if sort else (1 << 30) - 64)
    blocks, x = [], dv0
    while x < dv1:
        seen_v, seen_s, total, records, x1 = set(), set(), 0, 0, x
        while x1 < dv1:
            new_v = [k for k in dict.fromkeys(touch_view[x1]) if k not in seen_v]
            new_s = [q for q in dict.fromkeys(touch_src[x1]) if q not in seen_s]
            add = sum(per * n_kept[k] for k in new_v) + sum(2 * n_kept[src[q][1]] for q in new_s)
            if x1 > x and total + add > budget:
                break
            seen_v.update(new_v)
            seen_s.update(new_s)
            total, records, x1 = total + add, records + sum(n_kept[k] for k in new_v), x1 + 1
        S = [case["S"][ids[i]] for i in range(x, x1)]
        blocks.append(dict(x0=x, x1=x1, records=records, rows=sum(S), max_S=max([1] + S), pairs=sum(pairs[x:x1])))
        x = x1
    return blocks


def cut_budget(case, sort):
    """a budget that cuts the table between two views: the smallest sum of whole lists for which there is more than one block and a block of several
    views; where the lists leave no such cut (every list touches one view), half of all there is"""
    per = 2 if sort else 1
    sizes = [len(v["kept"]) for v in case["chain"] if v["n_tbm"] > 0]
    for j in range(1, len(sizes)):
        plan = plan_blocks(case, per * sum(sizes[:j]), sort)
        if len(plan) > 1 and any(b["x1"] - b["x0"] > 1 and b["records"] for b in plan):
            return per * sum(sizes[:j])
    return max(2, per * sum(sizes) // 2)


def _view(vid, l2g, early=False, sources=None):
    return dict(id=vid, l2g=list(l2g), early=early, sources=sources)


def make_case(name, S, chain, recs, seed, expect=None, rows=None, held=None, mutate=None, best_of=None, R=None, **info):
    """S: view id -> segments.  chain: _view entries in processing order.  recs: chain index -> (segment, local camera, target) triples.
    An early-return view's sources are the earlier chain views among its neighbours, in the order of its neighbour list (the host's rule),
    unless given.  mutate(kept lists): edits them after they were put in order.  best_of(k, S) -> (S, 2) float32: the best depth pairs, else the
    depths of the best record.  R: chain index -> candidate count (default: twice the list + 1)."""
    rng = np.random.default_rng(seed)
    index_of = {v["id"]: k for k, v in enumerate(chain)}
    kept = []
    for k, v in enumerate(chain):
        triples = sorted(set(recs.get(k, ())))
        assert not (v["early"] and triples), "an early-return view keeps nothing of its own"
        a = np.zeros(len(triples), MATCH_DTYPE)
        for i, (s, q, t) in enumerate(triples):
            a[i]["segID1"], a[i]["camID2"], a[i]["segID2"] = s, v["l2g"][q], t
        a["depths"] = rng.uniform(0.5, 9.0, (len(a), 4)).astype(np.float32)
        a["confidence"] = rng.uniform(1.0, 3.0, len(a)).astype(np.float32)
        kept.append(a)
    if mutate:
        mutate(kept)
    out = []
    for k, v in enumerate(chain):
        Sv, a = S[v["id"]], kept[k]
        bestpos = np.full(Sv, -1, np.int32)
        best = np.full((Sv, 2), -1.0, np.float32)
        for i in range(len(a)):                              # the first of the highest confidence (l3d_kept.hpp)
            s = int(a[i]["segID1"])
            if s < Sv and (bestpos[s] < 0 or a[i]["confidence"] > a[bestpos[s]]["confidence"]):
                bestpos[s] = i
        for s in range(Sv):
            if bestpos[s] >= 0:
                best[s] = a[bestpos[s]]["depths"][:2]
        if best_of is not None and not v["early"]:
            best = np.ascontiguousarray(best_of(k, Sv), np.float32).reshape(Sv, 2)
        if v["early"]:
            src = v["sources"]
            if src is None:
                src = [(q, index_of[g]) for q, g in enumerate(v["l2g"]) if g in index_of and index_of[g] < k]
            cams, idx = [c for c, _ in src], [i for _, i in src]
        else:
            cams, idx = [], []
        out.append(dict(id=v["id"], S=Sv, l2g=v["l2g"], n_tbm=0 if v["early"] else 1, source_cam=cams, source_index=idx, kept=a,
                        R=(R or {}).get(k, 2 * len(a) + 1) if not v["early"] else 0, best=best, bestpos=bestpos))
    exp = dict(build="transposed", refused=0)
    exp.update(expect or {})
    case = dict(name=name, view_ids=sorted(S), S=dict(S), chain=out, rows=rows, held=held, expect=exp)
    case.update(info)
    return case


CASES = {}


def _add(case):
    assert case["name"] not in CASES
    CASES[case["name"]] = case


# ---- short rows: row (view 0, segment 0), F towards views 20 and 21, B from their records; views 20 and 21 keep lists of their own towards view 0
def _short(name, n_f, b_from, extra_early=0, dense=False, seed=1):
    """n_f: F entries of the row, targets 0 .. n_f - 1 of view 20 then of view 21 (40 segments each); b_from: (view, segment) sources of its B column"""
    S = {0: 3, 20: 40, 21: 40, 30: 4}
    chain = [_view(0, [20, 21]), _view(20, [0]), _view(21, [0, 30])]
    recs = {0: [(0, t // 40, t % 40) for t in range(n_f)] + [(2, 0, 7)], 1: [], 2: []}
    for (w, s) in b_from:
        recs[1 if w == 20 else 2].append((s, 0, 0))
    recs[1].append((39, 0, 1))
    if extra_early:
        # view 30 returned early; its source 21 is its local camera 0, which names view 0: the records (segment 0 of 21 -> segment u of 30) put (30, u) into row (0, 0)
        chain.append(_view(30, [21], early=True))
        recs[2] += [(0, 1, u) for u in range(extra_early)]
    if dense:
        # two views that keep every pair of their 80 x 80 segments: the block's lists average more than 48 entries per row
        S.update({40: 80, 41: 80})
        chain.insert(3, _view(40, [41]))
        recs_dense = [(s, 0, t) for s in range(80) for t in range(80)]
        recs = {k if k < 3 else k + 1: v for k, v in recs.items()}
        recs[3] = recs_dense
    tot = n_f + len(b_from)
    unique = len(set([(20 + t // 40, t % 40) for t in range(n_f)]) | set(b_from))
    return make_case(name, S, chain, recs, seed, row=(0, 0), entries=tot, unique=unique, extras=extra_early, touched=3 if extra_early else 2, staged=not dense)


def _b(n, first=0):
    """n B sources: segments of view 21 from `first` up, then of view 20 from 39 down"""
    out = [(21, s) for s in range(first, min(40, first + n))]
    return out + [(20, 39 - i) for i in range(n - len(out))]


for _n in (62, 63, 64, 65):
    _add(_short("short_%d_entries" % _n, 40, _b(_n - 40, 24)))                      # 40 F + the rest B: 16 from view 21, the others from view 20, where F names them too (56 unique)
_add(_short("short_64_unique", 24, _b(40)))                                          # F: (20, 0..23); B: all of view 21: 64 unique -> not staged, recomputed by the write pass
_add(_short("short_70_entries_40_unique", 35, [(20, s) for s in range(30)] + [(20, s) for s in range(35, 40)]))
_add(_short("short_one_entry", 1, []))
_add(_short("short_f_and_b_same_target", 1, [(20, 0)]))
_add(_short("short_62_plus_2_early", 40, _b(22, 24), extra_early=2))                 # 62 + 2 = 64: still the short path, with the extras ranked in
_add(_short("short_63_plus_2_early", 40, _b(23, 24), extra_early=2))                 # 63 + 2 = 65: the bitmap, with the extras set in
_add(_short("short_63_entries_dense", 40, _b(23, 24), dense=True))
_add(_short("short_64_unique_dense", 24, _b(40), dense=True))
_add(_short("short_70_entries_40_unique_dense", 35, [(20, s) for s in range(30)] + [(20, s) for s in range(35, 40)], dense=True))


# ---- touch: view 0 keeps one match per neighbour view 1 .. n (2 segments each); every third neighbour keeps one back
def _touch(name, n, back=True, seed=2):
    S = {0: 2}
    S.update({i: 2 for i in range(1, n + 1)})
    chain = [_view(0, list(range(1, n + 1)))]
    recs = {0: [(0, q, 1) for q in range(n)] + [(1, 0, 0)]}
    for i in range(1, n + 1):
        if back and i % 3 == 0:
            recs[len(chain)] = [(0, 0, 0)]                  # (i, 0) -> (0, 0): a B entry of the row that no F entry names
            chain.append(_view(i, [0]))
    n_b = len(chain) - 1
    return make_case(name, S, chain, recs, seed, row=(0, 0), entries=n + n_b, unique=n + n_b, extras=0, touched=n, staged=True)


for _n in (63, 64, 65, 130):
    _add(_touch("touch_%d_views" % _n, _n))
_add(_touch("touch_64_views_one_entry_each", 64, back=False))                        # 64 entries from 64 views: the short path with every lane owning one view


def _target(name, St, seed=3):
    """view 1 of St segments with hits on its segment St - 1 from both sides; row (0, 0) is long (66 entries in view 2), so every touched view goes through the bitmap"""
    S = {0: 2, 1: St, 2: 70}
    chain = [_view(0, [1, 2]), _view(1, [0])]
    recs = {0: [(0, 0, St - 1), (1, 0, 0)] + [(0, 1, t) for t in range(66)], 1: [(St - 1, 0, 0), (St - 1, 0, 1), (0, 0, 1)]}
    return make_case(name, S, chain, recs, seed, row=(0, 0), entries=67 + 1, unique=67, extras=0, touched=2, staged=True, target_S=St)


for _n in (1, 31, 32, 33, 16000):
    _add(_target("target_view_of_%d_segments" % _n, _n))


# ---- two-level scatter: the pair (view 0 -> view 1) holds the entries, the pair (view 0 -> view 2) a few
def _scatter(name, S0, S1, pair, seed=4, **info):
    S = {0: S0, 1: S1, 2: 8}
    chain = [_view(0, [1, 2]), _view(2, [1])]
    recs = {0: list(pair) + [(s, 1, s % 8) for s in range(0, S0, max(1, S0 // 5))], 1: [(1, 0, S1 - 1)]}
    return make_case(name, S, chain, recs, seed, pair_entries=len(set(pair)), pair_target_S=S1, **info)


_add(_scatter("scatter_32768_entries_direct", 256, 128, [(s, 0, t) for s in range(256) for t in range(128)], two_level=False))
_add(_scatter("scatter_32769_entries_two_level", 257, 128, [(s, 0, t) for s in range(256) for t in range(128)] + [(256, 0, 0)], two_level=True))
_add(_scatter("scatter_32768_entries_cap_1024", 32, 14000, [(s, 0, (j * 13 + s) % 14000) for s in range(32) for j in range(1024)], two_level=False))
_add(_scatter("scatter_32769_entries_cap_1024", 33, 14000, [(s, 0, (j * 14 + s) % 14000) for s in range(33) for j in range(993)], two_level=True))
# one target segment with 7169 sources = the image of a block of narrow views (7168) + 1: no bucket width fits, whatever `cap` the block of this view of 8000
# sources gets (4096 beside it, 7168 when the blocks are cut so that it stands apart) -- the pair falls back to the direct scatter
_add(_scatter("scatter_busy_column_falls_back", 8000, 64, [(s, 0, 0) for s in range(cap_rule(64) + 1)] + [(s, 0, 1 + (s + i) % 63) for s in range(8000) for i in range(4)],
              two_level=False, busiest=cap_rule(64) + 1))


# ---- way out: what the transposed build refuses, the sort must still turn into the table
def _swap_adjacent(kept):
    a = kept[0]
    i = next(i for i in range(len(a) - 1) if a[i]["segID1"] == a[i + 1]["segID1"] and a[i]["camID2"] != a[i + 1]["camID2"])
    a[[i, i + 1]] = a[[i + 1, i]]


def _foreign_camera(kept):
    kept[0][len(kept[0]) // 2]["camID2"] = 3                  # view 3 is in the map, but no neighbour of view 0


def _wayout(name, S0, mutate, refused, seed=5):
    S = {0: S0, 1: 50, 2: 50, 3: 50}
    chain = [_view(0, [1, 2]), _view(1, [0, 3])]
    recs = {0: [(s, q, (3 * s + q) % 50) for s in range(0, S0, max(1, S0 // 40)) for q in (0, 1)] + [(S0 - 1, 0, 49)], 1: [(s, s % 2, s) for s in range(50)]}
    return make_case(name, S, chain, recs, seed, expect=dict(build="sorted", refused=refused), mutate=mutate)


_add(_wayout("wayout_view_of_16001_segments", WIDEST_VIEW + 1, None, 1))
_add(_wayout("wayout_adjacent_records_swapped", 60, _swap_adjacent, 2))
_add(_wayout("wayout_camera_is_no_neighbour", 60, _foreign_camera, 2))


# ---- keys / CSR: views without any entry first, in the middle and last; a map view that is only a target; records that point outside the map or past a view's end
def _keys(name, nd, seed=6):
    sizes = {0: 20, 1: 60, 2: 30, 3: nd - 200, 5: 50, 6: 10, 7: 10, 8: 20}            # views 0, 2 and 8 stay empty; views 5 and 7 are no chain views
    rng = np.random.default_rng(seed + nd)
    chain = [_view(1, [3, 5, 99]), _view(3, [1, 5]), _view(6, [7])]                  # view 99 is not in the map; the list of view 6 touches no view the others touch
    S3 = sizes[3]
    recs = {0: [], 1: [], 2: [(s, 0, (3 * s) % 10) for s in range(10)]}
    for s in range(0, 60, 2):
        recs[0] += [(s, 0, int(t)) for t in rng.choice(S3, 3, replace=False)] + [(s, 1, int(rng.integers(50))), (s, 2, 5)]
    recs[0] += [(59, 0, S3 - 1), (59, 0, S3), (59, 1, 49), (59, 1, 50), (58, 0, 0)]      # S3 and 50: target segments >= S_t
    for s in range(1, S3, 3):
        recs[1] += [(s, 0, int(rng.integers(60))), (s, 1, int(rng.integers(50)))]
    recs[1] += [(S3 - 1, 0, 59), (0, 1, 0)]
    return make_case(name, sizes, chain, recs, seed, n_dense=nd)


for _n in (255, 256, 257):
    _add(_keys("keys_n_dense_%d" % _n, _n))


# ---- early returns
def _early(name, chain, S, recs, seed=7, **info):
    return make_case(name, S, chain, recs, seed, **info)


# view 2 returns early with sources 7 and 9 (its local cameras 0 and 1): 0 names view 0 (12 segments: some of the sources' segments lie past its end), 1 names
# view 1 (in the map, no chain view).  Segment 5 of view 2 is reached by both sources (the lower rank wins) and twice by source 7 (the lower position wins).
_E2 = dict(S={0: 12, 1: 30, 2: 9, 7: 20, 9: 25},
           chain=[_view(7, [2, 9]), _view(9, [2, 7]), _view(2, [7, 9], early=True)],
           recs={0: [(3, 0, 5), (4, 0, 5), (4, 0, 6), (15, 0, 1), (19, 0, 8), (2, 1, 3), (3, 1, 24)],
                 1: [(1, 0, 5), (1, 0, 0), (11, 0, 6), (12, 0, 7), (24, 0, 8), (0, 1, 19), (5, 1, 3)]})
_add(_early("early_two_sources", _E2["chain"], _E2["S"], _E2["recs"], alias_short=True))
# three sources: local camera 0 names view 0 (a chain view), 1 names nothing (no view 1), 2 names the early-return view itself
_add(_early("early_three_sources", [_view(7, [2, 9]), _view(9, [2, 0]), _view(0, [2, 7]), _view(2, [7, 9, 0], early=True)], {0: 14, 2: 9, 7: 20, 9: 25},
            {0: [(3, 0, 5), (4, 0, 5), (15, 0, 1), (2, 1, 3)], 1: [(1, 0, 5), (11, 0, 6), (24, 0, 8), (5, 1, 3)], 2: [(0, 0, 5), (7, 0, 2), (13, 0, 8), (13, 1, 19)]}))
# source 9 is on the list of view 2 but does not have view 2 among its own neighbours (no records can point at it)
_add(_early("early_source_does_not_list_the_view", [_view(7, [2, 9]), _view(9, [7]), _view(2, [7, 9], early=True)], _E2["S"],
            {0: _E2["recs"][0], 1: [(0, 0, 19), (5, 0, 3)]}, unlisted_source=1))
# two early-return views at the end of a chain, the second a source-less one (its neighbours are not chain views)
_add(_early("early_two_views_one_without_sources", _E2["chain"] + [_view(0, [1], early=True)], _E2["S"], _E2["recs"]))


# ---- medians: views of 1, 255, 256, 257 and 1000 segments
MEDIAN_SIZES = (1, 255, 256, 257, 1000)


def _median(name, pattern, seed=8, R=None):
    S = {i: n for i, n in enumerate(MEDIAN_SIZES)}
    S[9] = 4
    chain = [_view(i, [9]) for i in range(len(MEDIAN_SIZES))]
    recs = {i: [(0, 0, i % 4), (MEDIAN_SIZES[i] - 1, 0, 3)] for i in range(len(MEDIAN_SIZES))}

    def best_of(k, Sv):
        rng = np.random.default_rng(1000 * seed + k)
        b = np.asarray(pattern(rng, Sv), np.float32).reshape(Sv, 2)
        return b
    return make_case(name, S, chain, recs, seed, best_of=best_of, R=R)


def _with_gaps(rng, b):
    """every sixth segment has no best hypothesis (the sentinel: x == -1); its y is read by nobody"""
    b = np.array(b, np.float32)
    if len(b) > 2:
        b[::6] = (-1.0, 7.0)
    return b


_add(_median("median_all_depths_equal", lambda rng, n: _with_gaps(rng, np.full((n, 2), 2.5))))
_add(_median("median_half_negative", lambda rng, n: _with_gaps(rng, rng.normal(0.0, 3.0, (n, 2)))))
_add(_median("median_signed_zeros", lambda rng, n: _with_gaps(rng, rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.5, 2.0], np.float32), (n, 2)))))
_add(_median("median_subnormal_and_huge", lambda rng, n: _with_gaps(rng, rng.choice(np.array([1e-42, -1e-42, 1e30, -1e30, 1e-45, 3.0], np.float32), (n, 2)))))
_add(_median("median_ties_across_the_rank", lambda rng, n: _with_gaps(rng, np.where(rng.random((n, 2)) < 0.6, 4.25, rng.normal(4.25, 1.0, (n, 2))))))
_add(_median("median_y_is_minus_one", lambda rng, n: np.stack([rng.uniform(1, 2, n), np.full(n, -1.0)], axis=1)))       # y == -1 is a depth like any other
_add(_median("median_no_best_anywhere", lambda rng, n: np.full((n, 2), -1.0)))
_add(_median("median_no_candidates", lambda rng, n: rng.uniform(1, 2, (n, 2)), R={i: 0 for i in range(len(MEDIAN_SIZES))}))


# ---- partial builds: the rows of a range of dense views, numbered from 0; with `held` the rows outside it empty
def _partial(name, rows, held, seed=9):
    S = {0: 7, 1: 33, 2: 64, 3: 5, 4: 65, 5: 20}
    ids = sorted(S)
    rng = np.random.default_rng(seed)
    chain = [_view(i, [j for j in ids if j != i and abs(j - i) <= 2]) for i in ids]
    recs = {}
    for k, v in enumerate(chain):
        recs[k] = [(int(rng.integers(S[v["id"]])), q, int(rng.integers(S[g]))) for q, g in enumerate(v["l2g"]) for _ in range(3 * S[v["id"]])]
    flags = None
    if held:
        flags = [1 if rows[0] - 2 <= i < rows[1] + 2 else 0 for i in range(len(ids))]
    return make_case(name, S, chain, recs, seed, rows=rows, held=flags)


for _nm, _rows in (("first", (0, 2)), ("middle", (2, 4)), ("last", (4, 6)), ("empty", (3, 3))):
    _add(_partial("partial_%s_rows" % _nm, _rows, False))
    _add(_partial("partial_%s_rows_held" % _nm, _rows, True))
