"""Crafted inputs for the slot kernels of the segment-sharded chain (l3d_chain_sharded.hip), one case per edge of the code: the ranks' ranges of worlds
that do not divide the segments (empty ranges, ranges of one), targets on both sides of every range boundary, runs around the sixteen lanes that share
one on the run-table route, slots that are empty, overflowed or not the view's to read, ring blocks around the wrap, the writer's rounds, capacities
met exactly and missed by one, and for the packers views that are unverified, empty, overflowed or not kept, batches of 1, 16 and a ragged rest.
Every case is made from those numbers, seeded, never from device output.  tests/test_shardslot_cases_cpu.py holds the cases and the models to each
other, tests/test_gpu_shard_slots.py runs them.

A writer case is a case of keptwrite_cases (the whole view's verified candidates) with the worlds it is cut into.  A collect case: views (as in
collect_cases; view k, the last, is under test), world, ring, `blocks` (view index -> the world slots' bytes, None: built from the view's kept list),
stage-1 rows.  A pack case: world, ring, views (S, N, l2g, kept, verified, ...), keep, batches, arena_cap."""
import numpy as np

import collect_cases as cc
import keptwrite_cases as kc
import keptwrite_model as km
import shardslot_model as sm

WORLDS = (1, 2, 3, 5, 8)
RUN_LENGTHS = (0, 1, 15, 16, 17, 64, 65, 300)
SCAN_STRIDE = 16 * 256            # threads over one (source, rank) list on the record route at the fewest workgroups


# ---------------------------------------------------------------------------------------------------------------- the slot writer
WRITER_CASES = {}


def _writer(case, worlds=WORLDS, **about):
    case = dict(case, worlds=tuple(worlds), about=dict(case["about"], **about))
    assert case["name"] not in WRITER_CASES
    WRITER_CASES[case["name"]] = case


_writer(kc.CASES["confidence_edges"], worlds=(1, 2, 3))                           # one segment: worlds 2 and 3 leave ranks with an empty range
_writer(kc.make("two_segments", 3, [[4, 0, 3], [2, 5, 1]], lambda y, i, m: i % 2 == 0), worlds=(1, 2, 3, 5))      # world 3: ranges of 0, 1 and 1 segments
_rng = np.random.default_rng(301)
_writer(kc.make("segments_301", 2, _rng.integers(0, 4, (301, 2)), lambda y, i, m: (y * 7 + i * 3) % 5 < 3))         # world 1: more than 256 segments in front
_writer(kc.make("second_round", 3, kc.split_rows([3, 2500, 70, 0, 2049], 3, 5), lambda y, i, m: i % 3 != 1), worlds=(1, 2, 3))
for _N in (1, 64, 65, 70):
    _r = np.full((7, _N), 2, np.int64)
    _r[3] = 0
    _r[:, 1::3] = 0
    _writer(kc.make("neighbours_%d" % _N, _N, _r, lambda y, i, m: i % 4 < 2), worlds=(1, 3))
_writer(kc.make("nothing_kept", 2, [[3, 1], [0, 2], [4, 4]], lambda y, i, m: False), worlds=(1, 2))

WRITER_MAXN = 70                  # one largest neighbour count for all writer cases: N < maxN wherever N is not 70
WRITER_VARIANTS = ("plain", "exact_fit", "one_record_short", "candidate_overflow")


def writer_geometry(case, world, side, slot_records=None):
    """side: the slot carries side words and a run table (slot_cams_min = 0), or neither (slot_cams_min above slot_records)"""
    if slot_records is None:
        slot_records = max([int(km.kept_counts(sm.sub_case(case, *sm.rank_range(case["S"], r, world))).sum()) for r in range(world)] + [1]) + 5
    return sm.geometry(case["S"] + (3 if case["N"] < WRITER_MAXN else 0), WRITER_MAXN, world, slot_records, 0 if side else slot_records + 1, 4)


def writer_settings(case, world, r, variant, side):
    """-> (geometry, cand_cap) of the variant for rank r; None: the variant needs something the rank's range does not have"""
    s0, s1 = sm.rank_range(case["S"], r, world)
    total, R = int(km.kept_counts(sm.sub_case(case, s0, s1)).sum()), int(case["row_start"][-1])
    if variant == "plain":
        return writer_geometry(case, world, side), None
    if variant == "exact_fit":
        return (writer_geometry(case, world, side, total), None) if total >= 1 else None
    if variant == "one_record_short":
        return (writer_geometry(case, world, side, total - 1), None) if total >= 2 else None
    return (writer_geometry(case, world, side), R - 1) if R > 0 else None


# ---------------------------------------------------------------------------------------------------------------- the collect step
COLLECT_CASES = {}


def _view(vid, S, l2g, tbm=(), sources=(), triples=None):
    v = cc.view(vid, S, l2g, tbm=tbm, sources=sources)
    if triples is not None:
        v["kept"] = cc.kept_list(v, triples)
    return v


def _collect(name, views, world, ring=0, blocks=None, counts=lambda y, cam: (y + cam) % 3, gap=1, slot_records=None, **about):
    k = len(views) - 1
    v = views[k]
    N = len(v["l2g"])
    rowA, metaA, depthsA, rowcnt = cc.stage1(v["S"], N, v["tbm"].tolist(), counts, gap, len(name))
    case = dict(name=name, views=views, k=k, world=world, ring=ring or len(views), blocks=blocks or {}, rowA=rowA, metaA=metaA, depthsA=depthsA, rowcnt=rowcnt,
                slot_records=slot_records, about=about)
    assert name not in COLLECT_CASES
    COLLECT_CASES[name] = case


def collect_geometry(case, side):
    views, W = case["views"], case["world"]
    most = 1
    for w in views[:case["k"]]:
        for r in range(W):
            s0, s1 = sm.rank_range(w["S"], r, W)
            most = max(most, int(((w["kept"]["segID1"] >= s0) & (w["kept"]["segID1"] < s1)).sum()))
    rec = case["slot_records"] or most + 3
    return sm.geometry(max(w["S"] for w in views), max(len(w["l2g"]) for w in views), W, rec, 0 if side else rec + 1, len(views), case["ring"])


def gathered_of(case, geom):
    """the gathered buffer as view k finds it: every earlier view's block where its exchange left it, later views over earlier ones; 0xee bytes where no
    view ever wrote"""
    block = geom["world"] * geom["slot_bytes"]
    G = np.full(geom["ring"] * block, 0xee, np.uint8)
    for j, w in enumerate(case["views"][:case["k"]]):
        make = case["blocks"].get(j)
        b = sm.view_blocks(geom, w) if make is None else make(geom, w)
        G[(j % geom["ring"]) * block:(j % geom["ring"] + 1) * block] = b
    return G


def _edges_case(world):
    """targets at s0 - 1, s0, s1 - 1 and s1 of every rank's range, from every rank's slot of the source"""
    rng = np.random.default_rng(10 + world)
    S = 23                                                    # no world but 1 divides it
    edges = sorted({min(max(e, 0), S - 1) for r in range(world) for s0, s1 in [sm.rank_range(S, r, world)] for e in (s0 - 1, s0, s1 - 1, s1)})
    src = _view(7, 17, [40, 9, 41], tbm=[0])
    t = [(y, 1, e) for e in edges for y in (0, 5 + e % 7, 16)] + [(int(rng.integers(0, 17)), 1, int(rng.integers(0, S))) for _ in range(30)] + [(3, 1, S), (4, 1, 65535)]
    src["kept"] = cc.kept_list(src, t + cc.fillers(rng, src, 40, 1))
    for i, bits in zip(np.flatnonzero(src["kept"]["camID2"] == 9)[:3], cc.SPECIAL_DEPTH_BITS):           # depths that must travel as bytes
        src["kept"]["depths"].view(np.uint32)[i, 1] = bits
    me = _view(9, S, [7, 50, 51], tbm=[1, 2], sources=[(0, 0)])
    _collect("range_edges_world_%d" % world, [src, me], world, edges=edges)


for _W in WORLDS:
    _edges_case(_W)


def _run_lengths():
    """runs of one (source segment, camera) of every length around the sixteen lanes of the run-table route; one target that collects a run of 300 reverse
    matches (ordered through the staging area) beside runs ordered in registers"""
    rng = np.random.default_rng(2)
    S = 320
    src = _view(4, 330, [70, 9, 80], tbm=[0])
    t = []
    for y, n in enumerate(RUN_LENGTHS):
        t += [(y, 1, int(s)) for s in rng.choice(S, n, replace=False)]
    t += [(y, 1, 7) for y in range(20, 320)]                  # 300 source segments aim at target 7
    t += [(y, 1, 9) for y in range(20, 50)]                   # 30 at target 9
    src["kept"] = cc.kept_list(src, t + cc.fillers(rng, src, 200, 1))
    me = _view(9, S, [4, 50], tbm=[1], sources=[(0, 0)])
    _collect("run_lengths", [src, me], 2, counts=lambda y, cam: 1 if y % 50 == 0 else 0, runs=list(RUN_LENGTHS))


_run_lengths()


def _long_slot():
    """one rank's slot of more records than one pass of the record route's threads covers"""
    rng = np.random.default_rng(3)
    S = 40
    src = _view(4, 600, [70, 9, 80, 81, 82, 83, 84, 85], tbm=[0])
    t = set()
    while len(t) < SCAN_STRIDE + 200:
        t |= {(int(a), int(b), int(c)) for a, b, c in zip(rng.integers(0, 600, 500), rng.integers(0, 8, 500), rng.integers(0, S, 500))}
    t |= {(599, 7, 1), (599, 1, S - 1)}                       # the list's last records: one for another camera, one for the view
    src["kept"] = cc.kept_list(src, sorted(t))
    me = _view(9, S, [4, 50], tbm=[1], sources=[(0, 0)])
    _collect("long_slot", [src, me], 1, records=len(src["kept"]))


_long_slot()


def _overflowed(bit, stale_count):
    """a slot as the writer leaves it when it overflows -- and behind the header the body of a good slot whose records all aim at the view: nothing of
    it may be read"""
    def make(geom, w):
        b = sm.view_blocks(geom, w)
        for r in range(geom["world"]):
            h = b[r * geom["slot_bytes"]:r * geom["slot_bytes"] + 32].view(np.int32)
            h[2] = bit
            if not stale_count:
                h[0] = 0
        return b
    return make


def _odd_sources():
    rng = np.random.default_rng(4)
    S = 12
    aimed = lambda w, cam: [(int(rng.integers(0, w["S"])), cam, int(rng.integers(0, S))) for _ in range(40)]
    empty = _view(20, 30, [77, 21], tbm=[1], triples=[])                       # verified, keeps nothing: n_kept = 0, whatever lies behind
    over1 = _view(21, 30, [77, 20], tbm=[1])
    over1["kept"] = cc.kept_list(over1, aimed(over1, 0))
    over2 = _view(22, 30, [77, 20], tbm=[1])
    over2["kept"] = cc.kept_list(over2, aimed(over2, 0))
    stranger = _view(23, 30, [20, 21], tbm=[0])                                # does not list view 77: slot -1
    stranger["kept"] = cc.kept_list(stranger, cc.fillers(rng, stranger, 40, None))
    good = _view(24, 30, [20, 77], tbm=[0])
    good["kept"] = cc.kept_list(good, aimed(good, 1) + [(3, 1, S), (4, 1, 65535)] + cc.fillers(rng, good, 30, 1))
    me = _view(77, S, [20, 21, 22, 23, 24, 600], tbm=[5], sources=[(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)])

    def stale_body(geom, w):                                                   # an empty slot over the stale body of a full one
        b = sm.view_blocks(geom, dict(w, kept=over1["kept"], l2g=over1["l2g"]))
        for r in range(geom["world"]):
            b[r * geom["slot_bytes"]:r * geom["slot_bytes"] + 32].view(np.int32)[[0, 5]] = 0
        return b
    _collect("sources_that_give_nothing", [empty, over1, over2, stranger, good, me], 3, blocks={0: stale_body, 1: _overflowed(1, True), 2: _overflowed(2, False)},
             counts=lambda y, cam: y % 4)


_odd_sources()


def _ring_wrap():
    """seven views in a ring of four blocks: the sources of view 6 are views 3 and 4, in blocks 3 and 0 -- either side of the wrap; views 0 and 2, whose
    blocks views 4 and 6 take over, aimed records at view 6 too"""
    rng = np.random.default_rng(5)
    S = 10
    views = []
    for j in range(6):
        w = _view(100 + j, 9 + j, [106, 300 + j], tbm=[1])
        w["kept"] = cc.kept_list(w, [(int(rng.integers(0, 9 + j)), 0, int(rng.integers(0, S))) for _ in range(25)] + cc.fillers(rng, w, 10, 0))
        views.append(w)
    me = _view(106, S, [103, 104, 900], tbm=[2], sources=[(0, 3), (1, 4)])
    _collect("ring_wrap", views + [me], 2, ring=4)


_ring_wrap()


def _neighbours(N):
    rng = np.random.default_rng(60 + N)
    S = 9
    if N == 1:
        return _collect("neighbours_1", [_view(5, S, [6], tbm=[0])], 2, counts=lambda y, cam: y % 3)
    w = _view(1, 20, [1000 + q for q in range(N - 1)] + [2], tbm=[0])          # the view is the source's LAST neighbour: row N - 1 (and N) of its run table
    w["kept"] = cc.kept_list(w, [(int(rng.integers(0, 20)), N - 1, int(rng.integers(0, S))) for _ in range(30)] + cc.fillers(rng, w, 60, N - 1))
    l2g = [2000 + q for q in range(N - 1)] + [1]
    _collect("neighbours_%d" % N, [w, _view(2, S, l2g, tbm=list(range(0, N - 1, max(1, N // 8))), sources=[(N - 1, 0)])], 3)


for _N in (1, 64, 65, 70):
    _neighbours(_N)


def _small_view():
    """two segments cut three ways: an empty range, two ranges of one segment"""
    src = _view(1, 5, [2, 3], tbm=[1], triples=[(0, 0, 0), (1, 0, 1), (2, 0, 0), (2, 1, 1), (4, 0, 1), (4, 0, 2)])
    _collect("two_segments_world_3", [src, _view(2, 2, [1, 8], tbm=[1], sources=[(0, 0)])], 3, counts=lambda y, cam: 2 - y)


_small_view()


def _smaller_than_the_geometry():
    """the view and its source are smaller than the largest view of the schedule: N < maxN, S < maxS, a last rank's range far below seg_cap - 1"""
    rng = np.random.default_rng(8)
    big = _view(50, 60, list(range(500, 512)), tbm=[0])
    big["kept"] = cc.kept_list(big, cc.fillers(rng, big, 50, None))
    src = _view(1, 7, [2, 3], tbm=[1])
    src["kept"] = cc.kept_list(src, [(int(rng.integers(0, 7)), 0, int(rng.integers(0, 5))) for _ in range(20)] + cc.fillers(rng, src, 8, 0))
    _collect("smaller_than_the_geometry", [big, src, _view(2, 5, [1, 8, 50], tbm=[1], sources=[(0, 1)])], 5)


_smaller_than_the_geometry()


# ---------------------------------------------------------------------------------------------------------------- the packers
PACK_CASES = {}


def _pack_views(n_views, world, seed, unverified=(), empty=(), overflowed=(), big_R=()):
    """views with short random lists; overflowed: (view, rank) slots that carry overflow bit 2 and a stale body"""
    rng = np.random.default_rng(seed)
    views = []
    for k in range(n_views):
        S, N = int(rng.integers(1, 14)), int(rng.integers(1, 5))
        v = cc.view(1000 + k, S, [2000 + 7 * k + q for q in range(N)], tbm=[0])
        n = 0 if k in empty else int(rng.integers(1, 40))
        v["kept"] = cc.kept_list(v, [(int(rng.integers(0, S)), int(rng.integers(0, N)), int(rng.integers(0, 500))) for _ in range(n)])
        v["verified"] = 0 if k in unverified else 1
        v["overflowed"] = [r for kk, r in overflowed if kk == k]
        v["big_R"] = k in big_R
        v["best"] = cc.fresh_depths(S)[:, :2].copy()
        views.append(v)
    return views


def _pack(name, world, views, ring=0, keep=None, batches=None, window=2, partition=False, short=0, tables=True, side=True):
    """batches None: the run's own schedule (capi.shard_retire) for the window; short: records the retire arena is short of holding everything kept"""
    assert name not in PACK_CASES
    PACK_CASES[name] = dict(name=name, world=world, views=views, ring=ring, keep=keep, batches=batches, window=window, partition=partition, short=short,
                            tables=tables, side=side)


def pack_inputs(case):
    """-> dict(geom, gathered, verified, keep, best_off, view_sn, rt_off, batches, arena_cap, pack_cap, best_cap, rt_cap, tables): everything
    l3d_test_shard_pack and the models take"""
    from line3d_amd import capi
    views, W = case["views"], case["world"]
    nv = len(views)
    most = 1
    for v in views:
        for r in range(W):
            s0, s1 = sm.rank_range(v["S"], r, W)
            most = max(most, int(((v["kept"]["segID1"] >= s0) & (v["kept"]["segID1"] < s1)).sum()))
    rec = most + 2
    batches, ring = case["batches"], case["ring"]
    if batches is None:
        plan = capi.shard_retire(nv, case["window"], 1, case["partition"], 0)
        batches, ring = [b[:3] for b in plan["batches"]], plan["ring"]
    geom = sm.geometry(max(v["S"] for v in views), max(len(v["l2g"]) for v in views), W, rec, 0 if case["side"] else rec + 1, nv, ring or nv)
    block = W * geom["slot_bytes"]
    G = np.full(nv * block, 0xee, np.uint8)
    for k, v in enumerate(views):
        b = sm.view_blocks(geom, v, bests=v["best"])
        for r in range(W):
            h = b[r * geom["slot_bytes"]:r * geom["slot_bytes"] + 32].view(np.int32)
            if r in v["overflowed"]:
                h[2], h[0] = 2, 0
            if v["big_R"]:
                h[1] = (1 << 30) + r
            if h[0] == 0 and geom["rt_off"]:                  # a slot without records: what lies in its run table is stale, never an offset
                o = r * geom["slot_bytes"] + geom["rt_off"]
                b[o:o + 4 * (geom["max_n"] + 1) * geom["seg_cap"]] = 0x11
        G[k * block:(k + 1) * block] = b
    verified = np.array([v["verified"] for v in views], np.uint8)
    keep = None if case["keep"] is None else np.asarray(case["keep"], np.uint8)
    view_sn = np.array([[v["S"], len(v["l2g"])] for v in views], np.int32)
    best_off = np.concatenate([[0], np.cumsum(view_sn[:, 0] + 1)])[:nv].astype(np.int64)          # (one entry of room between the views: a canary)
    here = verified.astype(bool) & (np.ones(nv, bool) if keep is None else keep.astype(bool))
    cells = np.where(here, (view_sn[:, 1] + 1) * view_sn[:, 0], 0)
    rt_off = np.concatenate([[0], np.cumsum(cells)])[:nv].astype(np.int64)
    hdrs = sm.headers_in_front(geom, G)
    per_view = sm.totals(hdrs, verified)[:, 0]
    kept_total, pack_total = int(per_view[here].sum()), int(per_view.sum())
    return dict(geom=geom, gathered=G, verified=verified, keep=keep, best_off=best_off, view_sn=view_sn, rt_off=rt_off, batches=[tuple(b) for b in batches],
                arena_cap=kept_total - case["short"], pack_cap=pack_total + 4, best_cap=int(view_sn[:, 0].sum()) + nv + 3, rt_cap=int(cells.sum()) + 5,
                tables=bool(case["tables"] and case["side"]))


_pack("one_view", 1, _pack_views(1, 1, 1), batches=[(0, 1, 1)])
_pack("world_3_batches_of_one", 3, _pack_views(6, 3, 2, unverified=(2,), empty=(4,)), batches=[(k, 1, k + 1) for k in range(6)])
_pack("world_3_overflowed_slot", 3, _pack_views(5, 3, 3, overflowed=((1, 1), (3, 0))), batches=[(0, 5, 5)])
_pack("world_8_schedule", 8, _pack_views(40, 8, 4, unverified=(0, 17, 39), empty=(5, 16)), window=3)                 # ring 21: two batches of 16 on the way, a ragged flush
_pack("world_8_keep_alternating", 8, _pack_views(40, 8, 5, unverified=(8,)), keep=[k % 2 for k in range(40)], window=3, partition=True)
_pack("world_3_keep_all", 3, _pack_views(20, 3, 6, unverified=(3,)), keep=[1] * 20, window=30, partition=True)      # a partitioned ring that never wraps
_pack("world_3_arena_exact", 3, _pack_views(20, 3, 7), window=1)
_pack("world_3_arena_one_short", 3, _pack_views(20, 3, 7), window=1, short=1)            # the last view of the last batch does not fit
_pack("world_1_tables_off", 1, _pack_views(9, 1, 8, empty=(0,)), batches=[(0, 4, 5), (4, 5, 9)], ring=5, tables=False)
_pack("world_3_no_side_words", 3, _pack_views(7, 3, 9), batches=[(0, 7, 7)], side=False)
_pack("world_3_candidates_past_2_31", 3, _pack_views(3, 3, 10, big_R=(1,)), batches=[(0, 3, 3)])
