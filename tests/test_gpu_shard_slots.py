"""The slot kernels of the segment-sharded chain (k_slot_write; k_exist_count_slots, the range scan and k_place_slots; k_pack_view, k_shard_totals,
k_check_slots, k_shard_pack_all, k_shard_retire) through l3d_test_shard_slot_write, l3d_test_shard_collect and l3d_test_shard_pack on the crafted
cases of tests/shardslot_cases.py against the plain models of tests/shardslot_model.py.  Everything compared is an integer or a copied float: bytes,
no tolerance anywhere.  Every output comes back whole over a fill of 0xff bytes, so a stray write shows as a broken canary.

One thing is not compared byte for byte: the order of the segments inside one bin of seg_order is the order of the scan's atomics; the bins, the
permutation and the untouched entries behind the range are held."""
import numpy as np
import pytest

import keptwrite_model as km
import shardslot_cases as sc
import shardslot_model as sm
from line3d_amd import capi
from test_shardslot_cases_cpu import TAGS, collect_tags

pytestmark = pytest.mark.gpu

SLACK = 8
_REACHED = set()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def call(what, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except capi.L3DError as e:          # a failing device call leaves nothing to compare, and nothing more is started on the device
        pytest.exit("%s: %s" % (what, e), 1)


def first_difference(got, want):
    d = np.flatnonzero(np.asarray(got).reshape(-1).view(np.uint8) != np.asarray(want).reshape(-1).view(np.uint8))
    return "first at byte %d of %d: %s / %s" % (d[0], len(d), np.asarray(got).reshape(-1).view(np.uint8)[d[0]:d[0] + 8], np.asarray(want).reshape(-1).view(np.uint8)[d[0]:d[0] + 8])


# ---------------------------------------------------------------------------------------------------------------- the slot writer
def write_slot(ctx, case, s0, s1, geom, cand_cap=None, what=""):
    return call(what, ctx.test_shard_slot_write, case["N"], case["row_start"], case["meta"], case["depths"], case["conf"], km.kept_counts(case), case["l2g"],
                sm.best_pairs(case), s0, s1, geom, cand_cap=cand_cap)


@pytest.mark.parametrize("name", list(sc.WRITER_CASES))
def test_slot_writer_on_every_world_rank_and_geometry(ctx, name):
    case = sc.WRITER_CASES[name]
    failures, ran = [], 0
    for world in case["worlds"]:
        for r in range(world):
            s0, s1 = sm.rank_range(case["S"], r, world)
            for side in (True, False):
                for variant in sc.WRITER_VARIANTS:
                    st = sc.writer_settings(case, world, r, variant, side)
                    if st is None:
                        continue
                    geom, cand_cap = st
                    what = "%s, world %d, rank %d, %s, %s" % (name, world, r, "side words" if side else "records only", variant)
                    got = write_slot(ctx, case, s0, s1, geom, cand_cap, what)
                    want = sm.slot_write(case, s0, s1, geom, cand_cap)
                    ran += 1
                    if got.tobytes() != want.tobytes():
                        failures.append("%s: %s" % (what, first_difference(got, want)))
                    else:
                        _REACHED.update(sm.writer_tags(case, s0, s1, geom, cand_cap))
    assert ran >= sum(case["worlds"]) * 2 and not failures, "\n".join(failures[:10])


# ---------------------------------------------------------------------------------------------------------------- the collect step
def run_collect(ctx, case, geom, G, s0, s1, sort_apart, views=None, what=""):
    views = case["views"] if views is None else views
    m = sm.collect(views, case["k"], G, geom, s0, s1, case["rowA"], case["metaA"], case["depthsA"], case["rowcnt"])
    out = call(what, ctx.test_shard_collect, views, case["k"], G, geom, s0, s1, case["rowA"], case["metaA"], case["depthsA"], case["rowcnt"], m["R"] + SLACK,
               sort_apart=sort_apart)
    return out, m


def check_collect(case, geom, s0, s1, sort_apart, out, m):
    v = case["views"][case["k"]]
    bad = []
    wps = max(1, min(256, (geom["seg_cap"] * 16 + 255) // 256)) if geom["rt_off"] else max(16, min(256, geom["slot_records"] // 4096))
    if (out["wps"], out["blocks_move"]) != (wps, ((s1 - s0) * len(v["tbm"]) + 3) // 4):
        bad.append("%d workgroups per list, %d move blocks" % (out["wps"], out["blocks_move"]))
    if out["R"] != m["R"] or out["row_start"].tobytes() != m["row_start"].tobytes():
        bad.append("row starts differ (R %d, model %d)" % (out["R"], m["R"]))
    if out["cursor"].tobytes() != m["cursor"].tobytes():
        bad.append("cursors differ: a cursor is its row's count of reverse matches, -1 outside the range")
    if not sm.seg_order_ok(out["seg_order"], s0, s1, m["seg_sizes"]):
        bad.append("seg_order is not the range's segments in bins that never decrease, untouched behind them")
    R = m["R"]
    meta, dep = out["cand_meta"], out["cand_depths"].view(np.uint32)
    if not ((meta[R:] == 0xffffffff).all() and (dep[R:] == 0xffffffff).all()):
        bad.append("slots behind R were written")
    meta, dep = meta[:R].copy(), dep[:R].copy()
    if not sort_apart:                  # the scatter's order inside a run is the atomics': compared as a multiset, by target (targets are distinct inside a run)
        for row in m["rev_rows"]:
            a, b = int(m["row_start"][row]), int(m["row_start"][row + 1])
            o = np.argsort(meta[a:b, 0], kind="stable")
            meta[a:b], dep[a:b] = meta[a:b][o], dep[a:b][o]
    if not np.array_equal(meta, m["meta"]) or not np.array_equal(dep, m["depths"]):
        d = np.flatnonzero((meta != m["meta"]).any(1) | (dep != m["depths"]).any(1))
        bad.append("%d candidates differ, first at %d: %s %s / %s %s" % (len(d), d[0], meta[d[0]], dep[d[0]], m["meta"][d[0]], m["depths"][d[0]]))
    return bad


@pytest.mark.parametrize("name", list(sc.COLLECT_CASES))
def test_collect_on_every_rank_geometry_and_order(ctx, name):
    case = sc.COLLECT_CASES[name]
    v = case["views"][case["k"]]
    failures = []
    for r in range(case["world"]):
        s0, s1 = sm.rank_range(v["S"], r, case["world"])
        sorted_out = {}
        for side in (True, False):
            geom = sc.collect_geometry(case, side)
            G = sc.gathered_of(case, geom)
            for sort_apart in (0, 1):
                what = "%s, rank %d, %s, sort_apart %d" % (name, r, "run tables" if side else "records", sort_apart)
                out, m = run_collect(ctx, case, geom, G, s0, s1, sort_apart, what=what)
                bad = check_collect(case, geom, s0, s1, sort_apart, out, m)
                if sort_apart:
                    sorted_out[side] = out
                if bad:
                    failures.append("%s: %s" % (what, "; ".join(bad)))
        # the two routes on the same case: the same bytes once the runs are ordered
        a, b = sorted_out[True], sorted_out[False]
        if any(a[key].tobytes() != b[key].tobytes() for key in ("row_start", "cursor", "cand_meta", "cand_depths")):
            failures.append("%s, rank %d: the run-table route and the record route differ" % (name, r))
    assert not failures, "\n".join(failures[:10])
    _REACHED.update(collect_tags(case))


# ---------------------------------------------------------------------------------------------------------------- the packers
def run_pack(ctx, inp, what=""):
    return call(what, ctx.test_shard_pack, inp["gathered"], inp["geom"], inp["verified"], inp["best_off"], inp["view_sn"], inp["batches"], inp["arena_cap"],
                inp["pack_cap"], inp["best_cap"], keep=inp["keep"], rt_off=inp["rt_off"], rt_cap=inp["rt_cap"], retire_tables=int(inp["tables"]))


def check_pack(inp, out):
    geom, G, ver = inp["geom"], inp["gathered"], inp["verified"]
    nv = geom["n_views"]
    bad = []

    def same(what, got, want):
        if np.ascontiguousarray(got).tobytes() != np.ascontiguousarray(want).tobytes():
            bad.append("%s differs, %s" % (what, first_difference(got, want)))
    hdrs = sm.headers_in_front(geom, G)
    rt = sm.retire(geom, G, ver, inp["keep"], inp["best_off"], inp["view_sn"], inp["rt_off"], inp["batches"], inp["arena_cap"], inp["best_cap"], inp["rt_cap"], inp["tables"])
    pa = sm.pack_all(geom, G, ver, inp["best_off"], inp["pack_cap"], inp["best_cap"])
    for k in range(nv):
        stage, hdr = sm.pack_view(geom, G, k) if ver[k] else (np.full(geom["stage_bytes"], 0xff, np.uint8), np.full(32, 0xff, np.uint8))
        same("view %d: staging buffer" % k, out["stage"][k], stage)
        same("view %d: pack header" % k, out["pack_hdr"][k], hdr)
    same("totals, headers in front of the slots", out["totals"][0], sm.totals(hdrs, ver))
    same("totals, compact table", out["totals"][1], sm.totals(rt["hdr_all"], ver))
    same("check words, headers in front of the slots", out["check"][0], sm.check(hdrs, ver))
    same("check words, compact table", out["check"][1], sm.check(rt["hdr_all"], ver))
    same("pack-all arena", out["pa_arena"], pa["arena"])
    same("pack-all best pairs", out["pa_best"], pa["best"])
    same("pack-all best positions", out["pa_bestpos"], pa["bestpos"])
    same("retire arena", out["rt_arena"], rt["arena"])
    same("retire best pairs", out["rt_best"], rt["best"])
    same("retire best positions", out["rt_bestpos"], rt["bestpos"])
    same("base_dev", out["base_dev"], rt["base_dev"])
    same("hdr_all", out["hdr_all"], rt["hdr_all"])
    same("side words of the retired records", out["qt_arena"], rt["qt"])
    same("run tables of the retired views", out["rt_all"], rt["rt_all"])
    if out["overflow"] != rt["overflow"]:
        bad.append("arena overflow flag %d, model %d" % (out["overflow"], rt["overflow"]))
    here = ver.astype(bool) & (np.ones(nv, bool) if inp["keep"] is None else inp["keep"].astype(bool))
    if not rt["overflow"] and here.tolist() == ver.astype(bool).tolist():       # the two runs against each other
        n = pa["total"]
        same("the retire arena against the pack-all arena", out["rt_arena"][:n], out["pa_arena"][:n])
        same("the retire best positions against pack-all's", out["rt_bestpos"], out["pa_bestpos"])
    return bad


@pytest.mark.parametrize("name", list(sc.PACK_CASES))
def test_packers(ctx, name):
    inp = sc.pack_inputs(sc.PACK_CASES[name])
    bad = check_pack(inp, run_pack(ctx, inp, name))
    assert not bad, "\n".join(bad[:10])
    _REACHED.update(sm.pack_tags(inp))


# ---------------------------------------------------------------------------------------------------------------- writer feeds reader
def test_slots_written_on_the_device_feed_the_readers(ctx):
    """the slot writer's own bytes, three ranks of one view, handed to the collect step of a later view and to the packers: the model's answers again --
    the model's idea of a slot is the kernel's"""
    src = sc.WRITER_CASES["two_segments"]
    world, S, N = 3, src["S"], src["N"]
    geom = sm.geometry(40, 3, world, 12, 0, 2)
    device = np.concatenate([write_slot(ctx, src, *sm.rank_range(S, r, world), geom, what="writer, rank %d" % r) for r in range(world)])
    model = np.concatenate([sm.slot_write(src, *sm.rank_range(S, r, world), geom) for r in range(world)])
    assert device.tobytes() == model.tobytes()
    assert sum(int(sm.parse_slot(geom, sm.slot_of(geom, device, 0, r))["header"][0]) for r in range(world)) == int(km.kept_counts(src).sum()) > 0
    # view 1 is the source's local camera 1; the source's targets are segments of view 1
    import collect_cases as cc
    me_id = int(src["l2g"][1])
    v0 = cc.view(500, S, src["l2g"], tbm=[0])
    v1 = cc.view(me_id, 40, [500, 77], tbm=[1], sources=[(0, 0)])
    rowA, metaA, depthsA, rowcnt = cc.stage1(40, 2, [1], lambda y, cam: y % 2, 1, 3)
    case = dict(views=[v0, v1], k=1, world=world, rowA=rowA, metaA=metaA, depthsA=depthsA, rowcnt=rowcnt)
    G = np.concatenate([device, np.full(len(device), 0xee, np.uint8)])
    total = 0
    for r in range(world):
        s0, s1 = sm.rank_range(40, r, world)
        for sort_apart in (0, 1):
            out, m = run_collect(ctx, case, geom, G, s0, s1, sort_apart, what="reader, rank %d" % r)
            bad = check_collect(case, geom, s0, s1, sort_apart, out, m)
            assert not bad, bad
        total += len(m["rev_rows"])
    assert total > 0
    # ... and the packers over the same block
    inp = dict(geom=sm.geometry(40, 3, world, 12, 0, 1), gathered=device, verified=np.ones(1, np.uint8), keep=None, best_off=np.zeros(1, np.int64),
               view_sn=np.array([[S, N]], np.int32), rt_off=np.zeros(1, np.int64), batches=[(0, 1, 1)], arena_cap=12, pack_cap=12, best_cap=S + 2,
               rt_cap=(N + 1) * S + 2, tables=True)
    out = run_pack(ctx, inp, "packers over device-written slots")
    bad = check_pack(inp, out)
    assert not bad, bad
    whole = km.writer(src, arena_cap=12)                # the whole view's list, as the single-GPU writer leaves it
    assert out["rt_arena"].tobytes() == whole["records"].tobytes() and out["qt_arena"].tobytes() == whole["side"].tobytes()
    assert out["rt_all"][:(N + 1) * S].tobytes() == whole["rt"].tobytes() and out["rt_bestpos"][:S].tobytes() == whole["best_pos"].tobytes()
    _REACHED.add("writer feeds reader")


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(fn, *a, **kw):
    with pytest.raises(capi.L3DError):
        fn(*a, **kw)


def test_the_slot_writer_refuses_before_launch(ctx):
    case = sc.WRITER_CASES["two_segments"]
    S, N = case["S"], case["N"]
    geom = sc.writer_geometry(case, 2, True)
    args = lambda c=case, s0=0, s1=1, g=geom, **kw: ([c["N"], kw.get("row_start", c["row_start"]), kw.get("meta", c["meta"]), c["depths"], c["conf"],
                                                        kw.get("kept", km.kept_counts(c)), c["l2g"], sm.best_pairs(c), s0, s1, g])
    wide = dict(case, N=256, l2g=np.arange(256, dtype=np.uint32), row_start=np.zeros(S * 256 + 1, np.int32), meta=case["meta"][:0], depths=case["depths"][:0], conf=case["conf"][:0])
    refused(ctx.test_shard_slot_write, *args(wide))                                        # N outside [1, 255]
    rs = case["row_start"].copy(); rs[0] = 1
    refused(ctx.test_shard_slot_write, *args(row_start=rs))                                # row_start does not start at 0
    rs = case["row_start"].copy(); rs[2] = rs[3] + 1
    refused(ctx.test_shard_slot_write, *args(row_start=rs))                                # ... does not ascend
    meta = case["meta"].copy(); meta[0, 1] = 1
    refused(ctx.test_shard_slot_write, *args(meta=meta))                                   # a candidate whose camera is not its row's
    meta = case["meta"].copy(); meta[0, 0] = 65536
    refused(ctx.test_shard_slot_write, *args(meta=meta))                                   # a target that does not fit 16 bits
    kept = km.kept_counts(case); kept[0] += 1
    refused(ctx.test_shard_slot_write, *args(kept=kept))                                   # kept_cnt that is not the count
    refused(ctx.test_shard_slot_write, *args(s0=1, s1=S + 1))                              # a range outside [0, S]
    refused(ctx.test_shard_slot_write, *args(s0=1, s1=0))
    refused(ctx.test_shard_slot_write, *args(s0=0, s1=S, g=sm.geometry(S, sm_maxn(case), 4, 9, 0, 4)))    # a range longer than seg_cap - 1
    refused(ctx.test_shard_slot_write, *args(g=sm.geometry(S, N - 1, 2, 9, 0, 4)))         # N > maxN
    refused(ctx.test_shard_slot_write, *args(g=sm.geometry(S - 1, N, 1, 9, 0, 4)))         # S > maxS
    _REACHED.add("writer refusals")


def sm_maxn(case):
    return max(case["N"], 3)


def test_the_collect_hook_refuses_before_launch(ctx):
    case = sc.COLLECT_CASES["range_edges_world_2"]
    geom = sc.collect_geometry(case, True)
    G = sc.gathered_of(case, geom)
    v = case["views"][1]
    s0, s1 = sm.rank_range(v["S"], 1, 2)
    S_src = case["views"][0]["S"]
    a0, a1 = sm.rank_range(S_src, 0, 2)

    def go(G=G, geom=geom, views=case["views"], s0=s0, s1=s1, cand_cap=4000):
        return ctx.test_shard_collect(views, len(views) - 1, G, geom, s0, s1, case["rowA"], case["metaA"], case["depthsA"], case["rowcnt"], cand_cap)

    def broken(edit, geom=geom, G=G):
        B = G.copy()
        edit(sm.parse_slot(geom, sm.slot_of(geom, B, 0, 0)))
        return B

    def set_(name, i, value):
        def edit(p):
            p[name][i] = value
        return edit
    go()                                                                                   # (the case itself passes)
    refused(go, G=broken(set_("header", 0, geom["slot_records"] + 1)))                      # n_kept outside [0, slot_records]
    refused(go, G=broken(set_("header", 0, -1)))
    refused(go, G=broken(set_("header", 3, a1 + 1)))                                       # s0 > s1
    refused(go, G=broken(set_("header", 4, a0 + geom["seg_cap"])))                         # s1 - s0 > seg_cap - 1

    recs = sm.parse_slot(geom, sm.slot_of(geom, G, 0, 0))["records"]
    i = next(i for i in range(1, 20) if (int(recs["segID1"][i]), int(recs["camID2"][i])) != (int(recs["segID1"][i - 1]), int(recs["camID2"][i - 1])))

    def swap(p):
        p["records"][[i - 1, i]] = p["records"][[i, i - 1]]
        p["side"][[i - 1, i]] = p["side"][[i, i - 1]]
    refused(go, G=broken(swap))                                                            # records out of (segment, camera) order

    def outside(p):
        p["records"]["segID1"][0] = a1
    refused(go, G=broken(outside))                                                         # a segment outside the header's range

    def stranger(p):
        p["records"]["camID2"][0] = 999999
    refused(go, G=broken(stranger))                                                        # a camera that is no neighbour
    refused(go, G=broken(set_("side", 0, 0xffffffff)))                                     # a side word that is not its record's
    refused(go, G=broken(lambda p: p["rt"].__setitem__((1, 0), int(p["rt"][1, 0]) + 1)))   # a run-table entry that is not consistent with the records
    refused(go, G=broken(lambda p: p["rt"].__setitem__((3, a1 - a0 - 1), -1)))             # ... in the row behind the last camera
    refused(go, s0=0, s1=v["S"])                                                           # a range longer than seg_cap - 1
    refused(go, cand_cap=3)                                                                # no room for the range's candidates
    # the overflowed slot's body is not looked at
    over = broken(lambda p: (p["header"].__setitem__(2, 2), p["records"]["camID2"].__setitem__(0, 999999)))
    go(G=over)
    # two sources whose indices differ by exactly the ring: the earlier one's block is overwritten
    ring = sc.COLLECT_CASES["ring_wrap"]
    views = [dict(w) for w in ring["views"]]
    views[6] = dict(views[6], l2g=np.array([101, 105, 900], np.uint32), source_index=np.array([1, 5], np.int32))
    for j in (1, 5):
        views[j] = dict(views[j], l2g=np.array([106, 300 + j], np.uint32))
    g4 = sc.collect_geometry(ring, True)
    refused(ctx.test_shard_collect, views, 6, sc.gathered_of(ring, g4), g4, 0, 5, ring["rowA"], ring["metaA"], ring["depthsA"], ring["rowcnt"], 4000)
    _REACHED.add("collect refusals")


def test_the_pack_hook_refuses_before_launch(ctx):
    inp = sc.pack_inputs(sc.PACK_CASES["world_1_tables_off"])             # nine views in a ring of five blocks
    run = lambda **kw: run_pack_raw(ctx, dict(inp, **kw))
    run()
    refused(run, batches=[(0, 4, 5), (5, 4, 9)])                          # not contiguous
    refused(run, batches=[(4, 5, 9), (0, 4, 9)])                          # not ascending from view 0
    refused(run, batches=[(0, 4, 3), (4, 5, 9)])                          # retires a view that is not exchanged yet
    refused(run, batches=[(0, 4, 6), (4, 5, 9)])                          # view 5 has overwritten the block of view 0
    refused(run, pack_cap=inp["pack_cap"] - 5)                            # the verified views keep more
    refused(run, verified=np.full(9, 2, np.uint8))
    refused(run, best_cap=3)
    G = inp["gathered"].copy()
    sm.parse_slot(inp["geom"], sm.slot_of(inp["geom"], G, 1, 0))["header"][0] = inp["geom"]["slot_records"] + 1
    refused(run, gathered=G)                                              # n_kept outside [0, slot_records]
    G = inp["gathered"].copy()
    sm.parse_slot(inp["geom"], sm.slot_of(inp["geom"], G, 1, 0))["header"][4] = int(inp["view_sn"][1][0]) + 1
    refused(run, gathered=G)                                              # a range past the view's segments
    refused(run, rt_cap=1, tables=True)                                   # a view's run table ends past rt_cap
    refused(run_pack_raw, ctx, dict(sc.pack_inputs(sc.PACK_CASES["world_3_no_side_words"]), tables=True))      # retire tables without side words in the slots
    _REACHED.add("pack refusals")


def run_pack_raw(ctx, inp):
    return ctx.test_shard_pack(inp["gathered"], inp["geom"], inp["verified"], inp["best_off"], inp["view_sn"], inp["batches"], inp["arena_cap"], inp["pack_cap"],
                               inp["best_cap"], keep=inp["keep"], rt_off=inp["rt_off"], rt_cap=inp["rt_cap"], retire_tables=int(inp["tables"]))


def test_every_path_was_reached_on_the_device():
    want = TAGS | {"writer feeds reader", "writer refusals", "collect refusals", "pack refusals"}
    assert want <= _REACHED, sorted(want - _REACHED)
