"""The crafted cases of tests/shardslot_cases.py and the plain models of tests/shardslot_model.py held to each other and to the models of the
single-GPU chain, without a device: every path the GPU test wants to reach is reached by a case; the ranks' modelled slots, put together in rank
order, are the kept writer's whole-view answer byte for byte (the sharded chain's central claim); the ranks' modelled candidate rows, put together,
are the single-GPU collect step's; a slot's bytes parse back into its parts; the two ways of filing all views into one arena agree."""
import numpy as np
import pytest

import collect_model as cm
import keptwrite_model as km
import shardslot_cases as sc
import shardslot_model as sm

# every path of the slot kernels that the cases are built to reach (tests/test_gpu_shard_slots.py demands the same list of the device runs)
TAGS = {
    "writer: side words and run table", "writer: records only", "writer: empty range, header only", "writer: range of one segment", "writer: overflow bit 1",
    "writer: overflow bit 2", "writer: exact fit", "writer: run table of a rank other than 0", "writer: more than 256 segments in the range",
    "writer: segment of several rounds", "writer: run-table prefix over two camera chunks", "writer: fewer neighbours than the geometry's most",
    "writer: one neighbour", "writer: NaN and 1.0 are not kept",
    "source that does not list the view", "source slot with overflow bit 1", "source slot with overflow bit 2", "source slot without records",
    "record scan wraps its grid stride", "target at s0 - 1", "target at s0", "target at s1 - 1", "target at s1", "empty range", "range of one segment",
    "run of 0", "run of 1", "run of 15", "run of 16", "run of 17", "run of 64", "run of 65", "run of 300", "reverse run ordered in registers",
    "reverse run ordered through the staging area", "sources either side of the ring's wrap", "collect: world 1", "collect: world 2", "collect: world 3",
    "collect: world 5", "collect: world 8", "collect: 64 neighbours", "collect: 65 neighbours", "collect: 70 neighbours", "collect: one neighbour",
    "collect: view smaller than the geometry",
    "pack: world 1", "pack: world 3", "pack: world 8", "pack: retire tables on", "pack: retire tables off", "pack: keep absent", "pack: keep all", "pack: keep some",
    "pack: unverified view", "pack: view without records", "pack: overflowed slot among good ones", "pack: candidates clamped at 2^31 - 1", "pack: ring of all views",
    "pack: partitioned ring that never wraps", "pack: ring that wraps", "pack: batch of 1", "pack: batch of 16", "pack: ragged batch", "pack: arena fits exactly",
    "pack: arena one record short",
}


def writer_runs():
    for name, case in sc.WRITER_CASES.items():
        for world in case["worlds"]:
            for r in range(world):
                for side in (True, False):
                    for variant in sc.WRITER_VARIANTS:
                        st = sc.writer_settings(case, world, r, variant, side)
                        if st is not None:
                            yield case, world, r, side, variant, st[0], st[1]


def collect_tags(case):
    """the tags of a collect case over every rank's range (the model fills them in), and what its shape adds"""
    tags = set()
    geom = sc.collect_geometry(case, True)
    G = sc.gathered_of(case, geom)
    v = case["views"][case["k"]]
    for r in range(case["world"]):
        s0, s1 = sm.rank_range(v["S"], r, case["world"])
        m = sm.collect(case["views"], case["k"], G, geom, s0, s1, case["rowA"], case["metaA"], case["depthsA"], case["rowcnt"], tags)
        runs = [int(m["cursor"][row]) for row in m["rev_rows"]]
        if any(2 <= n <= 256 for n in runs):
            tags.add("reverse run ordered in registers")
        if any(n > 256 for n in runs):
            tags.add("reverse run ordered through the staging area")
    tags.add("collect: world %d" % case["world"])
    N = len(v["l2g"])
    if N in (64, 65, 70):
        tags.add("collect: %d neighbours" % N)
    if N == 1:
        tags.add("collect: one neighbour")
    if N < geom["max_n"] and v["S"] < geom["maxS"]:
        tags.add("collect: view smaller than the geometry")
    blocks = sorted(int(si) % geom["ring"] for si in v["source_index"])
    if len(v["source_index"]) and geom["ring"] < len(case["views"]) and 0 in blocks and geom["ring"] - 1 in blocks:
        tags.add("sources either side of the ring's wrap")
    for q, si in enumerate(v["source_index"]):         # the runs of the source's records towards the view, per source segment
        slot = sm.source_slot(case["views"], case["k"], q)
        w = case["views"][int(si)]
        if slot >= 0 and "runs" in case["about"]:
            mine = w["kept"][w["kept"]["camID2"] == v["id"]]
            for n in np.bincount(mine["segID1"].astype(np.int64), minlength=w["S"]).tolist():
                if n in sc.RUN_LENGTHS:
                    tags.add("run of %d" % n)
    return tags


def test_every_path_is_reached_by_a_case():
    reached = set()
    for case, world, r, side, variant, geom, cand_cap in writer_runs():
        reached |= sm.writer_tags(case, *sm.rank_range(case["S"], r, world), geom, cand_cap)
    for case in sc.COLLECT_CASES.values():
        reached |= collect_tags(case)
    for case in sc.PACK_CASES.values():
        reached |= sm.pack_tags(sc.pack_inputs(case))
    assert TAGS <= reached, sorted(TAGS - reached)
    assert reached <= TAGS | {"pack: ring"}, sorted(reached - TAGS)


def test_cases_stay_small():
    for case in sc.WRITER_CASES.values():
        assert case["S"] <= 600 and case["N"] <= 70 and len(case["conf"]) <= 6000, case["name"]
    for case in sc.COLLECT_CASES.values():
        assert all(w["S"] <= 600 and len(w["l2g"]) <= 70 and len(w["kept"]) <= 5000 for w in case["views"]) and len(case["views"]) <= 40, case["name"]
    for case in sc.PACK_CASES.values():
        assert len(case["views"]) <= 40 and all(len(v["kept"]) <= 5000 for v in case["views"]), case["name"]


@pytest.mark.parametrize("name", list(sc.WRITER_CASES))
def test_the_ranks_slots_in_rank_order_are_the_whole_views_list(name):
    """the product's central claim, on the models: records, side words, run table and best positions of the ranks' slots, positions shifted by the
    records in front and run-table columns side by side, are keptwrite_model.writer's of the whole view, byte for byte"""
    case = sc.WRITER_CASES[name]
    S, N = case["S"], case["N"]
    total = int(km.kept_counts(case).sum())
    whole = km.writer(case, arena_cap=total)
    for world in case["worlds"]:
        geom = sc.writer_geometry(case, world, True)
        recs, side, bpos, rt, in_front = [], [], np.zeros(S, np.int32), np.zeros((N + 1, S), np.int32), 0
        for r in range(world):
            s0, s1 = sm.rank_range(S, r, world)
            p = sm.parse_slot(geom, sm.slot_write(case, s0, s1, geom))
            h = dict(zip(sm.HEADER_KEYS, p["header"].tolist()))
            assert (h["overflow"], h["s0"], h["s1"], h["pad0"], h["R"]) == (0, s0, s1, h["n_kept"], int(case["row_start"][-1]))
            n = h["n_kept"]
            recs.append(p["records"][:n]), side.append(p["side"][:n])
            bpos[s0:s1] = np.where(p["bpos"][:s1 - s0] < 0, -1, in_front + p["bpos"][:s1 - s0])
            rt[:, s0:s1] = in_front + p["rt"][:N + 1, :s1 - s0]
            in_front += n
        assert in_front == total
        assert np.concatenate(recs).tobytes() == whole["records"].tobytes(), world
        assert np.concatenate(side).tobytes() == whole["side"].tobytes(), world
        assert bpos.tobytes() == whole["best_pos"].tobytes() and rt.tobytes() == whole["rt"].tobytes(), world
        # and without side words the same records
        plain = sc.writer_geometry(case, world, False)
        assert plain["cam_off"] == 0 and plain["rt_off"] == 0
        again = [sm.parse_slot(plain, sm.slot_write(case, *sm.rank_range(S, r, world), plain)) for r in range(world)]
        assert np.concatenate([p["records"][:p["header"][0]] for p in again]).tobytes() == whole["records"].tobytes()


def overflowed_views(case):
    geom = sc.collect_geometry(case, True)
    G = sc.gathered_of(case, geom)
    flags = [0] * len(case["views"])
    for j in range(case["k"]):
        if j + geom["ring"] >= case["k"]:
            flags[j] = int(any(sm.parse_slot(geom, sm.slot_of(geom, G, j % geom["ring"], r))["header"][2] for r in range(case["world"])))
    return flags


@pytest.mark.parametrize("name", list(sc.COLLECT_CASES))
@pytest.mark.parametrize("side", (True, False))
def test_the_ranks_rows_together_are_the_single_gpu_collect_step(name, side):
    """the union over the ranks' ranges of the modelled rows equals collect_model on the whole kept lists (an overflowed view's list: unread)"""
    case = sc.COLLECT_CASES[name]
    views, k = case["views"], case["k"]
    v = views[k]
    S, N = v["S"], len(v["l2g"])
    whole = cm.model(dict(views=views, k=k, overflowed=overflowed_views(case), rowA=case["rowA"], metaA=case["metaA"], depthsA=case["depthsA"], rowcnt=case["rowcnt"]))
    geom = sc.collect_geometry(case, side)
    G = sc.gathered_of(case, geom)
    seen = 0
    for r in range(case["world"]):
        s0, s1 = sm.rank_range(S, r, case["world"])
        m = sm.collect(views, k, G, geom, s0, s1, case["rowA"], case["metaA"], case["depthsA"], case["rowcnt"])
        a, b = int(whole["row_start"][s0 * N]), int(whole["row_start"][s1 * N])
        assert m["R"] == b - a and np.array_equal(m["row_start"][s0 * N:s1 * N + 1], whole["row_start"][s0 * N:s1 * N + 1] - a)
        assert np.array_equal(m["meta"], whole["meta"][a:b]) and np.array_equal(m["depths"], whole["depths"][a:b])
        assert np.array_equal(m["cursor"][s0 * N:s1 * N], whole["cursor"][s0 * N:s1 * N])
        assert (m["row_start"][:s0 * N] == -1).all() and (m["row_start"][s1 * N + 1:S * N] == -1).all() and (m["cursor"][:s0 * N] == -1).all()
        seen += m["R"]
    assert seen == whole["R"]


def test_a_slot_parses_back_into_its_parts():
    rng = np.random.default_rng(1)
    for side in (True, False):
        geom = sm.geometry(11, 3, 2, 9, 0 if side else 10, 4)
        assert bool(geom["cam_off"]) == side and bool(geom["rt_off"]) == side
        recs = np.frombuffer(rng.integers(0, 256, 7 * 32, dtype=np.uint8).tobytes(), sm.MATCH_DTYPE)
        best, bpos = rng.random((5, 2), dtype=np.float32), rng.integers(-1, 7, 5).astype(np.int32)
        sd, rt = rng.integers(0, 1 << 32, 7, dtype=np.uint64).astype(np.uint32), rng.integers(0, 8, (4, 5)).astype(np.int32)
        hdr = sm.header(7, 123, 0, 2, 7, 7)
        b = sm.build_slot(geom, hdr, best, bpos, recs, sd if side else None, rt if side else None)
        assert len(b) == geom["slot_bytes"] and geom["slot_bytes"] % 256 == 0
        p = sm.parse_slot(geom, b)
        assert np.array_equal(p["header"], hdr) and p["best"][:5].tobytes() == best.tobytes() and np.array_equal(p["bpos"][:5], bpos)
        assert p["records"][:7].tobytes() == recs.tobytes()
        assert (p["bpos"][5:] == sm.BESTPOS_CANARY).all() and (p["best"][5:].view(np.uint32) == 0xffffffff).all() and (p["records"][7:].view(np.uint8) == 0xff).all()
        if side:
            assert np.array_equal(p["side"][:7], sd) and np.array_equal(p["rt"][:4, :5], rt)
            assert (p["side"][7:] == 0xffffffff).all() and (p["rt"][:, 5:] == -1).all()
        else:
            assert p["side"] is None and p["rt"] is None
        covered = 32 + 5 * 8 + geom["seg_cap"] * 4 + 7 * 32 + (7 * 4 + 4 * 5 * 4 if side else 0)
        assert int((b != 0xff).sum()) <= covered


@pytest.mark.parametrize("name", list(sc.PACK_CASES))
def test_pack_all_and_retire_file_the_same_lists(name):
    """both are the verified (and kept) views' lists back to back; where every verified view is kept and fits, the two arenas are the same bytes"""
    inp = sc.pack_inputs(sc.PACK_CASES[name])
    geom, ver, keep = inp["geom"], inp["verified"], inp["keep"]
    views = sc.PACK_CASES[name]["views"]
    pa = sm.pack_all(geom, inp["gathered"], ver, inp["best_off"], inp["pack_cap"], inp["best_cap"])
    rt = sm.retire(geom, inp["gathered"], ver, keep, inp["best_off"], inp["view_sn"], inp["rt_off"], inp["batches"], inp["arena_cap"], inp["best_cap"], inp["rt_cap"],
                   inp["tables"])

    def lists(flags):
        out = [v["kept"] for k, v in enumerate(views) if flags[k] and not v["overflowed"]]
        out += [np.zeros(0, sm.MATCH_DTYPE)]
        return np.concatenate(out)
    clean = not any(v["overflowed"] for v in views)
    here = ver.astype(bool) & (np.ones(len(views), bool) if keep is None else keep.astype(bool))
    if clean:
        want = lists(ver)
        assert pa["total"] == len(want) and pa["arena"][:len(want)].tobytes() == want.tobytes()
        if not rt["overflow"]:
            want = lists(here)
            assert rt["base_dev"][sum(b[1] for b in inp["batches"])] == len(want) and rt["arena"][:len(want)].tobytes() == want.tobytes()
    if not rt["overflow"] and here.tolist() == ver.astype(bool).tolist():
        n = pa["total"]
        assert rt["arena"][:n].tobytes() == pa["arena"][:n].tobytes()
        assert rt["best"].tobytes() == pa["best"].tobytes() and rt["bestpos"].tobytes() == pa["bestpos"].tobytes()
    assert rt["overflow"] == (1 if sc.PACK_CASES[name]["short"] else 0)
    hdrs = sm.headers_in_front(geom, inp["gathered"])
    retired = sum(b[1] for b in inp["batches"])
    assert retired == len(views)
    # the compact table the retire run leaves says what the headers in front of the slots say
    assert np.array_equal(sm.totals(rt["hdr_all"], ver), sm.totals(hdrs, ver)) and np.array_equal(sm.check(rt["hdr_all"], ver), sm.check(hdrs, ver))
