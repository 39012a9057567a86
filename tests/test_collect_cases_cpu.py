"""The crafted cases of tests/collect_cases.py against the numbers they are made for, and tests/collect_model.py against a second, slower count -- no
device.  (The host rule for the lanes per run is held to its table in tests/test_keptwrite_cases_cpu.py; the mirror used by the device tests is held
to the library's here.)"""
import numpy as np

import collect_cases as cc
import collect_model as cm


def runs_of(case):
    m = cm.model(case)
    return [int(m["cursor"][r]) for r in m["rev_rows"]], m


def test_preconditions_hold_for_every_case():
    for name, case in cc.CASES.items():
        cc.check_preconditions(case)            # sources and cameras to be matched disjoint, sources earlier, lists ordered, targets distinct inside a run
        v = case["views"][case["k"]]
        S, N = v["S"], len(v["l2g"])
        assert case["k"] == len(case["views"]) - 1 and case["rowA"].shape == case["rowcnt"].shape == (S * N,), name
        tbm = set(v["tbm"].tolist())
        for row in range(S * N):
            if row % N in tbm:
                a, n = case["rowA"][row], case["rowcnt"][row]
                assert 0 <= a and a + n <= len(case["metaA"]) and (case["metaA"][a:a + n, 1] == row % N).all(), (name, row)
            else:
                assert case["rowcnt"][row] == 0, (name, row)
        bits = np.concatenate([w["kept"]["depths"].view(np.uint32).reshape(-1) for w in case["views"]] + [case["depthsA"].view(np.uint32).reshape(-1)])
        assert len(np.unique(bits)) == len(bits), name                         # every depth its own bit pattern


def test_model_against_a_plain_count():
    for name, case in cc.CASES.items():
        m = cm.model(case)
        v = case["views"][case["k"]]
        S, N = v["S"], len(v["l2g"])
        want = case["rowcnt"].astype(np.int64).copy()
        for cam, si in zip(v["source_cam"], v["source_index"]):
            w = case["views"][si]
            if w["n_tbm"] == 0 or (case["overflowed"] is not None and case["overflowed"][si]):
                continue
            for r in w["kept"]:
                if r["camID2"] == v["id"] and r["segID2"] < S:
                    want[int(r["segID2"]) * N + cam] += 1
        assert np.array_equal(np.diff(m["row_start"]), want) and m["R"] == want.sum(), name
        for row in m["rev_rows"]:
            a, b = m["row_start"][row], m["row_start"][row + 1]
            assert (np.diff(m["meta"][a:b, 0].astype(np.int64)) > 0).all() and (m["meta"][a:b, 1] == row % N).all(), (name, row)
        assert cm.seg_order_ok(np.argsort(-m["seg_sizes"], kind="stable"), m["seg_sizes"]) or S == 0
        if S > 1 and m["seg_sizes"].max() >= 32 + m["seg_sizes"].min():
            assert not cm.seg_order_ok(np.argsort(m["seg_sizes"], kind="stable"), m["seg_sizes"]), name


def test_cases_hold_the_numbers_they_are_for():
    C = cc.CASES
    runs, m = runs_of(C["run_lengths"])
    assert sorted(runs + [0]) == sorted(list(cc.RUN_LENGTHS) + [1]) == sorted(C["run_lengths"]["about"]["runs"])
    src = C["run_lengths"]["views"][0]["kept"]
    aimed = src[src["camID2"] == 9]
    assert (aimed["segID2"] >= C["run_lengths"]["views"][1]["S"]).sum() == 1              # one record past the view's segments: dropped
    assert set(cc.SPECIAL_DEPTH_BITS) <= set(aimed["depths"].view(np.uint32).reshape(-1).tolist())
    c = C["run_lengths"]
    rc = c["rowcnt"].reshape(-1, 4)[:, 1].tolist()
    assert rc[:4] == [0, 1, 64, 65]                                                       # stage-1 rows of 0, 1, 64, 65 entries
    starts = np.sort(c["rowA"][c["rowcnt"] > 0])
    assert (c["metaA"][:, 0] == 0xdeadbeef).sum() >= 3 * 20                               # gaps between the rows
    c = C["source_segment_counts"]
    assert [w["S"] for w in c["views"][:5]] == [1, 5, 16, 17, 100] == c["about"]["source_S"] and c["views"][5]["S"] == 40
    for w in c["views"][:5]:                                                               # the first and the last chunk of every source hold records aimed at the view
        mine = w["kept"][w["kept"]["camID2"] == 99]
        assert 0 in mine["segID1"] and w["S"] - 1 in mine["segID1"]
    c = C["largest_view"]
    _, m = runs_of(c)
    assert c["views"][1]["S"] == 16384 and {r // 2 for r in m["rev_rows"]} == {0, 8000, 16383}
    c = C["sources_that_give_nothing"]
    v = c["views"][5]
    kinds = [(len(w["kept"]), w["n_tbm"], 77 in w["l2g"].tolist(), bool(c["overflowed"][i])) for i, w in enumerate(c["views"][:5])]
    assert kinds[0] == (0, 1, True, False) and kinds[1][:2] == (0, 0) and kinds[2][0] > 0 and kinds[2][3] and kinds[3][0] > 0 and not kinds[3][2]
    _, m = runs_of(c)
    assert {r % 6 for r in m["rev_rows"]} == {4}                                          # only the fifth source contributes
    good = c["views"][4]["kept"]
    assert ((good["camID2"] == 77) & (good["segID2"] >= v["S"])).sum() == 2
    c = C["list_lengths"]
    assert [len(w["kept"]) for w in c["views"][:3]] == [8191, 8192, 8193] == c["about"]["lengths"] and cc.MIN_BPS_RECORDS == 32 * 256
    assert all(w["kept"]["camID2"][-1] == 40 for w in c["views"][:3])                    # the last record of each list counts
    assert [len(C["neighbours_%d" % n]["views"][-1]["l2g"]) for n in (1, 2, 24, 255)] == [1, 2, 24, 255]
    for n in (2, 24, 255):
        assert C["neighbours_%d" % n]["views"][-1]["source_cam"].tolist() == [n - 1]
    for rows in (1, 4095, 4096, 4097, 8191, 8193):
        c = C["rows_%d" % rows]
        v = c["views"][-1]
        m = cm.model(c)
        assert v["S"] * len(v["l2g"]) == rows and (np.diff(m["row_start"])[:min(rows, cc.TILE)] > 0).any()
        if rows > cc.TILE:
            assert m["row_start"][cc.TILE] > 0 and m["row_start"][-1] > m["row_start"][cc.TILE]      # the carry into the second tile matters


def test_rule_mirrors():
    from line3d_amd import capi
    for opt in (-1, 0, 1, 2, 3, 4, 8, 16, 32, 64, 65, 512):
        for avg in (0.0, 0.9, 3.0, 70.0, 1e7):
            assert cm.lanes_rule(opt, avg) == capi.rt_lanes(opt, avg), (opt, avg)
    assert cm.rules(cc.CASES["run_lengths"], 0, -1, 0.0)[1] == 32 and cm.rules(cc.CASES["run_lengths"], 0, -1, 3.0e6)[1] == 512
