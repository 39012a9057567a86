"""The crafted tables of tests/affinity_cases.py and the model of tests/affinity_model.py, checked without a GPU: the model's candidate list equals the
literal `used` rule (tests/cpp/literal_used_rule.c) item for item on every valid case and on a few hundred random small tables, every case reaches
the branch it was built for, the table check's verdicts are what the cases state, the byte flags alone reproduce the candidates, and the exact-weight
construction holds in float32."""
import numpy as np
import pytest

import affinity_cases as ac
import affinity_model as am
from helpers import literal_rule_items, literal_rule_lib

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return literal_rule_lib()


@pytest.fixture(scope="module")
def models():
    return {n: ac.run_model(c["t"]) for n, c in ac.CASES.items()}


def same_items(items, lit):
    if len(items) != len(lit):
        return False
    mine = np.zeros(len(items), lit.dtype)
    for k, (a, b, f, cw) in enumerate(items):
        mine[k] = (a, b, f, cw)
    return mine.tobytes() == lit.tobytes()


def test_the_cases_the_issue_lists_are_all_here():
    names = set(ac.CASES)
    want = {"group_%d" % n for n in (1, 2, 63, 64, 65, 128, 129)} | {"words_T_%d" % n for n in (1, 63, 64, 65, 128, 129)} \
        | {"f2_list_%d" % n for n in (0, 1, 63, 64, 65, 130)} | {"n_hyp_%d" % n for n in (1, 255, 256, 257)} \
        | {"group_starts_in_lane_63", "chain_64", "chain_70", "fan_65", "blocks_40_by_40", "real_geometry", "nothing_passes"}
    assert want <= names, sorted(want - names)
    assert len(ac.CASES) >= 60 and len(ac.INVALID) >= 24
    assert max(int(np.diff(c["t"]["seg_base"]).max()) for c in ac.CASES.values()) <= 141
    assert max(int(c["t"]["seg_base"][-1]) for c in ac.CASES.values()) <= 300


@pytest.mark.parametrize("name", list(ac.CASES))
def test_model_equals_the_literal_rule_and_the_case_reaches_its_branch(lib, models, name):
    c, m = ac.CASES[name], models[name]
    assert same_items(m["items"], literal_rule_items(lib, c["t"]))
    assert m["codes"] == (), m["message"]
    assert c["reach"](m, c["t"]), c["why"]
    assert int(m["src_count"].sum()) == len(m["items"])
    # the upload reads the CSR totals: the arrays the test owns end exactly there
    t = c["t"]
    assert t["pot_start"][-1] == len(t["pot_tgt"]) and t["coll_start"][-1] == len(t["coll_other"]) == len(t["coll_w"])


@pytest.mark.parametrize("name", list(ac.CASES))
def test_flags_replayed_give_the_candidates(models, name):
    c, m = ac.CASES[name], models[name]
    t = c["t"]
    replay = am.replay_flags(t, m["flags"])
    assert [(a, b, f, cw.tobytes()) for a, b, f, cw in replay] == [(a, b, f, cw.tobytes()) for a, b, f, cw in m["items"]]
    # family 0 <=> bit 1, in entry order
    fam0 = [(a, b) for a, b, f, _ in m["items"] if f == 0]
    src_of = np.repeat(np.arange(len(t["best"])), np.diff(t["pot_start"]))
    bits = [(int(t["best"][src_of[e]]), int(t["best"][t["pot_tgt"][e]])) for e in np.flatnonzero(m["flags"] & 2)]
    assert fam0 == bits
    assert not (m["flags"] & 2)[(m["flags"] & 1) == 0].any() and not (m["flags"] & 1)[(m["flags"] & 4) != 0].any()
    assert not m["flags"][t["best"][src_of] < 0].any()


def test_random_tables_model_equals_literal_rule(lib):
    n_items, kinds = 0, set()
    for seed in range(320):
        one_way, asym = bool(seed & 1), bool(seed & 2)
        t = ac.random_table(1000 + seed, one_way=one_way, asym=asym)
        m = ac.run_model(t)
        assert m["codes"] == ()
        assert same_items(m["items"], literal_rule_items(lib, t)), seed
        replay = am.replay_flags(t, m["flags"])
        assert [(a, b, f) for a, b, f, _ in replay] == [(a, b, f) for a, b, f, _ in m["items"]], seed
        n_items += len(m["items"])
        kinds.add((m["two_way"], m["sym"]))
    assert n_items > 8000 and kinds == {(True, True), (True, False), (False, True), (False, False)}


def test_symmetry_verdicts(models):
    for n, c in ac.CASES.items():
        asym = n.startswith("asym_") or n in ("f2_earlier_does_not_list_source", "real_geometry")
        assert models[n]["sym"] == (not asym), n


@pytest.mark.parametrize("name", list(ac.INVALID))
def test_invalid_table_differs_from_its_base_in_one_place(name):
    c = ac.INVALID[name]
    diff = []
    for k in am.TABLE_KEYS:
        a, b = c["t"][k], ac.BASE[k]
        assert a.shape == b.shape and a.dtype == b.dtype
        if k != "hyp":
            diff += [(k, int(i)) for i in np.flatnonzero(a != b)]
        else:
            assert a.tobytes() == b.tobytes()
    assert sorted(diff) == sorted((k, int(i)) for k, i, _ in c["change"]) and len(diff) == c["places"]
    assert len(diff) == 1 or name == "hyp_dense_not_ascending"
    codes, message, _ = am.validate(c["t"])
    assert codes == c["codes"] and len(codes) in (1, 2) and message == c["message"] and message
    assert am.validate(ac.BASE)[0] == ()
    t = c["t"]
    assert t["pot_start"][-1] == len(t["pot_tgt"]) and t["coll_start"][-1] == len(t["coll_other"])


def test_invalid_tables_cover_every_code_and_host_check():
    seen = {c["codes"] for c in ac.INVALID.values()}
    assert {(1,), (2,), (3,), (4,), (5,), ("host", am.HOST_CSR0), ("host", am.HOST_ASCEND), ("host", am.HOST_COVER)} == seen
    assert am.validate(ac.no_hypotheses()) == ((), "", True)


def test_exact_weight_construction_in_float32():
    """the threshold cases land on the intended side, and their neighbours one ulp away on the other"""
    half = F32(0.5)
    assert F32(half * F32(ac.SA25 + ac.SA25)) == ac.C25 and not ac.C25 > F32(0.25)
    up25 = F32(half * F32(ac.SA25 + ac.SB25))
    assert up25 == np.nextafter(ac.C25, F32(1)) and up25 > F32(0.25) and np.nextafter(up25, F32(0)) == ac.C25
    assert F32(half * F32(ac.C01 + ac.C01)) == ac.C01 and not ac.C01 > F32(0.01)
    up01 = F32(half * F32(ac.C01 + ac.SB01))
    assert up01 == np.nextafter(ac.C01, F32(1)) and up01 > F32(0.01) and np.nextafter(up01, F32(0)) == ac.C01
    # family 2: ((cw * 0.5) * (sa + sb)) * sim
    for cw, sa, sb, want in ((ac.C01, F32(1), F32(1), ac.C01), (ac.UP(ac.C01), F32(1), F32(1), up01), (F32(1), ac.C01, ac.C01, ac.C01), (F32(1), ac.C01, ac.SB01, up01)):
        assert F32(F32(F32(cw * half) * F32(sa + sb)) * F32(1)) == want
    # the two classes: similarity exactly 1 and 0 in the reference's arithmetic is pinned on the device (test_gpu_affinity_paths.py); here: what the
    # construction rests on -- a point of a class' line lies on it, the other class' points at distance 1 from it, far outside k_upper * depth = 0.2
    x, y = ac.hyp_record("x"), ac.hyp_record("y")
    for h in (x, y):
        assert np.cross(h["P1"], h["dir"]).tolist() == [0, 0, 0] and np.cross(h["P2"], h["dir"]).tolist() == [0, 0, 0]
    assert float(x["dir"] @ y["dir"]) == 0.0 and np.linalg.norm(np.cross(x["P1"], y["dir"])) == 1.0


def test_threshold_cases_sit_exactly_on_their_thresholds(models):
    for name, thr in (("threshold_family_0", ac.C25), ("threshold_family_1", ac.C01), ("threshold_family_2_through_cw", ac.C01),
                      ("threshold_family_2_through_scores", ac.C01)):
        m = models[name]
        on = [(w, p) for w, p in zip(m["w"], m["passed"]) if w == thr]
        above = [(w, p) for w, p in zip(m["w"], m["passed"]) if w == np.nextafter(thr, F32(1))]
        assert len(on) == 1 and not on[0][1] and len(above) == 1 and above[0][1], name


def test_parts_of_the_model_put_together_give_the_whole():
    """the part arithmetic the GPU test relies on, on the model alone: any split of the sources at view boundaries, merged, is the whole list"""
    edge = np.dtype([("i", "<i4"), ("j", "<i4"), ("w", "<f4")])
    for name in ("blocks_40_by_40", "one_way_in_two_views_of_five", "failing_candidate_before_passing_one", "untouched_hypotheses_front_middle_end"):
        t = ac.CASES[name]["t"]
        m = ac.run_model(t)
        nh = len(t["hyp_dense"])
        l2g = (np.arange(nh) * 3 + 5).astype(np.int32)
        vhb = [int(v) for v in t["view_hyp_begin"]]
        for cuts in ([0, vhb[1], nh], [0, vhb[1], vhb[1], nh]):
            parts = [am.part(t, m["items"], m["sim"], cuts[r], cuts[r + 1], r << 44, l2g) for r in range(len(cuts) - 1)]
            A, node_hyp = am.merge_parts(parts, l2g, int(l2g[-1]) + 1, edge)
            assert A.tobytes() == m["edges"].tobytes() and node_hyp.tobytes() == l2g[m["node_hyp"]].tobytes(), (name, cuts)
            assert sum(p["n_candidates"] for p in parts) == len(m["items"])
