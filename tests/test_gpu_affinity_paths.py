"""The affinity fill (l3d_affinity.hip: k_aff_validate, k_aff_sym, k_aff_groups in both variants, k_aff_words, k_aff_items<false/true>, first-touch minima,
numbering and edges) on the crafted tables of tests/affinity_cases.py against the plain model of tests/affinity_model.py: the whole fill through
Context.affinity_fill under the option sets a case names, the byte flags / needs_prev / launch count / coll_sym and a part's passed list and minima
through l3d_test_affinity_fill (the core the sharded fill runs, with a FillPart), and tables that are wrong in one place.  Everything compared is an
integer or an exact float32 product: bytes, no tolerance anywhere."""
import numpy as np
import pytest

import affinity_cases as ac
import affinity_model as am
from line3d_amd import capi

pytestmark = pytest.mark.gpu

DEFAULTS = {"L3D_AFF_CHUNK": 0, "L3D_AFF_SYM": 1, "L3D_AFF_PER_VIEW": 0, "L3D_AFF_BLOCK": 0, "L3D_AFF_WORD_BLOCK": 0}
OPTION_SETS = {
    "default": {},
    "chunk1": {"L3D_AFF_CHUNK": 1}, "chunk2": {"L3D_AFF_CHUNK": 2}, "chunk5": {"L3D_AFF_CHUNK": 5}, "chunk63": {"L3D_AFF_CHUNK": 63},
    "sym0": {"L3D_AFF_SYM": 0},
    "per_view": {"L3D_AFF_PER_VIEW": 1},
    "block1": {"L3D_AFF_BLOCK": 1}, "block7": {"L3D_AFF_BLOCK": 7}, "block32": {"L3D_AFF_BLOCK": 32},
    "wblock1": {"L3D_AFF_WORD_BLOCK": 1}, "wblock3": {"L3D_AFF_WORD_BLOCK": 3},
    "mixed_a": {"L3D_AFF_CHUNK": 5, "L3D_AFF_SYM": 0, "L3D_AFF_PER_VIEW": 1, "L3D_AFF_BLOCK": 7},
    "mixed_b": {"L3D_AFF_CHUNK": 2, "L3D_AFF_BLOCK": 1, "L3D_AFF_WORD_BLOCK": 1},
}
HOOK_CHUNKS = (0, 1, 2, 5, 63)
_RAN, _REACHED, _MODELS = set(), set(), {}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def device(what, fn, *a, **kw):
    """a device call that must succeed: a failing one leaves nothing to compare, and nothing more is started on the device"""
    try:
        return fn(*a, **kw)
    except capi.L3DError as e:
        pytest.exit("%s: %s" % (what, e), 1)


def options(ctx, env):
    for k, v in dict(DEFAULTS, **env).items():
        ctx.set_option(k, v)


def model(ctx, name):
    if name not in _MODELS:
        t = ac.CASES[name]["t"]
        sim = None
        if t.get("sim") == "device":
            items = am.enumerate_candidates(t)["items"]
            sim = device(name + ": similarities", ctx.similarity_coll3D_batch, t["hyp"], np.array([[a, b] for a, b, _, _ in items], np.int32), t["sigma_a"])
        _MODELS[name] = ac.run_model(t, sim)
    return _MODELS[name]


def whole_fill_differs(ctx, what, t, m):
    A, node_hyp, n_cand = device(what, ctx.affinity_fill, *ac.arrays(t))
    counts = device(what, ctx.last_fill_counts)
    bad = []
    if A.tobytes() != m["edges"].tobytes():
        k = next((i for i in range(min(len(A), len(m["edges"]))) if A[i].tobytes() != m["edges"][i].tobytes()), min(len(A), len(m["edges"])))
        bad.append("edges differ (%d / %d entries, first at %d)" % (len(A), len(m["edges"]), k))
    if node_hyp.tobytes() != m["node_hyp"].tobytes():
        bad.append("node_hyp differs: %s / %s" % (node_hyp[:8], m["node_hyp"][:8]))
    if n_cand != len(m["items"]) or counts != (len(m["items"]), int(m["passed"].sum())):
        bad.append("counts: %d, %s / %d, %d" % (n_cand, counts, len(m["items"]), int(m["passed"].sum())))
    return bad


def test_the_two_classes_have_similarity_exactly_1_and_0(ctx):
    """what every exact weight rests on: the similarity the fill computes (the seam call runs the same device function) for hypotheses of one class is
    exactly 1, of different classes exactly 0"""
    hyp = np.array([ac.hyp_record("x"), ac.hyp_record("y"), ac.hyp_record("x"), ac.hyp_record("y")])
    pairs = np.array([[0, 2], [1, 3], [0, 0], [0, 1], [1, 0], [2, 3]], np.int32)
    sim = device("similarities", ctx.similarity_coll3D_batch, hyp, pairs, ac.SIGMA_A)
    assert sim.tobytes() == np.array([1, 1, 1, 0, 0, 0], np.float32).tobytes()


@pytest.mark.parametrize("name", list(ac.CASES))
def test_whole_fill_under_the_case_option_sets(ctx, name):
    c = ac.CASES[name]
    t, m = c["t"], model(ctx, name)
    assert c["reach"](m, t)
    failures = []
    try:
        if "fresh_context" in c:      # the pass lists grow from their first small size only on a context that has not filled before
            fresh = capi.Context(0)
            try:
                options(fresh, OPTION_SETS[c["fresh_context"]])
                bad = whole_fill_differs(fresh, "%s / fresh context" % name, t, m)
                if bad:
                    failures.append("fresh context, %s: %s" % (c["fresh_context"], "; ".join(bad)))
            finally:
                fresh.close()
            _REACHED.add("fresh context")
        for s in c["sets"]:
            options(ctx, OPTION_SETS[s])
            bad = whole_fill_differs(ctx, "%s / %s" % (name, s), t, m)
            if bad:
                failures.append("%s: %s" % (s, "; ".join(bad)))
            _RAN.add((name, s))
    finally:
        options(ctx, {})
    assert not failures, "\n".join(failures)
    _REACHED.add(name)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_hook_flags_schedule_and_symmetry(ctx, name):
    """the byte flags after the last k_aff_groups launch, needs_prev, the number of launches and coll_sym, under each chunk and both aff_sym values;
    the part [0, n_hyp) with no renumbering is the whole enumeration: passed pairs, weights and minima"""
    t, m = ac.CASES[name]["t"], model(ctx, name)
    nh = len(t["hyp_dense"])
    whole = am.part(t, m["items"], m["sim"], 0, nh)
    failures = []
    try:
        for chunk in HOOK_CHUNKS:
            for sym in (1, 0):
                for per_view in ((0, 1) if chunk == 0 and sym == 1 else (0,)):
                    options(ctx, {"L3D_AFF_CHUNK": chunk, "L3D_AFF_SYM": sym, "L3D_AFF_PER_VIEW": per_view})
                    out = device("%s / chunk %d sym %d" % (name, chunk, sym), ctx.test_affinity_fill, ac.arrays(t))
                    bad = []
                    if out["flags"].tobytes() != m["flags"].tobytes():
                        e = int(np.flatnonzero(out["flags"] != m["flags"])[0])
                        bad.append("flags differ, first at entry %d: %d / %d" % (e, out["flags"][e], m["flags"][e]))
                    if out["needs_prev"].tobytes() != m["needs_prev"].tobytes():
                        bad.append("needs_prev %s / %s" % (out["needs_prev"], m["needs_prev"]))
                    if out["n_launches"] != (m["launches_per_view"] if per_view else m["launches"]):
                        bad.append("%d launches of k_aff_groups" % out["n_launches"])
                    if out["coll_sym"] != int(m["sym"] and sym == 1):
                        bad.append("coll_sym %d" % out["coll_sym"])
                    if out["pairs"].tobytes() != whole["pairs"].tobytes() or out["w"].tobytes() != whole["w"].tobytes() or out["n_candidates"] != len(m["items"]):
                        bad.append("passed list: %d of %d / %d of %d" % (out["n_passed"], out["n_candidates"], len(whole["w"]), len(m["items"])))
                    if out["first"].tobytes() != whole["first"].tobytes():
                        bad.append("first-touch minima differ")
                    if bad:
                        failures.append("chunk %d, aff_sym %d, per_view %d: %s" % (chunk, sym, per_view, "; ".join(bad)))
                    _RAN.add((name, "hook", chunk, sym, per_view))
    finally:
        options(ctx, {})
    assert not failures, "\n".join(failures)
    _REACHED.add("coll_sym %d" % int(m["sym"]))
    _REACHED.add("%d launches" % m["launches"])
    if m["needs_prev"].any():
        _REACHED.add("needs_prev cut")


def part_cuts(t):
    """sources split at view boundaries into 2 and 3 parts; an empty part and a part of one source among them"""
    vhb = [int(v) for v in t["view_hyp_begin"]]
    nh, V = vhb[-1], len(vhb) - 1
    cuts = [[0, vhb[(V + 1) // 2], nh], [0, vhb[1], vhb[1], nh]]
    if V >= 3:
        cuts.append([0, vhb[1], vhb[2], nh])
    one = next((v for v in range(V) if vhb[v + 1] - vhb[v] == 1), None)
    if one is not None:
        cuts.append([0, vhb[one], vhb[one + 1], nh])
    return cuts


@pytest.mark.parametrize("name", list(ac.CASES))
def test_parts_equal_the_model_and_put_together_the_whole_fill(ctx, name):
    """affinity_fill_core with a FillPart, as every rank of the sharded fill runs it: pos_base = rank << 44, a non-identity loc2glob, assume_symmetric 0 and
    (tables with every record both ways only) 1.  Every part's passed list and minima equal the model's; the lists in rank order with the element-wise
    minimum of the minima, numbered, are the whole fill's edge list."""
    t, m = ac.CASES[name]["t"], model(ctx, name)
    nh = len(t["hyp_dense"])
    l2g = (np.arange(nh) * 3 + 5).astype(np.int32)
    failures = []
    for cuts in part_cuts(t):
        for assume in ((0, 1) if m["two_way"] else (0,)):
            parts = []
            for r in range(len(cuts) - 1):
                h0, h1 = cuts[r], cuts[r + 1]
                out = device("%s / part %d of %s" % (name, r, cuts), ctx.test_affinity_fill, ac.arrays(t), h0=h0, h1=h1, pos_base=r << 44, loc2glob=l2g,
                             assume_symmetric=assume)
                want = am.part(t, m["items"], m["sim"], h0, h1, r << 44, l2g)
                bad = [k for k in ("pairs", "w", "first") if out[k].tobytes() != want[k].tobytes()]
                if out["n_candidates"] != want["n_candidates"] or out["n_passed"] != len(want["w"]):
                    bad.append("counts %d, %d / %d, %d" % (out["n_candidates"], out["n_passed"], want["n_candidates"], len(want["w"])))
                if out["flags"].tobytes() != m["flags"].tobytes():
                    bad.append("flags")
                if out["needs_prev"].tobytes() != am.needs_prev(t, assume).tobytes() or out["n_launches"] != am.group_launches(t, assume_symmetric=assume):
                    bad.append("schedule")
                if bad:
                    failures.append("cuts %s, part %d, assume_symmetric %d: %s" % (cuts, r, assume, ", ".join(bad)))
                parts.append(out)
                _REACHED.add("part: empty" if h1 == h0 else "part: one source" if h1 - h0 == 1 else "part: several sources")
            A, node_hyp = am.merge_parts(parts, l2g, int(l2g[-1]) + 1, capi.EDGE_DTYPE)
            if A.tobytes() != m["edges"].tobytes() or node_hyp.tobytes() != l2g[m["node_hyp"]].tobytes():
                failures.append("cuts %s, assume_symmetric %d: the parts put together are not the whole fill" % (cuts, assume))
            _RAN.add((name, "parts", tuple(cuts), assume))
            _REACHED.add("assume_symmetric %d" % assume)
    assert not failures, "\n".join(failures)


def _refused(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.L3DError as e:
        return e.code, str(e)
    return 0, ""


@pytest.mark.parametrize("name", list(ac.INVALID))
def test_a_table_that_is_wrong_in_one_place_is_refused(ctx, name):
    """k_aff_validate's promise: a bad table is an error message and not a fault inside the later kernels -- L3D_ERR_INVALID with the finding's message,
    from the fill and from the hook"""
    c = ac.INVALID[name]
    for what, fn, args in (("fill", ctx.affinity_fill, ac.arrays(c["t"])), ("hook", ctx.test_affinity_fill, (ac.arrays(c["t"]),))):
        code, text = _refused(fn, *args)
        assert code == 1 and text.endswith(": " + c["message"]), (what, code, text)        # L3D_ERR_INVALID
    _REACHED.add("refused: " + name)


def test_no_hypotheses_is_ok_and_empty(ctx):
    t = ac.no_hypotheses()
    A, node_hyp, n_cand = device("no hypotheses", ctx.affinity_fill, *ac.arrays(t))
    assert len(A) == 0 and len(node_hyp) == 0 and n_cand == 0
    out = device("no hypotheses, hook", ctx.test_affinity_fill, ac.arrays(t))
    assert out["n_passed"] == 0 and out["n_candidates"] == 0 and out["n_launches"] == 0 and len(out["first"]) == 0
    _REACHED.add("no hypotheses")


def test_valid_tables_after_the_refused_ones(ctx):
    """the context that refused all of them still fills: the invalid tables' base and a case with several passes and blocks"""
    assert {"refused: " + n for n in ac.INVALID} <= _REACHED
    base = ac.run_model(ac.BASE)
    assert base["codes"] == () and len(base["edges"]) > 10
    assert not whole_fill_differs(ctx, "base after the refused tables", ac.BASE, base)
    out = device("base, hook", ctx.test_affinity_fill, ac.arrays(ac.BASE))
    assert out["flags"].tobytes() == base["flags"].tobytes() and out["coll_sym"] == 1
    assert not whole_fill_differs(ctx, "chain_70 after the refused tables", ac.CASES["chain_70"]["t"], model(ctx, "chain_70"))
    _REACHED.add("valid after refused")


def test_every_case_ran_and_every_branch_was_reached():
    runs = {(n, s) for n, c in ac.CASES.items() for s in c["sets"]}
    assert runs <= _RAN and len(runs) >= 3 * len(ac.CASES)
    assert {s for _, s in runs} == set(OPTION_SETS)
    for n in ac.CASES:
        assert sum(1 for r in _RAN if r[0] == n and r[1] == "hook") == 2 * len(HOOK_CHUNKS) + 1, n
        assert any(r[0] == n and r[1] == "parts" for r in _RAN), n
    want = set(ac.CASES) | {"refused: " + n for n in ac.INVALID} | {"fresh context", "coll_sym 0", "coll_sym 1", "1 launches", "2 launches", "3 launches", "needs_prev cut",
                                                                   "part: empty", "part: one source", "part: several sources", "assume_symmetric 0", "assume_symmetric 1",
                                                                   "no hypotheses", "valid after refused"}
    assert want <= _REACHED, sorted(want - _REACHED)
