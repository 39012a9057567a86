"""The builder of matchViews' products (l3d_products.hip) on the crafted kept lists of tests/products_cases.py, through l3d_test_products: every case on
every variant of the build -- the sort, the transposed build with rebuilt side arrays, with side arrays made beforehand, with the chain's early pair
transposes, the lanes per run, the block sizes -- against the plain model of tests/products_model.py.  Everything compared is an integer or a selected
float: no tolerance anywhere.  The hook's report is held to mirrors of the builder's rules, so a case meant for one build that quietly took another fails."""
import numpy as np
import pytest

import products_cases as pc
import products_model as pm
from line3d_amd import capi

pytestmark = pytest.mark.gpu

#            options (prod_transpose, prod_pair_g, prod_block_keys; "cut": pc.cut_budget), side_arrays, early_pairs
VARIANTS = {
    "sort": (dict(prod_transpose=0), 0, 0),
    "rebuilt": (dict(), 0, 0),
    "native": (dict(), 1, 0),
    "early_pairs": (dict(), 1, 1),
    "g0": (dict(prod_pair_g=0), 0, 0),
    "g1": (dict(prod_pair_g=1), 0, 0),
    "g16": (dict(prod_pair_g=16), 1, 0),
    "g64": (dict(prod_pair_g=64), 0, 0),
    "early_pairs_g0": (dict(prod_pair_g=0), 1, 1),
    "block_1": (dict(prod_block_keys=1), 0, 0),
    "block_cut": (dict(prod_block_keys="cut"), 0, 0),
    "native_block_1": (dict(prod_block_keys=1), 1, 0),
    "sort_block_1": (dict(prod_transpose=0, prod_block_keys=1), 0, 0),
    "sort_block_cut": (dict(prod_transpose=0, prod_block_keys="cut"), 0, 0),
}
UNORDERED = ("wayout_adjacent_records_swapped", "wayout_camera_is_no_neighbour")       # lists that get no side arrays: nothing for the early pair transposes to read
EXCLUDED = [(c, v) for c in UNORDERED for v in VARIANTS if VARIANTS[v][2]]
RUNS = [(c, v) for c in pc.CASES for v in VARIANTS if (c, v) not in EXCLUDED]
assert len(RUNS) == len(pc.CASES) * len(VARIANTS) - len(UNORDERED) * 2

_RAN, _REACHED, _DIGESTS, _MODELS = set(), set(), {}, {}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = pm.model(pc.CASES[name])
    return _MODELS[name]


def run(ctx, case, variant):
    opts, side, early = VARIANTS[variant]
    sort = opts.get("prod_transpose", 1) == 0
    budget = opts.get("prod_block_keys", 0)
    if budget == "cut":
        budget = pc.cut_budget(case, sort)
    ctx.set_option("prod_transpose", 0 if sort else 1)
    ctx.set_option("prod_pair_g", opts.get("prod_pair_g", -1))
    ctx.set_option("prod_block_keys", budget)
    try:
        out = ctx.test_products(case["chain"], case["view_ids"], [0] + list(np.cumsum([case["S"][i] for i in case["view_ids"]])), side_arrays=side,
                                early_pairs=early, rows=case["rows"], held=case["held"])
    except capi.L3DError as e:          # a failing device call leaves nothing to compare, and nothing more is started on the device
        pytest.exit("%s / %s: %s" % (case["name"], variant, e), 1)
    return out, sort, budget


def check_report(case, variant, out, sort, budget):
    """what the hook says ran, against the case's expectation and mirrors of the builder's rules"""
    opts, side, early = VARIANTS[variant]
    rep, exp, name = out["report"], case["expect"], case["name"]
    bad = []
    ordered = name not in UNORDERED
    if rep["side_arrays_used"] != (1 if side and ordered else 0):
        bad.append("side arrays used: %d" % rep["side_arrays_used"])
    want_build = capi.PROD_SORTED if sort or exp["build"] == "sorted" else capi.PROD_TRANSPOSED
    want_refused = 0 if sort else exp["refused"]
    if (rep["build"], rep["refused"]) != (want_build, want_refused):
        bad.append("build %d, refused %d: expected %d, %d" % (rep["build"], rep["refused"], want_build, want_refused))
    plan = pc.plan_blocks(case, budget, rep["build"] == capi.PROD_SORTED)
    if rep["n_blocks"] != len(plan):
        bad.append("%d blocks, the rule gives %d" % (rep["n_blocks"], len(plan)))
    if rep["build"] == capi.PROD_TRANSPOSED:
        dv0, dv1 = case["rows"] or (0, len(case["view_ids"]))
        touch = max([0] + [len(pc.touched_views(case, case["view_ids"][x])) for x in range(dv0, dv1)])
        if rep["max_touch"] != touch:
            bad.append("a row touches %d views, the case has %d" % (rep["max_touch"], touch))
        use_early = early and ordered
        caps = [-1 if use_early or b["pairs"] == 0 or b["rows"] == 0 else pc.cap_rule(b["max_S"]) for b in plan]
        staged = [1 if b["rows"] > 0 and pc.staging_rule(b["records"], b["rows"]) else 0 for b in plan]
        if rep["block_cap"] != caps or rep["block_staged"] != staged:
            bad.append("cap %s staged %s, the rules give %s %s" % (rep["block_cap"], rep["block_staged"], caps, staged))
        g = opts.get("prod_pair_g", -1)
        if g >= 0 and any(x not in (-1, g) for x in rep["block_g"] + [rep["early_g"]]):
            bad.append("lanes per run %s / %d, asked for %d" % (rep["block_g"], rep["early_g"], g))
        if use_early:
            St = max([1] + [case["S"][g_] for v in case["chain"] if v["n_tbm"] > 0 for g_ in v["l2g"] if g_ in case["S"]])
            if rep["early_cap"] != pc.cap_rule(St):
                bad.append("early cap %d, the rule gives %d" % (rep["early_cap"], pc.cap_rule(St)))
        elif rep["early_cap"] != -1:
            bad.append("early transposes ran")
    return bad


def note_branches(case, variant, out):
    """the branches a passed run has been through, by the report and the case's own numbers (tests/test_products_cases_cpu.py holds the cases to them)"""
    opts, side, early = VARIANTS[variant]
    rep, name = out["report"], case["name"]
    has_early = any(v["n_tbm"] == 0 and len(v["source_index"]) for v in case["chain"])
    if rep["build"] == capi.PROD_SORTED:
        _REACHED.add("sorted build")
        if rep["n_blocks"] > 1:
            _REACHED.add("sorted build over several blocks")
        if has_early:
            _REACHED.add("k_prod_keys_early")
        for r in (1, 2):
            if rep["refused"] == r:
                _REACHED.add("refusal %d" % r)
        return
    if "row" in case:
        short = len(pc.touched_views(case, case["row"][0])) <= 64 and case["entries"] + case["extras"] <= pc.SHORT_ROW
        _REACHED.add("short path" if short else "bitmap")
        if short and 1 in rep["block_staged"] and case["unique"] + case["extras"] < pc.SHORT_ROW:
            _REACHED.add("staged rows")
        if short and 1 not in rep["block_staged"]:
            _REACHED.add("short path without staging")
        if short and case["unique"] + case["extras"] == pc.SHORT_ROW:
            _REACHED.add("64 unique: recomputed by the write pass")
    if rep["max_touch"] > 64:
        _REACHED.add("more than 64 touched views")
    caps = rep["block_cap"] + [rep["early_cap"]]
    if case.get("two_level"):
        for cap in (7168, 1024):
            if cap in caps:
                _REACHED.add("two-level scatter, cap %d" % cap)
    if name == "scatter_busy_column_falls_back" and max(caps) > 0:
        _REACHED.add("direct fallback")
    if has_early:
        _REACHED.add("k_prod_early_rt" if rep["side_arrays_used"] else "k_prodt_early")
        if not rep["side_arrays_used"]:
            _REACHED.add("k_prod_keys_early")
    if early and rep["early_cap"] >= 0:
        _REACHED.add("early pair transposes")


def compare(ctx, case, variant, out):
    m = model_of(case["name"])
    bad = []
    nd, n_pot = m["n_dense"], out["n_pot"]
    tgt = out["pot_tgt"]
    if len(tgt) != n_pot + 64 or not (tgt[n_pot:] == -1).all():
        bad.append("the slots behind n_pot were written")
    if case["rows"] is None:
        if n_pot != len(m["pot_tgt"]) or not np.array_equal(out["pot_start"], m["pot_start"]) or not np.array_equal(tgt[:n_pot], m["pot_tgt"]):
            wrong = [d for d in range(nd) if out["pot_start"][d + 1] - out["pot_start"][d] != len(m["rows"][d])
                     or tgt[out["pot_start"][d]:out["pot_start"][d + 1]].tolist() != m["rows"][d]]
            bad.append("n_pot %d (model %d), rows that differ: %s" % (n_pot, len(m["pot_tgt"]), wrong[:8]))
    else:
        base = [0] + list(np.cumsum([case["S"][i] for i in case["view_ids"]]))
        r0, r1 = base[case["rows"][0]], base[case["rows"][1]]
        first = m["pot_start"][r0]
        if n_pot != m["pot_start"][r1] - first:
            bad.append("n_pot %d, the model's slice has %d" % (n_pot, m["pot_start"][r1] - first))
        elif r1 > r0 or case["held"] is not None:
            ps = out["pot_start"]
            if r1 > r0 and (not np.array_equal(ps[r0:r1 + 1], m["pot_start"][r0:r1 + 1] - first) or not np.array_equal(tgt[:n_pot], m["pot_tgt"][first:first + n_pot])):
                bad.append("the rows of the range differ")
            if case["held"] is not None:
                lo, hi = (r0, r1 + 1) if r1 > r0 else (nd + 1, nd + 1)
                if (ps[:lo] != 0).any() or (ps[hi:] != n_pot).any() or (np.diff(ps) < 0).any():
                    bad.append("rows outside the range are not empty")
    if out["best"].tobytes() != m["best"].tobytes():
        d = [i for i in range(nd) if out["best"][i].tobytes() != m["best"][i].tobytes()]
        bad.append("best matches differ at %s: %s / %s" % (d[:6], out["best"][d[0]], m["best"][d[0]]))
    s = out["summary"]
    if s["median_depth"].astype(np.float32).tobytes() != m["median"].tobytes():
        bad.append("medians %s, model %s" % (s["median_depth"], m["median"]))
    if s["verified"].tolist() != m["verified"] or s["n_kept"].tolist() != m["n_kept"] or s["n_candidates"].tolist() != m["n_candidates"]:
        bad.append("summary %s" % s)
    # the getters answer as after a resident chain
    for k in range(len(case["chain"])):
        if ctx.chain_kept_list(k).tobytes() != np.array(m["lists"][k], dtype=pm.MATCH_DTYPE).tobytes():
            bad.append("l3d_chain_kept_list(%d) differs" % k)
    hsh, cnt = ctx.chain_records_digest(len(case["chain"]))
    if cnt.tolist() != [n if v else 0 for n, v in zip(m["n_kept"], m["verified"])]:
        bad.append("digest lengths %s" % cnt)
    if _DIGESTS.setdefault(case["name"], hsh.tobytes()) != hsh.tobytes():
        bad.append("record digests differ between variants")
    return bad


@pytest.mark.parametrize("name", list(pc.CASES))
def test_case_on_every_variant(ctx, name):
    case = pc.CASES[name]
    failures = []
    for variant in VARIANTS:
        if (name, variant) in EXCLUDED:
            continue
        out, sort, budget = run(ctx, case, variant)
        bad = check_report(case, variant, out, sort, budget) + compare(ctx, case, variant, out)
        if bad:
            failures.append("%s: %s" % (variant, "; ".join(bad)))
        else:
            note_branches(case, variant, out)
        _RAN.add((name, variant))
    assert not failures, "\n".join(failures)


def test_every_pair_ran_and_every_branch_was_reached():
    assert _RAN == set(RUNS) and len(_RAN) == len(pc.CASES) * len(VARIANTS) - len(EXCLUDED)
    want = {"short path", "staged rows", "short path without staging", "64 unique: recomputed by the write pass", "bitmap", "more than 64 touched views",
            "two-level scatter, cap 7168", "two-level scatter, cap 1024", "direct fallback", "refusal 1", "refusal 2", "sorted build",
            "sorted build over several blocks", "k_prod_keys_early", "k_prod_early_rt", "k_prodt_early", "early pair transposes"}
    assert want <= _REACHED, sorted(want - _REACHED)
