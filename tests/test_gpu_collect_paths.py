"""The step of the resident chain that collects a view's candidates -- reverse matches counted out of the earlier views' kept lists, the row scan, the
merge with the stage-1 rows, the ordering of the runs -- through l3d_test_collect_candidates on the crafted cases of tests/collect_cases.py, on both
routes (records scanned; run tables with every lane count), with and without the separate sort launch, with too little room, against the plain model
of tests/collect_model.py.  Everything compared is an integer or a float that was moved: bytes, no tolerance anywhere.  The hook's report is held to
mirrors of the chain's rules, so a case that quietly took another route fails."""
import numpy as np
import pytest

import collect_cases as cc
import collect_model as cm
from line3d_amd import capi

pytestmark = pytest.mark.gpu

SLACK = 16
VARIANTS = {
    "scanned": dict(route=0, sort=0),
    "scanned_sorted": dict(route=0, sort=1),
    "scanned_long_lists": dict(route=0, sort=1, avg_kept=3.0e6),
    "run_tables": dict(route=1, sort=1),
    "run_tables_unsorted": dict(route=1, sort=0),
    "run_tables_long_lists": dict(route=1, sort=1, avg_kept=3.0e6),
    "scanned_short_of_room": dict(route=0, sort=1, short=1),
    "run_tables_short_of_room": dict(route=1, sort=1, short=1),
}
VARIANTS.update({"run_tables_g%d" % g: dict(route=1, sort=1, rt_g=g) for g in (1, 2, 4, 8, 16, 32, 64)})      # (never anything but these seven)
assert all(v.get("rt_g", -1) in (-1, 1, 2, 4, 8, 16, 32, 64) for v in VARIANTS.values())
_RAN, _REACHED, _MODELS = set(), set(), {}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = cm.model(cc.CASES[name])
    return _MODELS[name]


def applies(case, variant):
    return not (VARIANTS[variant].get("short") and model_of(case["name"])["R"] == 0)


RUNS = [(n, v) for n in cc.CASES for v in VARIANTS if applies(cc.CASES[n], v)]


def run(ctx, case, variant):
    kw, m = VARIANTS[variant], model_of(case["name"])
    cap = m["R"] - 1 if kw.get("short") else m["R"] + SLACK
    try:
        out = ctx.test_collect_candidates(case["views"], case["k"], case["rowA"], case["metaA"], case["depthsA"], case["rowcnt"], route=kw["route"],
                                          rt_g=kw.get("rt_g", -1), sort_apart=kw["sort"], cand_cap=cap, avg_kept=kw.get("avg_kept", 0.0), overflowed=case["overflowed"])
    except capi.L3DError as e:          # a failing device call leaves nothing to compare, and nothing more is started on the device
        pytest.exit("%s / %s: %s" % (case["name"], variant, e), 1)
    return out, cap


def check(case, variant, out, cap):
    kw, m = VARIANTS[variant], model_of(case["name"])
    v = case["views"][case["k"]]
    S, N, n_src = v["S"], len(v["l2g"]), len(v["source_cam"])
    bad = []
    # the report against mirrors of the chain's rules
    g, bps, blocks_move = cm.rules(case, kw["route"], kw.get("rt_g", -1), kw.get("avg_kept", 0.0))
    if (out["g"], out["bps"], out["blocks_move"]) != (g, bps, blocks_move):
        bad.append("g %d, workgroups per source %d, move blocks %d: the rules give %d, %d, %d" % (out["g"], out["bps"], out["blocks_move"], g, bps, blocks_move))
    want = capi.CK_SCAN
    if kw["route"] == 0:
        want |= (capi.CK_EXIST_COUNT if n_src else 0) | (capi.CK_PLACE if blocks_move + n_src else 0)
    else:
        want |= (capi.CK_EXIST_COUNT_RT if n_src and S else 0) | (capi.CK_PLACE_RT if blocks_move + n_src else 0)
    want |= capi.CK_SORT_RUNS if kw["sort"] and n_src and S else 0
    if out["kernels"] != want:
        bad.append("kernels %#x, expected %#x" % (out["kernels"], want))
    # row starts, scan by-products
    if out["R"] != m["R"] or not np.array_equal(out["row_start"], m["row_start"]):
        d = np.flatnonzero(out["row_start"] != m["row_start"])
        bad.append("row starts differ from row %s on (R %d, model %d)" % (d[:1], out["R"], m["R"]))
    if not cm.seg_order_ok(out["seg_order"], m["seg_sizes"]):
        bad.append("seg_order is no permutation with bins that never decrease")
    short = bool(kw.get("short"))
    if not np.array_equal(out["cursor"], np.zeros_like(m["cursor"]) if short else m["cursor"]):
        bad.append("cursors differ")
    # candidates
    meta, dep = out["cand_meta"], out["cand_depths"].view(np.uint32)
    if short:
        if not ((meta == 0xffffffff).all() and (dep == 0xffffffff).all()):
            bad.append("candidates were written although they do not fit")
        return bad
    R = m["R"]
    if not ((meta[R:] == 0xffffffff).all() and (dep[R:] == 0xffffffff).all()):
        bad.append("slots behind R were written")
    meta, dep = meta[:R].copy(), dep[:R].copy()
    if not kw["sort"]:                  # the order inside a run is not determined before the runs are ordered: by target here (targets are distinct)
        for row in m["rev_rows"]:
            a, b = int(m["row_start"][row]), int(m["row_start"][row + 1])
            o = np.argsort(meta[a:b, 0], kind="stable")
            meta[a:b], dep[a:b] = meta[a:b][o], dep[a:b][o]
    if not np.array_equal(meta, m["meta"]) or not np.array_equal(dep, m["depths"]):
        d = np.flatnonzero((meta != m["meta"]).any(1) | (dep != m["depths"]).any(1))
        bad.append("%d candidates differ, first at %d: %s %s / %s %s" % (len(d), d[0], meta[d[0]], dep[d[0]], m["meta"][d[0]], m["depths"][d[0]]))
    return bad


def note(case, variant, out):
    kw, m = VARIANTS[variant], model_of(case["name"])
    for bit, what in ((capi.CK_EXIST_COUNT, "k_exist_count"), (capi.CK_EXIST_COUNT_RT, "k_exist_count_rt + k_exist_combine"), (capi.CK_SCAN, "k_scan"),
                      (capi.CK_PLACE, "k_place"), (capi.CK_PLACE_RT, "k_place_rt"), (capi.CK_SORT_RUNS, "k_exist_sort_runs")):
        if out["kernels"] & bit:
            _REACHED.add(what)
    runs = [int(m["cursor"][r]) for r in m["rev_rows"]]
    if kw["sort"] and not kw.get("short"):
        if any(2 <= r <= 256 for r in runs):
            _REACHED.add("register sort")
        if any(r > 256 for r in runs):
            _REACHED.add("staged sort")
    if len(m["row_start"]) - 1 > cc.TILE:
        _REACHED.add("multi-tile scan")
    if kw.get("short"):
        _REACHED.add("too little room, route %d" % kw["route"])
    if kw["route"] == 1:
        _REACHED.add("g %d" % out["g"])
    if out["bps"] == 512:
        _REACHED.add("512 workgroups per source")


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_on_every_variant(ctx, name):
    case = cc.CASES[name]
    failures, seen = [], {}
    for variant in VARIANTS:
        if not applies(case, variant):
            continue
        out, cap = run(ctx, case, variant)
        bad = check(case, variant, out, cap)
        if VARIANTS[variant]["sort"] and not VARIANTS[variant].get("short"):       # both routes, every lane count: identical bytes
            digest = (out["row_start"].tobytes(), out["cand_meta"].tobytes(), out["cand_depths"].tobytes(), out["cursor"].tobytes())
            if seen.setdefault("sorted", digest) != digest:
                bad.append("differs from the first sorted variant")
        if bad:
            failures.append("%s: %s" % (variant, "; ".join(bad)))
        else:
            note(case, variant, out)
        _RAN.add((name, variant))
    assert not failures, "\n".join(failures)


def test_every_case_ran_and_every_branch_was_reached():
    assert _RAN == set(RUNS) and len(RUNS) >= len(cc.CASES) * (len(VARIANTS) - 2)
    want = {"k_exist_count", "k_exist_count_rt + k_exist_combine", "k_scan", "k_place", "k_place_rt", "k_exist_sort_runs", "register sort", "staged sort",
            "multi-tile scan", "too little room, route 0", "too little room, route 1", "512 workgroups per source"} | {"g %d" % g for g in (1, 2, 4, 8, 16, 32, 64)}
    assert want <= _REACHED, sorted(want - _REACHED)
