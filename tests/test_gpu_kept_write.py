"""The chains' kept writer (k_kept_write_chain: records, side words, run table, best positions, result record), the per-view seam call's writer behind its
scan, and the rebuild of side words and run tables from records, through l3d_test_kept_write on the crafted cases of tests/keptwrite_cases.py against
the plain model of tests/keptwrite_model.py.  Everything compared is an integer or a float that was copied or halved: bytes, no tolerance anywhere.
The whole arena comes back, so a record written outside the view's slice shows as a broken canary."""
import numpy as np
import pytest

import keptwrite_cases as kc
import keptwrite_model as km
from line3d_amd import capi

pytestmark = pytest.mark.gpu

VARIANTS = ("plain", "predecessor_exact_room", "arena_one_short", "candidate_overflow", "seam_writer")
SLACK = 8                   # records of room behind the list: canaries
_RAN, _REACHED = set(), set()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def call(ctx, what, case, **kw):
    try:
        return ctx.test_kept_write(case["N"], case["row_start"], case["meta"], case["depths"], case["conf"], km.kept_counts(case), case["l2g"], **kw)
    except capi.L3DError as e:          # a failing device call leaves nothing to compare, and nothing more is started on the device
        pytest.exit("%s: %s" % (what, e), 1)


def settings(case, variant):
    """-> the hook's keywords for the variant (None: the variant needs something the case does not have)"""
    total, R = int(km.kept_counts(case).sum()), int(case["row_start"][-1])
    if variant == "plain":
        return dict(arena_cap=total + SLACK, jobs=[None])
    if variant == "predecessor_exact_room":
        return dict(prev=(5, 3), arena_cap=8 + total, jobs=[None])
    if variant == "arena_one_short":
        return dict(prev=(5, 3), arena_cap=8 + total - 1, jobs=[None]) if total > 0 else None
    if variant == "candidate_overflow":
        return dict(cand_cap=R - 1, arena_cap=total + SLACK, jobs=[None]) if R > 0 else None
    return dict(writer=1, arena_cap=total + SLACK)


def diff(out, want, keys):
    bad = []
    for k in keys:
        a, b = out[k], want[k]
        same = a.tobytes() == b.tobytes() if isinstance(b, np.ndarray) else a == b
        if not same:
            where = ""
            if isinstance(b, np.ndarray) and a.shape == b.shape and len(b):
                av, bv = (a.view(np.uint8).reshape(len(a), -1), b.view(np.uint8).reshape(len(b), -1))
                rows = np.flatnonzero((av != bv).any(axis=1))
                where = " first at %d: %s / %s" % (rows[0], a[rows[0]], b[rows[0]])
            bad.append("%s differs%s" % (k, where if where else ": %s / %s" % (a, b)))
    return bad


RUNS = [(n, v) for n in kc.CASES for v in VARIANTS if settings(kc.CASES[n], v) is not None]


@pytest.mark.parametrize("name", list(kc.CASES))
def test_case_on_every_variant(ctx, name):
    case = kc.CASES[name]
    sizes = [int(case["row_start"][(y + 1) * case["N"]] - case["row_start"][y * case["N"]]) for y in range(case["S"])]
    failures, plain_records = [], None
    for variant in VARIANTS:
        kw = settings(case, variant)
        if kw is None:
            continue
        out = call(ctx, "%s / %s" % (name, variant), case, **kw)
        if variant == "seam_writer":
            total = int(km.kept_counts(case).sum())
            want = km.writer(case, arena_cap=kw["arena_cap"])
            bad = diff(out, want, ("records", "n_kept", "R"))
            # the other outputs are not the seam writer's: untouched
            if not ((out["side"] == 0xffffffff).all() and (out["rt"] == -1).all() and (out["best_pos"] == km.BESTPOS_CANARY).all()):
                bad.append("the seam writer wrote side words, a run table or best positions")
            if plain_records is not None and out["records"][:total].tobytes() != plain_records[:total].tobytes():
                bad.append("the two writers' records differ")
        else:
            want = km.writer(case, prev=kw.get("prev"), cand_cap=kw.get("cand_cap"), arena_cap=kw["arena_cap"])
            bad = diff(out, want, ("kept_base", "n_kept", "R", "overflow", "n_want", "records", "side", "rt", "best_pos"))
            # the rebuild of the list the writer just left: its side words and run table byte for byte, no error
            job, base, n = out["jobs"][0], want["kept_base"], want["n_kept"]
            if job["n"] != n or out["rebuild_err"] != 0:
                bad.append("rebuild: %d records, %d errors" % (job["n"], out["rebuild_err"]))
            elif not want["overflow"]:
                if job["qt"].tobytes() != want["side"][base:base + n].tobytes() or job["rt"].tobytes() != want["rt"].tobytes():
                    bad.append("the rebuilt side words or run table differ from the writer's")
            elif case["S"] and not (job["rt"] == 0).all():
                bad.append("the run table of an empty list is not all zero")
            if variant == "plain":
                plain_records = out["records"]
        if bad:
            failures.append("%s: %s" % (variant, "; ".join(bad)))
        else:
            _REACHED.add("k_kept_write + k_scan" if variant == "seam_writer" else "k_kept_write_chain")
            if variant != "seam_writer":
                _REACHED.add("rebuild of a written list")
                for bit in (1, 2):
                    if out["overflow"] == bit:
                        _REACHED.add("overflow bit %d" % bit)
                if not out["overflow"] and max(sizes + [0]) > kc.ROUND and out["n_kept"] > 0:
                    _REACHED.add("writer of several rounds")
                if not out["overflow"] and case["N"] > 64:
                    _REACHED.add("run-table prefix over several camera chunks")
                if not out["overflow"] and case["S"] > 256:
                    _REACHED.add("kept counts of more than 256 segments in front")
                if kw.get("prev") and not out["overflow"]:
                    _REACHED.add("slice behind a predecessor")
        _RAN.add((name, variant))
    assert not failures, "\n".join(failures)


def _tiny():
    return kc.CASES["confidence_edges"]


def test_several_lists_rebuilt_in_one_launch(ctx):
    """lists of 0, 1, 64, 65 and 1025 records, of different sizes and neighbour counts, as the jobs of one launch"""
    case = _tiny()
    out = call(ctx, "good lists", case, arena_cap=3 + SLACK, jobs=kc.GOOD_LISTS)
    assert out["rebuild_err"] == 0 and out["rebuild_blocks"] == 2
    for l, job in zip(kc.GOOD_LISTS, out["jobs"]):
        qt, rt, err = km.rebuild(l["records"], l["S"], l["l2g"])
        assert err == 0 and job["n"] == len(qt) and job["qt"].tobytes() == qt.tobytes() and job["rt"].tobytes() == rt.tobytes(), len(qt)
    _REACHED.add("several jobs in one launch")


@pytest.mark.parametrize("name", list(kc.BAD_LISTS))
def test_a_list_that_is_wrong_in_one_place_is_counted(ctx, name):
    """each crafted list on its own: one record whose camera is no neighbour, or one descent of the (segment, camera) order -- inside a wave, across
    waves, across workgroups, across the strides of the two passes.  The counter is what keeps every consumer from reading the rebuilt table."""
    l = kc.BAD_LISTS[name]
    out = call(ctx, name, _tiny(), arena_cap=3 + SLACK, jobs=[l])
    qt, rt, err = km.rebuild(l["records"], l["S"], l["l2g"])
    assert err == 1 and out["rebuild_err"] == err, (name, out["rebuild_err"])
    assert out["jobs"][0]["qt"].tobytes() == qt.tobytes()
    assert out["rebuild_blocks"] == (len(qt) + 1023) // 1024
    _REACHED.add("rebuild error: " + name)


def test_every_case_ran_and_every_branch_was_reached():
    assert _RAN == set(RUNS) and len(RUNS) >= len(kc.CASES) * 3
    want = {"k_kept_write_chain", "k_kept_write + k_scan", "rebuild of a written list", "overflow bit 1", "overflow bit 2", "writer of several rounds",
            "run-table prefix over several camera chunks", "kept counts of more than 256 segments in front", "slice behind a predecessor",
            "several jobs in one launch"} | {"rebuild error: " + n for n in kc.BAD_LISTS}
    assert want <= _REACHED, sorted(want - _REACHED)
