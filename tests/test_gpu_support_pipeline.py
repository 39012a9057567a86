"""The support of the result's lines in the pipeline (Line3D.gather_support, Line3D.set_support) on make_scene(32, 100, 6, seed=11): gather_support equals the
model of tests/support_model.py run on the object's own result and views, bit for bit; with set_support on, the first members of every line are the old
members in their old order, the added ones are exactly the model's, no 2-D segment is in two lines and the 3-D segments are byte-equal to a run with
it off; an object with the option set and cleared gives the bytes of one that never saw it; the OBSERVED selection of a view that had no member of
some line now includes that line; with merging and refinement on, the support runs last, on their result; reset keeps the setting."""
import numpy as np
import pytest

import support_cases as sc
import support_model as sm

pytestmark = pytest.mark.gpu

P = dict(dist_px=3.0, cos_min=sc.COS5, min_overlap=0.5, near=1e-6, margin=3.0)       # the defaults of gather_support and set_support


@pytest.fixture(scope="module")
def scene():
    from line3d_amd.synth import make_scene
    return make_scene(32, 100, 6, seed=11)


def _views(scene):
    return {int(v["id"]): ((np.asarray(v["K"], np.float64), np.asarray(v["R"], np.float64), np.asarray(v["t"], np.float64), int(v["width"]), int(v["height"])),
                           np.asarray(v["segments"], np.float32).reshape(-1, 4)) for v in scene.views}


def _run(scene, support=None, clear=False, merge=False, refine=False):
    from line3d_amd.pipeline import Line3D, load_scene
    l3d = Line3D("", matchingNeighbors=6)
    if support is not None:
        l3d.set_support(True, **support)
    if clear:
        l3d.set_support(False)
    if merge:
        l3d.set_merging(True)
    if refine:
        l3d.set_refinement(True)
    load_scene(l3d, scene)
    l3d.compute3Dmodel(False)
    return l3d


def _bytes(result):
    return [(tuple(s2), b"".join(a.tobytes() + b.tobytes() for a, b in s3)) for s2, s3 in result]


def _members(result):
    return [[(int(c), int(s)) for c, s in s2] for s2, _ in result]


def _lines(result):
    """getResult() as the model's input: members, and the 3-D segments as (k, 6)"""
    return [([(int(c), int(s)) for c, s in s2], np.array([np.concatenate([a, b]) for a, b in s3], np.float64).reshape(-1, 6)) for s2, s3 in result]


def _same_gather(got, exp):
    return (got["records"].dtype == sm.LINE_RECORD and got["records"].tobytes() == exp["records"].tobytes() and got["line_start"].tolist() == exp["line_start"].tolist()
            and got["line_views"].tolist() == exp["line_views"].tolist() and got["counts"].tolist() == exp["counts"].tolist())


@pytest.fixture(scope="module")
def runs(scene):
    """off: an object that never saw the option, with its result and the model's gather on it; on: the object with the option (defaults)"""
    off = _run(scene)
    plain = off.getResult()
    model = sm.gather(_lines(plain), _views(scene), **P)
    on = _run(scene, support={})
    yield dict(off=off, plain=plain, model=model, on=on, views=_views(scene))
    off.close()
    on.close()


def test_gather_support_equals_the_model_on_the_objects_own_result(runs):
    from line3d_amd import capi
    got, exp = runs["off"].gather_support(), runs["model"]
    n = len(runs["plain"])
    print("lines %d, records %d, members found again %d, not found %d, segments on a line and members of none %d; views with a member median %g, with a record median %g / min %d"
          % (n, *got["counts"].tolist(), np.median(got["line_views"][:, 0]), np.median(got["line_views"][:, 1]), got["line_views"][:, 1].min()))
    assert capi.LINE_SUPPORT == sm.LINE_RECORD and capi.LINE_SUPPORT.itemsize == 24
    assert _same_gather(got, exp)
    assert got["counts"][1] >= 0.95 * sum(len(m) for m, _ in _lines(runs["plain"])) and np.median(got["line_views"][:, 1]) >= 4 * np.median(got["line_views"][:, 0])
    # the same through explicit parameters, and other parameters give another answer that is the model's again
    assert _same_gather(runs["off"].gather_support(dist_px=3.0, angle_deg=5.0, min_overlap=0.5, near_z=1e-6), exp)
    q = dict(P, dist_px=2.0, margin=2.0)
    other = runs["off"].gather_support(capi.support_params(dist_px=2.0, cos_min=sc.COS5, min_overlap=0.5, near_z=1e-6, margin=2.0))
    assert other["counts"][0] < got["counts"][0] and _same_gather(other, sm.gather(_lines(runs["plain"]), runs["views"], **q))


def test_gather_does_not_change_the_result(runs):
    assert _bytes(runs["off"].getResult()) == _bytes(runs["plain"])


def test_with_the_option_on_the_member_lists_are_extended_by_exactly_the_models_records(runs):
    plain, model, on = runs["plain"], runs["model"], runs["on"]
    got = on.getResult()
    assert len(got) == len(plain)
    before, after = _members(plain), _members(got)
    n_added = 0
    for k in range(len(plain)):
        assert after[k][:len(before[k])] == before[k], "the old members, in their old order, come first"
        assert after[k][len(before[k]):] == model["added"][k] == sorted(model["added"][k]), "the added members are the model's, in (view id, segment) order"
        n_added += len(model["added"][k])
    assert n_added > sum(len(m) for m in before), "the support more than doubles the observations of this scene"
    every = [key for m in after for key in m]
    assert len(every) == len(set(every)), "a 2-D segment is in two lines"
    assert [b for _, b in _bytes(got)] == [b for _, b in _bytes(plain)], "the 3-D segments are untouched"


def test_support_reports_what_the_finish_recorded(runs):
    from line3d_amd import capi
    plain, model, on = runs["plain"], runs["model"], runs["on"]
    st = on.support()
    assert [st[k] for k in ("records", "members_found", "members_not_found", "segments_unclaimed")] == model["counts"].tolist()
    assert st["members_before"].tolist() == [len(m) for m in _members(plain)] and st["members_added"].tolist() == [len(a) for a in model["added"]]
    after = _members(on.getResult())
    assert st["views_before"].tolist() == model["line_views"][:, 0].tolist() and st["views_after"].tolist() == [len({c for c, _ in m}) for m in after]
    # (the duplicate lines of an edge share its segments -- each goes to the line that holds its best row -- so the views per line grow less than the
    # views with a record do; no line loses a view)
    print("views with a member per line, median: %g before, %g after" % (np.median(st["views_before"]), np.median(st["views_after"])))
    assert np.all(st["views_after"] >= st["views_before"]) and st["views_after"].sum() > st["views_before"].sum()
    with pytest.raises(capi.L3DError, match="without the support"):
        runs["off"].support()
    # a gather on the extended result: every added member is now a member that is found again, and nothing is left to add
    again = on.gather_support()
    assert again["counts"][1] == model["counts"][1] + sum(len(a) for a in model["added"]) and not np.any(again["records"]["flags"] == 4)


def test_set_and_cleared_gives_the_bytes_of_an_object_that_never_saw_it(scene, runs):
    c = _run(scene, support=dict(dist_px=5.0), clear=True)
    try:
        assert _bytes(c.getResult()) == _bytes(runs["plain"])
    finally:
        c.close()


def test_observed_selection_sees_the_added_views(runs):
    plain, on, off = runs["plain"], runs["on"], runs["off"]
    before, after = _members(plain), _members(on.getResult())
    line, view = next((k, c) for k in range(len(plain)) for c, _ in after[k][len(before[k]):] if c not in {v for v, _ in before[k]})
    old = off.project_result(view_ids=[view], select="observed", margin=3.0)         # (the margin of the support: the line's row exists in this view)
    new = on.project_result(view_ids=[view], select="observed", margin=3.0)
    assert line not in old[2].tolist() and line in new[2].tolist()
    assert set(old[2].tolist()) < set(new[2].tolist())


def test_the_support_runs_last_behind_merging_and_refinement(scene):
    base = _run(scene, merge=True, refine=True)
    both = _run(scene, support={}, merge=True, refine=True)
    try:
        want, got = base.getResult(), both.getResult()
        assert [b for _, b in _bytes(got)] == [b for _, b in _bytes(want)], "the merged, refined 3-D segments are what they were"
        model = sm.gather(_lines(want), _views(scene), **P)
        bm, am = _members(want), _members(got)
        for k in range(len(want)):
            assert am[k][:len(bm[k])] == bm[k] and am[k][len(bm[k]):] == model["added"][k]
        assert both.support()["records"] == model["counts"][0] and both.merging()["lines_after"] == len(got) and len(both.refinement()["status"]) == len(got)
    finally:
        base.close()
        both.close()


def test_refusals_and_reset(scene):
    from line3d_amd import capi
    from line3d_amd.pipeline import Line3D, load_scene
    l3d = Line3D("", matchingNeighbors=6)
    try:
        with pytest.raises(capi.L3DError, match="no result yet"):
            l3d.gather_support()
        for bad in (dict(dist_px=-1.0), dict(dist_px=float("nan")), dict(angle_deg=91.0), dict(min_overlap=1.5), dict(min_overlap=float("nan"))):
            with pytest.raises(capi.L3DError, match="set_support"):
                l3d.set_support(True, **bad)
        l3d.set_support(True)
        l3d.reset()                                         # keeps the setting
        load_scene(l3d, scene)
        l3d.compute3Dmodel(False)
        assert l3d.support()["records"] > 0
        with pytest.raises(capi.L3DError, match="cos_min"):
            l3d.gather_support(capi.support_params(cos_min=1.5))
    finally:
        l3d.close()
