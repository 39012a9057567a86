"""The merging of duplicate lines in the pipeline (Line3D.set_merging) on make_scene(32, 100, 6, seed=11) against tests/golden/merge_small.npz, which the
oracle and the model of tests/merge_model.py made on the CPU (tests/golden/make_golden_merge.py): groups, member lists and order equal the golden
exactly, the 3-D segments within the tolerance tests/test_gpu_config2_golden.py uses for fitted lines (1e-4), at most two thirds of the lines remain, no
merged line mixes ground-truth ids, merging() is consistent with the two results, an object with the option set and cleared gives the bytes of one
that never saw it, reset keeps the setting, a node object gives the ordinary object's bytes, the refinement runs on the merged list, and the TXT
writer and project_result see it."""
import os

import numpy as np
import pytest

import merge_model as mm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_small.npz")
TOL = 1e-4
KINDS = {"plain": False, "rdd": True}


@pytest.fixture(scope="module")
def scene():
    from line3d_amd.synth import make_scene
    return make_scene(32, 100, 6, seed=11)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert g["scene"].tolist() == [32, 100, 6, 11]
    return g


def _run(scene, merge=None, diffusion=False, devices=None, clear=False, refine=False):
    from line3d_amd.pipeline import Line3D, load_scene
    l3d = Line3D("", matchingNeighbors=6, devices=devices) if devices is not None else Line3D("", matchingNeighbors=6)
    if merge is not None:
        l3d.set_merging(True, **merge)
    if clear:
        l3d.set_merging(False)
    if refine:
        l3d.set_refinement(True)
    load_scene(l3d, scene)
    l3d.compute3Dmodel(diffusion)
    return l3d


def _bytes(result):
    return [(tuple(s2), b"".join(a.tobytes() + b.tobytes() for a, b in s3)) for s2, s3 in result]


def _members(result):
    return [[(int(c), int(s)) for c, s in s2] for s2, _ in result]


def _golden_result(g, prefix):
    ids, io, pts, po = g[prefix + "_ids"], g[prefix + "_id_off"], g[prefix + "_pts"], g[prefix + "_pt_off"]
    return [([(int(c), int(s)) for c, s in ids[io[k]:io[k + 1]]], pts[po[k]:po[k + 1]]) for k in range(len(io) - 1)]


@pytest.fixture(scope="module")
def runs(scene):
    """per kind: the result without the option, and the object with it (defaults)"""
    out = {}
    for kind, diffusion in KINDS.items():
        p = _run(scene, diffusion=diffusion)
        plain = p.getResult()
        from line3d_amd.capi import L3DError
        with pytest.raises(L3DError):
            p.merging()
        p.close()
        out[kind] = (plain, _run(scene, merge={}, diffusion=diffusion))
    yield out
    for _, l3d in out.values():
        l3d.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_unmerged_result_is_the_goldens_starting_list(runs, golden, kind):
    """the order of the merged list follows from the order of this one"""
    assert _members(runs[kind][0]) == [m for m, _ in _golden_result(golden, kind + "_r0")]


@pytest.mark.parametrize("kind", list(KINDS))
def test_merged_result_equals_the_golden(runs, golden, scene, kind):
    plain, l3d = runs[kind]
    got, st = l3d.getResult(), l3d.merging()
    cnt = golden[kind + "_counts"].tolist()
    exp = _golden_result(golden, "%s_r%d" % (kind, cnt[2]))
    print(kind, {k: v for k, v in st.items() if not hasattr(v, "shape")}, "golden", cnt)
    assert _members(got) == [m for m, _ in exp], "groups, member lists and order"
    worst = 0.0
    for (_, s3), (_, e3) in zip(got, exp):
        assert len(s3) == len(e3)
        for (a, b), e in zip(s3, e3):
            worst = max(worst, float(np.abs(np.concatenate([a, b]) - e).max()))
    print("worst end point difference", worst)
    assert worst <= TOL
    assert [st[k] for k in ("lines_before", "lines_after", "rounds", "pairs_first_round", "groups_merged", "lines_released", "empty_refits")] == cnt[:7]
    assert st["final_index"].tolist() == golden[kind + "_final_index"].tolist() and st["n_sources"].tolist() == golden[kind + "_n_sources"].tolist()
    assert 3 * len(got) <= 2 * len(plain)
    views = {int(v["id"]): v for v in scene.views}
    for (s2, s3), ns in zip(got, st["n_sources"]):
        if ns > 1:
            assert len(set(int(views[int(c)]["gt"][int(s)]) for c, s in s2)) == 1, "a merged line mixes ground-truth ids"
            assert len(s3) == 1


@pytest.mark.parametrize("kind", list(KINDS))
def test_counts_and_final_index_are_consistent_with_the_two_results(runs, kind):
    plain, l3d = runs[kind]
    got, st = l3d.getResult(), l3d.merging()
    assert st["lines_before"] == len(plain) == len(st["final_index"]) and st["lines_after"] == len(got) == len(st["n_sources"])
    assert np.bincount(st["final_index"], minlength=len(got)).tolist() == st["n_sources"].tolist()
    assert np.all(np.diff([int(np.nonzero(st["final_index"] == k)[0][0]) for k in range(len(got))]) > 0), "a merged line stands where its lowest-index line stood"
    pm, pb, gb = _members(plain), _bytes(plain), _bytes(got)
    for k, m in enumerate(_members(got)):
        src = np.nonzero(st["final_index"] == k)[0]
        assert m == sorted(x for i in src for x in pm[i])
        if len(src) == 1:
            assert gb[k] == pb[src[0]], "a line that was not merged keeps its bytes"
    assert st["lines_before"] - st["lines_after"] == int((st["n_sources"] - 1).sum()) and 1 <= st["rounds"] <= 3


def test_the_first_round_is_merge_lines_on_the_unmerged_result(runs, golden, scene, gpu_ctx):
    plain = runs["plain"][0]
    views = {int(v["id"]): v for v in scene.views}
    lines = np.array([np.concatenate([s3[0][0], s3[-1][1]]) for _, s3 in plain])
    tol = np.array([mm.line_tol(lines[k, :3], lines[k, 3:], plain[k][0], views, 4.0) for k in range(len(plain))])
    out = gpu_ctx.merge_lines(lines, tol)
    assert out["pairs"].tolist() == golden["plain_r1_pairs"].tolist() and out["group"].tolist() == golden["plain_r1_group"].tolist()


def test_option_set_then_cleared_gives_the_bytes_of_an_object_that_never_saw_it(scene, runs):
    from line3d_amd.capi import L3DError
    l3d = _run(scene, merge={}, clear=True)
    assert _bytes(l3d.getResult()) == _bytes(runs["plain"][0])
    with pytest.raises(L3DError):
        l3d.merging()
    l3d.close()


def test_reset_keeps_the_setting(scene, runs):
    from line3d_amd.pipeline import load_scene
    l3d = runs["plain"][1]
    want = _bytes(l3d.getResult())
    l3d.reset()
    load_scene(l3d, scene)
    l3d.compute3Dmodel(False)
    assert _bytes(l3d.getResult()) == want and l3d.merging()["lines_after"] == len(want)


def test_node_object_gives_the_ordinary_objects_bytes(scene, runs):
    node = _run(scene, merge={}, devices=[0, 0])
    assert _bytes(node.getResult()) == _bytes(runs["plain"][1].getResult())
    assert node.merging()["final_index"].tolist() == runs["plain"][1].merging()["final_index"].tolist()
    node.close()


def test_refinement_runs_on_the_merged_list(scene, runs):
    l3d = _run(scene, merge={}, refine=True)
    got, ref = l3d.getResult(), l3d.refinement()
    assert _members(got) == _members(runs["plain"][1].getResult())
    assert len(ref["status"]) == len(got) == l3d.merging()["lines_after"]
    for li, ((_, s3), ns) in enumerate(zip(got, l3d.merging()["n_sources"])):
        if ns < 2:
            continue
        pts = np.array([p for a, b in s3 for p in (a, b)])
        far = np.linalg.norm(pts - pts[0], axis=1)
        j = int(np.argmax(far))
        d = (pts[j] - pts[0]) / far[j]
        assert np.linalg.norm(np.cross(pts - pts[0], d), axis=1).max() <= 1e-9 * far[j], "line %d: segments are collinear" % li
    l3d.close()


def test_parameters_reach_the_rule(scene, runs):
    """8 pixels merge at least as much as 4; one round stops after one"""
    wide = _run(scene, merge=dict(dist_px=8.0))
    one = _run(scene, merge=dict(max_rounds=1))
    base = runs["plain"][1].merging()
    assert wide.merging()["pairs_first_round"] >= base["pairs_first_round"] and wide.merging()["lines_after"] <= base["lines_after"]
    assert one.merging()["rounds"] == 1 and one.merging()["pairs_first_round"] == base["pairs_first_round"] and one.merging()["lines_after"] >= base["lines_after"]
    from line3d_amd.capi import L3DError
    for bad in (dict(dist_px=-1.0), dict(angle_deg=91.0), dict(max_gap=float("nan")), dict(max_rounds=0)):
        with pytest.raises(L3DError):
            wide.set_merging(True, **bad)
    wide.close()
    one.close()


def test_txt_writer_and_project_result_see_the_merged_list(runs, tmp_path):
    l3d = runs["plain"][1]
    result = l3d.getResult()
    path = str(tmp_path / "lines.txt")
    l3d.save3DLinesAsTXT(path)
    rows = [ln.split() for ln in open(path).read().splitlines()]
    assert len(rows) == len(result)
    for row, (s2, s3) in zip(rows, result):
        n = int(row[0])
        assert n == len(s3) and int(row[1 + 6 * n]) == len(s2)
        assert row[1:1 + 6 * n] == ["%g" % x for a, b in s3 for x in list(a) + list(b)]
    seg2d, seg_index, line_index, flags, start = l3d.project_result(view_ids=[0, 5], select="all")
    assert len(line_index) > 0 and line_index.max() < len(result) and seg_index.max() < sum(len(s3) for _, s3 in result)
    assert len(set(line_index[start[0]:start[1]].tolist())) > len(result) // 4
