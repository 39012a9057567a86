"""The planes in the pipeline (Line3D.set_planes) on make_scene_boxes(32, 8, 6, seed 1): the object's planes equal capi.plane_lines_host applied to the
object's own getResult() lines, with tol computed in numpy by the stated rule (dist_px x the junctions' sigma) and the seeds taken from the junction
records of those lines (bit for bit, no golden needed), with the junctions option on and off; the device call on those inputs equals the host twin;
against the scene's true faces -- not set for set against tests/golden/planes_small.npz, whose lines are the oracle's: the device's end points may
differ from them by 1e-4, and some decisions of the rule lie closer to their thresholds than that -- the golden's three conditions hold; the option set
and then cleared gives the bytes of an object that never saw it; planes on with junctions off leaves the result's bytes alone and junctions() still
refuses; a reset keeps the setting; a node object gives the ordinary object's bytes; bad parameters are refused; the OBJ file parses back to each
plane's rectangle corners as the same doubles; and merging, refinement, junctions with snap, planes and support run together."""
import math

import numpy as np
import pytest

import junction_model as jm
import plane_cases as pc
import plane_model as pm

pytestmark = pytest.mark.gpu

COS10 = math.cos(10.0 * math.pi / 180.0)
KEYS = ("eligible_lines", "eligible_hypotheses", "hypothesis_edges", "components", "hypotheses_released", "candidates_dropped", "planes_found", "member_records")


@pytest.fixture(scope="module")
def scene():
    from line3d_amd.synth import make_scene_boxes
    return make_scene_boxes(32, 8, 6, seed=1)


def _run(scene, planes=None, junctions=None, devices=None, clear=False, merge=False, refine=False, support=False):
    from line3d_amd.pipeline import Line3D, load_scene
    l3d = Line3D("", matchingNeighbors=6, devices=devices) if devices is not None else Line3D("", matchingNeighbors=6)
    if junctions is not None:
        l3d.set_junctions(True, **junctions)
    if planes is not None:
        l3d.set_planes(True, **planes)
    if clear:
        l3d.set_planes(False)
    if merge:
        l3d.set_merging(True)
    if refine:
        l3d.set_refinement(True)
    if support:
        l3d.set_support(True)
    load_scene(l3d, scene)
    l3d.compute3Dmodel(False)
    return l3d


def _bytes(result):
    return [(tuple(s2), b"".join(a.tobytes() + b.tobytes() for a, b in s3)) for s2, s3 in result]


def _model_form(result):
    return [([(int(c), int(s)) for c, s in s2], np.array([list(a) + list(b) for a, b in s3], np.float64).reshape(-1, 6)) for s2, s3 in result]


def _inputs(scene, result, dist_px):
    """lines, tol and seeds of the object's own result by the stated rules, in numpy: the junctions' table (defaults), tol = dist_px x the junctions'
    sigma, the seeds = the L and T records of the junction search on that table, in record order"""
    from line3d_amd import capi
    views = {int(v["id"]): v for v in scene.views}
    form = _model_form(result)
    lines, jtol, ext = jm.result_table(form, views)
    rec = capi.junction_lines_host(lines, jtol, ext, cos_max=COS10)["records"]
    keep = (rec["where_i"] != jm.INTERIOR) | (rec["where_j"] != jm.INTERIOR)
    seeds = np.stack([rec["i"][keep], rec["j"][keep]], axis=1).astype(np.int32).reshape(-1, 2)
    tol = np.array([pm.line_tolerance(dist_px, jm.line_sigma(lines[k, :3], lines[k, 3:], m, views)) for k, (m, _) in enumerate(form)], np.float64)
    return lines, tol, seeds


@pytest.fixture(scope="module")
def runs(scene):
    """the result without the option; the object with planes and junctions (defaults); the object with planes alone, at 5 px"""
    from line3d_amd.capi import L3DError
    p = _run(scene)
    plain = p.getResult()
    with pytest.raises(L3DError):
        p.planes()
    p.close()
    both, alone = _run(scene, planes={}, junctions={}), _run(scene, planes=dict(dist_px=5.0))
    yield plain, both, alone
    both.close()
    alone.close()


def _same_as_host(l3d, scene, dist_px):
    from line3d_amd import capi
    lines, tol, seeds = _inputs(scene, l3d.getResult(), dist_px)
    exp = capi.plane_lines_host(lines, tol, seeds, cos_max=COS10, cos_min=COS10, min_lines=3)
    got = l3d.planes()
    assert got["planes"].tobytes() == exp["planes"].tobytes() and got["members"].tobytes() == exp["members"].tobytes() and len(exp["planes"]) >= 30
    assert [got[k] for k in KEYS] == exp["counts"].tolist()
    assert got["planes_per_line"].tolist() == np.bincount(exp["members"]["line"], minlength=len(lines)).tolist()
    return lines, tol, seeds, exp


def test_the_objects_planes_are_the_rule_on_its_own_lines(scene, runs):
    _same_as_host(runs[1], scene, 4.0)


def test_planes_without_junctions_leave_the_result_alone_and_junctions_still_refuses(scene, runs):
    from line3d_amd.capi import L3DError
    plain, both, alone = runs
    assert _bytes(alone.getResult()) == _bytes(plain) == _bytes(both.getResult())
    with pytest.raises(L3DError):
        alone.junctions()
    _same_as_host(alone, scene, 5.0)
    assert both.junctions()["vertices_found"] > 30


def test_the_device_call_on_the_objects_lines_equals_the_host_twin(gpu_ctx, scene, runs):
    lines, tol, seeds, exp = _same_as_host(runs[1], scene, 4.0)
    got = gpu_ctx.plane_lines(lines, tol, seeds, cos_max=COS10, cos_min=COS10, min_lines=3)
    assert pc.same(got, exp), pc.difference(got, exp)


def test_the_true_faces_are_recalled(scene, runs):
    """the golden's three conditions, against truth: at least 9 of 10 covered faces recalled, no plane's seeds mix boxes, the true corners of every
    recalled face within 1.0 x the largest member tolerance of its plane"""
    l3d = runs[1]
    result = l3d.getResult()
    lines, tol, _ = _inputs(scene, result, 4.0)
    views = {int(v["id"]): v for v in scene.views}
    edge_of = np.array([np.bincount([int(views[c]["gt"][s]) for c, s in m]).argmax() for m, _ in _model_form(result)], np.int32)
    fr = pm.face_recall(scene.corners, scene.corner_edges, edge_of, edge_of // 12, tol, l3d.planes())
    print("faces covered %d, recalled %d; planes whose seeds mix boxes %d; planes that match no face %d; corner distance %.3f x the largest member tolerance"
          % (len(fr["covered"]), len(fr["recalled"]), len(fr["mixed"]), len(fr["unmatched"]), fr["corner_ratio"]))
    assert len(fr["covered"]) >= 30 and 10 * len(fr["recalled"]) >= 9 * len(fr["covered"])
    assert not fr["mixed"]
    assert fr["corner_ratio"] <= 1.0


def test_option_set_then_cleared_gives_the_bytes_of_an_object_that_never_saw_it(scene, runs):
    from line3d_amd.capi import L3DError
    l3d = _run(scene, planes=dict(dist_px=6.0), clear=True)
    assert _bytes(l3d.getResult()) == _bytes(runs[0])
    with pytest.raises(L3DError):
        l3d.planes()
    with pytest.raises(L3DError):
        l3d.junctions()
    l3d.close()


def test_reset_keeps_the_setting(scene):
    from line3d_amd.pipeline import load_scene
    l3d = _run(scene, planes=dict(min_lines=4))
    want, wp = _bytes(l3d.getResult()), l3d.planes()
    l3d.reset()
    load_scene(l3d, scene)
    l3d.compute3Dmodel(False)
    got = l3d.planes()
    assert _bytes(l3d.getResult()) == want and got["planes"].tobytes() == wp["planes"].tobytes() and got["members"].tobytes() == wp["members"].tobytes()
    assert len(got["planes"]) > 0 and got["planes"]["n_lines"].min() >= 4
    l3d.close()


def test_node_object_gives_the_ordinary_objects_bytes(scene, runs):
    node = _run(scene, planes={}, junctions={}, devices=[0, 0])
    want, got = runs[1].planes(), node.planes()
    assert _bytes(node.getResult()) == _bytes(runs[1].getResult())
    assert got["planes"].tobytes() == want["planes"].tobytes() and got["members"].tobytes() == want["members"].tobytes()
    assert got["planes_per_line"].tolist() == want["planes_per_line"].tolist() and [got[k] for k in KEYS] == [want[k] for k in KEYS]
    node.close()


def test_parameters_are_checked(runs):
    from line3d_amd.capi import L3DError
    l3d = runs[1]
    for bad in (dict(dist_px=-1.0), dict(dist_px=float("inf")), dict(dist_px=float("nan")), dict(angle_deg=-1.0), dict(angle_deg=90.0), dict(angle_deg=float("nan")),
                dict(min_lines=1)):
        with pytest.raises(L3DError):
            l3d.set_planes(True, **bad)


def test_the_obj_file_parses_back_to_the_rectangles(runs, tmp_path):
    from line3d_amd.capi import L3DError
    l3d = runs[1]
    pl = l3d.planes()["planes"]
    path = str(tmp_path / "planes.obj")
    l3d.save3DPlanesAsOBJ(path)
    verts, groups, faces = [], [], []
    for ln in open(path).read().splitlines():
        f = ln.split()
        if f[0] == "v":
            verts.append([float(x) for x in f[1:4]])
        elif f[0] == "g":
            groups.append(f[1])
        elif f[0] == "f":
            faces.append([int(x) - 1 for x in f[1:]])
    verts = np.array(verts, np.float64).reshape(-1, 3)
    assert groups == ["plane_%d" % k for k in range(len(pl))] and faces == [[4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3] for k in range(len(pl))] and len(verts) == 4 * len(pl)
    for k, p in enumerate(pl):
        for e, (a, b) in enumerate(((p["rect"][0], p["rect"][2]), (p["rect"][1], p["rect"][2]), (p["rect"][1], p["rect"][3]), (p["rect"][0], p["rect"][3]))):
            want = ((p["c"] * p["N"]) + (a * p["u"])) + (b * p["v"])
            assert verts[4 * k + e].tobytes() == want.tobytes(), (k, e)
    with pytest.raises(L3DError):
        l3d.save3DPlanesAsOBJ(str(tmp_path / "no" / "such" / "folder.obj"))


def test_merging_refinement_junctions_with_snap_planes_and_support_together(scene):
    l3d = _run(scene, planes={}, junctions=dict(snap=True), merge=True, refine=True, support=True)
    result, j, p = l3d.getResult(), l3d.junctions(), l3d.planes()
    n = len(result)
    assert n == l3d.merging()["lines_after"] == len(l3d.refinement()["status"]) == len(l3d.support()["members_before"]) == len(j["vertex_P"]) == len(p["planes_per_line"])
    assert j["ends_moved"] > 0 and p["eligible_lines"] == n and p["eligible_hypotheses"] <= j["l_records"] + j["t_records"]
    assert p["planes_found"] == len(p["planes"]) > 20 and p["member_records"] == len(p["members"]) == int(p["planes_per_line"].sum()) == int(p["planes"]["n_lines"].sum())
    assert p["components"] - p["candidates_dropped"] == p["planes_found"] and p["members"]["line"].max() < n
    l3d.close()
