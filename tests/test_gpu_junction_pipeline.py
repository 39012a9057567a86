"""The junctions in the pipeline (Line3D.set_junctions) on make_scene_boxes(32, 8, 6, seed of the golden): the object's junctions equal
capi.junction_lines_host applied to the object's own getResult() lines with tol / ext computed in numpy by the stated rule (bit for bit, no golden
needed); against tests/golden/junction_small.npz, which the oracle and the model of tests/junction_model.py made on the CPU
(tests/golden/make_golden_junctions.py; no decision of the rule on its lines lies within 1e-3 of its threshold, so the 1e-4 the device's end points may
differ by cannot flip one): vertex memberships and attachments equal, positions within 1e-4, the golden's own corners recalled, no vertex joins lines
of different boxes; the option set and cleared gives the bytes of an object that never saw it, reset keeps the setting, a node object gives the ordinary
object's bytes; with snap every moved end lies on its line's previous axis, the other lines keep their bytes and the 2-D members do not change; the
OBJ file parses back to the result's doubles with node_vertex as its shared indices; and merging, refinement, support and junctions run together."""
import math
import os

import numpy as np
import pytest

import junction_model as jm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "junction_small.npz")
TOL = 1e-4
COS10 = math.cos(10.0 * math.pi / 180.0)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert g["scene"].tolist()[:3] == [32, 8, 6]
    return g


@pytest.fixture(scope="module")
def scene(golden):
    from line3d_amd.synth import make_scene_boxes
    return make_scene_boxes(32, 8, 6, seed=int(golden["scene"][3]))


def _run(scene, junctions=None, devices=None, clear=False, merge=False, refine=False, support=False):
    from line3d_amd.pipeline import Line3D, load_scene
    l3d = Line3D("", matchingNeighbors=6, devices=devices) if devices is not None else Line3D("", matchingNeighbors=6)
    if junctions is not None:
        l3d.set_junctions(True, **junctions)
    if clear:
        l3d.set_junctions(False)
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


def _members(result):
    return [[(int(c), int(s)) for c, s in s2] for s2, _ in result]


def _model_form(result):
    return [(m, np.array([list(a) + list(b) for a, b in s3], np.float64).reshape(-1, 6)) for m, (_, s3) in zip(_members(result), result)]


def _per_line(out, n):
    """(vertex of P, vertex of Q, line P rests on, line Q rests on) from a junction_lines result"""
    per = np.full((n, 4), -1, np.int32)
    for l in range(n):
        for e in (0, 1):
            per[l, e] = out["node_vertex"][2 * l + e]
            a = out["node_attach"][2 * l + e]
            if a >= 0:
                r = out["records"][a]
                per[l, 2 + e] = r["j"] if r["i"] == l else r["i"]
    return per


def _got_per_line(j):
    return np.stack([j["vertex_P"], j["vertex_Q"], j["attach_line_P"], j["attach_line_Q"]], axis=1)


@pytest.fixture(scope="module")
def runs(scene):
    """the result without the option, and the object with it (defaults)"""
    from line3d_amd.capi import L3DError
    p = _run(scene)
    plain = p.getResult()
    with pytest.raises(L3DError):
        p.junctions()
    p.close()
    on = _run(scene, junctions={})
    yield plain, on
    on.close()


@pytest.fixture(scope="module")
def host_twin(scene, runs):
    """capi.junction_lines_host on the object's own lines, tol and ext by the stated rule in numpy"""
    from line3d_amd import capi
    result = runs[1].getResult()
    views = {int(v["id"]): v for v in scene.views}
    lines, tol, ext = jm.result_table(_model_form(result), views)
    return lines, tol, ext, capi.junction_lines_host(lines, tol, ext, cos_max=COS10)


def test_without_snap_the_result_keeps_its_bytes(runs):
    assert _bytes(runs[1].getResult()) == _bytes(runs[0])


def test_the_objects_junctions_are_the_rule_on_its_own_lines(runs, host_twin):
    _, l3d = runs
    lines, tol, ext, exp = host_twin
    got = l3d.junctions()
    n = len(lines)
    assert got["vertices"].tobytes() == exp["vertices"].tobytes() and len(exp["vertices"]) > 30
    assert _got_per_line(got).tolist() == _per_line(exp, n).tolist()
    keys = ("eligible_lines", "l_records", "t_records", "x_records", "components", "vertices_found", "nodes_released", "nodes_attached")
    assert [got[k] for k in keys] == exp["counts"].tolist() and got["ends_moved"] == got["moves_skipped"] == 0


def test_the_device_call_on_the_objects_lines_equals_the_host_twin(gpu_ctx, host_twin):
    import junction_cases as jc
    lines, tol, ext, exp = host_twin
    got = gpu_ctx.junction_lines(lines, tol, ext, cos_max=COS10)
    assert jc.same(got, exp), jc.difference(got, exp)


def _to_golden(result, golden):
    """the index in the golden of every line of the result, by its 2-D members"""
    ids, io = golden["ids"], golden["id_off"]
    where = {tuple(sorted((int(c), int(s)) for c, s in ids[io[k]:io[k + 1]])): k for k in range(len(io) - 1)}
    assert len(where) == len(io) - 1
    return [where[tuple(sorted(m))] for m in _members(result)]


def test_against_the_golden(runs, golden):
    _, l3d = runs
    result, got = l3d.getResult(), l3d.junctions()
    to_g = _to_golden(result, golden)
    n = len(result)
    assert sorted(to_g) == list(range(n)) and n == len(golden["lines"])
    worst = max(float(np.abs(np.concatenate([s3[0][0], s3[-1][1]]) - golden["lines"][to_g[k]]).max()) for k, (_, s3) in enumerate(result))
    print("worst end point difference to the oracle's lines", worst)
    assert worst <= TOL
    per, gper = _got_per_line(got), golden["per_line"]
    # memberships: the same sets of (golden line, end) per vertex; attachments: the same line per end
    sets = lambda per_v, name: {frozenset((name(l), e) for l in range(n) for e in (0, 1) if per_v[l, e] == k) for k in range(int(per_v[:, :2].max()) + 1)}
    assert sets(per, lambda l: to_g[l]) == sets(gper, lambda l: l)
    for l in range(n):
        for e in (2, 3):
            assert (to_g[per[l, e]] if per[l, e] >= 0 else -1) == gper[to_g[l], e]
    assert [got[k] for k in ("l_records", "t_records", "x_records", "components", "vertices_found", "nodes_released", "nodes_attached")] == golden["counts"].tolist()[1:]
    # positions: a vertex is named by its members
    gpos = {frozenset((l, e) for l in range(n) for e in (0, 1) if gper[l, e] == k): golden["vertices"]["X"][k] for k in range(len(golden["vertices"]))}
    worst = 0.0
    for k in range(len(got["vertices"])):
        key = frozenset((to_g[l], e) for l in range(n) for e in (0, 1) if per[l, e] == k)
        worst = max(worst, float(np.abs(got["vertices"]["X"][k] - gpos[key]).max()))
    print("worst vertex position difference", worst)
    assert worst <= TOL


def test_the_goldens_corners_are_recalled_and_no_vertex_mixes_boxes(runs, golden, scene, host_twin):
    _, l3d = runs
    lines, tol, ext, _ = host_twin
    result, got = l3d.getResult(), l3d.junctions()
    views = {int(v["id"]): v for v in scene.views}
    node_vertex = _got_per_line(got)[:, :2].reshape(-1)
    covered, recalled, line_box = jm.corner_recall(scene, _model_form(result), views, lines, tol, ext, node_vertex)
    print("corners covered %d, recalled %d" % (len(covered), len(recalled)))
    assert covered == golden["covered"].tolist() and recalled == golden["recalled"].tolist() and 10 * len(recalled) >= 8 * len(covered)
    for k in range(len(got["vertices"])):
        assert len({int(line_box[v >> 1]) for v in np.nonzero(node_vertex == k)[0]}) == 1, "vertex %d joins lines of different boxes" % k


def test_option_set_then_cleared_gives_the_bytes_of_an_object_that_never_saw_it(scene, runs):
    from line3d_amd.capi import L3DError
    l3d = _run(scene, junctions=dict(snap=True), clear=True)
    assert _bytes(l3d.getResult()) == _bytes(runs[0])
    with pytest.raises(L3DError):
        l3d.junctions()
    l3d.close()


def test_node_object_gives_the_ordinary_objects_bytes(scene, runs):
    node = _run(scene, junctions={}, devices=[0, 0])
    want = runs[1].junctions()
    got = node.junctions()
    assert _bytes(node.getResult()) == _bytes(runs[1].getResult())
    assert got["vertices"].tobytes() == want["vertices"].tobytes() and _got_per_line(got).tolist() == _got_per_line(want).tolist()
    node.close()


def test_parameters_are_checked(runs):
    from line3d_amd.capi import L3DError
    l3d = runs[1]
    for bad in (dict(dist_px=-1.0), dict(ext_px=float("inf")), dict(angle_min_deg=0.0), dict(angle_min_deg=91.0), dict(max_ext_rel=0.6), dict(max_ext_rel=float("nan"))):
        with pytest.raises(L3DError):
            l3d.set_junctions(True, **bad)


@pytest.fixture(scope="module")
def snapped(scene):
    l3d = _run(scene, junctions=dict(snap=True))
    yield l3d
    l3d.close()


def test_snap_moves_ends_along_their_own_axes(runs, snapped, host_twin):
    plain, _ = runs
    lines, tol, ext, exp = host_twin
    result, got = snapped.getResult(), snapped.junctions()
    assert _members(result) == _members(plain), "the 2-D members do not change"
    assert _got_per_line(got).tolist() == _per_line(exp, len(lines)).tolist() and got["vertices"].tobytes() == exp["vertices"].tobytes()
    pb, gb = _bytes(plain), _bytes(result)
    moved = 0
    for l, ((_, s3), (_, p3)) in enumerate(zip(result, plain)):
        touched = [e for e in (0, 1) if got["vertex_P" if e == 0 else "vertex_Q"][l] >= 0 or got["attach_line_P" if e == 0 else "attach_line_Q"][l] >= 0]
        if not touched:
            assert gb[l] == pb[l], "a line without a junction keeps its bytes"
            continue
        P, Q = lines[l, :3], lines[l, 3:]
        L = np.linalg.norm(Q - P)
        d = (Q - P) / L
        for e in (0, 1):
            new, old = (s3[0][0], p3[0][0]) if e == 0 else (s3[-1][1], p3[-1][1])
            if e not in touched:
                assert new.tobytes() == old.tobytes()
                continue
            moved += int(new.tobytes() != old.tobytes())
            off = (new - P) - np.dot(new - P, d) * d
            assert np.linalg.norm(off) <= 1e-12 * L, "line %d end %d left its axis" % (l, e)
        inner = [(a.tobytes(), b.tobytes()) for a, b in s3]
        assert inner[0][1] == p3[0][1].tobytes() or len(s3) == 1
        assert [x for x in inner[1:-1]] == [(a.tobytes(), b.tobytes()) for a, b in p3[1:-1]]
    new, n_moved, n_skipped = jm.snap_result(_model_form(plain), lines, exp)
    assert (got["ends_moved"], got["moves_skipped"]) == (n_moved, n_skipped) and moved <= n_moved and n_moved > 60
    assert b"".join(s.tobytes() for _, s in new) == b"".join(a.tobytes() + b.tobytes() for _, s3 in result for a, b in s3), "the model's snapped result, bit for bit"


def test_reset_keeps_the_setting(scene, snapped):
    from line3d_amd.pipeline import load_scene
    want, wj = _bytes(snapped.getResult()), snapped.junctions()
    snapped.reset()
    load_scene(snapped, scene)
    snapped.compute3Dmodel(False)
    got = snapped.junctions()
    assert _bytes(snapped.getResult()) == want and got["vertices"].tobytes() == wj["vertices"].tobytes() and got["ends_moved"] == wj["ends_moved"] > 0


def _parse_obj(path):
    verts, groups = [], []
    for ln in open(path).read().splitlines():
        f = ln.split()
        if f[0] == "v":
            verts.append([float(x) for x in f[1:4]])
        elif f[0] == "g":
            groups.append((f[1], []))
        elif f[0] == "l":
            groups[-1][1].append((int(f[1]) - 1, int(f[2]) - 1))
    return np.array(verts, np.float64).reshape(-1, 3), groups


@pytest.mark.parametrize("which", ["on", "snapped", "off"])
def test_the_obj_file_parses_back_to_the_result(scene, runs, snapped, tmp_path, which):
    l3d = {"on": runs[1], "snapped": snapped}.get(which) or _run(scene)
    result = l3d.getResult()
    j = l3d.junctions() if which != "off" else None
    nv = len(j["vertices"]) if j else 0
    path = str(tmp_path / "wire.obj")
    l3d.save3DLinesAsOBJ(path)
    verts, groups = _parse_obj(path)
    assert [g for g, _ in groups] == ["line_%d" % k for k in range(len(result))]
    if j:
        assert verts[:nv].tobytes() == j["vertices"]["X"].tobytes()
    own = 0
    for l, ((_, s3), (_, els)) in enumerate(zip(result, groups)):
        assert len(els) == len(s3)
        for k, ((a, b), (ia, ib)) in enumerate(zip(s3, els)):
            for e, (p, idx) in enumerate(((a, ia), (b, ib))):
                shared = j["vertex_P" if e == 0 else "vertex_Q"][l] if j and ((e == 0 and k == 0) or (e == 1 and k == len(s3) - 1)) else -1
                if shared >= 0:
                    assert idx == shared, "the shared indices are exactly node_vertex"
                else:
                    assert idx >= nv and verts[idx].tobytes() == np.asarray(p, np.float64).tobytes()
                    own += 1
    assert len(verts) == nv + own
    if which == "off":
        l3d.close()


def test_merging_refinement_support_and_junctions_together(scene):
    l3d = _run(scene, junctions=dict(snap=True), merge=True, refine=True, support=True)
    result, j = l3d.getResult(), l3d.junctions()
    n = len(result)
    assert n == l3d.merging()["lines_after"] == len(l3d.refinement()["status"]) == len(l3d.support()["members_before"]) == len(j["vertex_P"])
    assert j["eligible_lines"] == n and j["vertices_found"] == len(j["vertices"]) > 20
    per = _got_per_line(j)
    assert per[:, :2].max() == len(j["vertices"]) - 1 and per[:, 2:].max() < n
    assert np.bincount(per[:, :2][per[:, :2] >= 0]).tolist() == j["vertices"]["degree"].tolist()
    l3d.close()
