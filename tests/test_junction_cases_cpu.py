"""The junction case tables (tests/junction_cases.py) on a machine without a GPU: every table is the case its name claims (asserted with the model of
tests/junction_model.py, the rules of include/line3d_amd.h "JUNCTIONS OF 3-D LINES" in numpy), the host entry point l3d_test_junction_lines_host --
the very functions the kernels run -- equals the model bit for bit on all of them (records, node_vertex, vertices, node_attach, counts), every refusal
comes with its code and cause, the host code is clean under AddressSanitizer and UBSan (tests/cpp/junction_asan.cpp), the Python mirrors of the
junction structs have the header's layout, the C++ facade's methods and the example driver compile, make_scene_boxes is deterministic and leaves
make_scene's bytes alone, and tests/golden/junction_small.npz is what the model gives on its own lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import junction_cases as jc
import junction_model as jm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = [c["name"] for c in jc.CASES]


def host(case):
    from line3d_amd import capi
    return capi.junction_lines_host(case["lines"], case["tol"], case["ext"], cos_max=case["cos_max"], crossings=case["crossings"])


def table_of(case):
    return [jm.prepare(case["lines"][k], case["tol"][k], case["ext"][k]) for k in range(len(case["lines"]))]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(name):
    case = jc.BY_NAME[name]
    m = jc.model_of(case)
    n = len(case["lines"])
    rec, nv, vert, att, counts = m["records"], m["node_vertex"], m["vertices"], m["node_attach"], m["counts"].tolist()
    kinds = jm.kinds_of(rec)
    pairs = list(zip(rec["i"].tolist(), rec["j"].tolist()))
    # what holds for every table
    assert all(i < j for i, j in pairs) and pairs == sorted(set(pairs))
    assert len(nv) == len(att) == 2 * n and counts[1:4] == [int((kinds == k).sum()) for k in range(3)] and counts[5] == len(vert)
    assert case["crossings"] or counts[3] == 0
    for k in range(len(vert)):
        nodes = np.nonzero(nv == k)[0]
        assert len(nodes) == vert["degree"][k] >= 2 and nodes[0] == vert["first_node"][k]
        assert len(set((nodes >> 1).tolist())) == len(nodes)                      # at most one end of a line stays in a vertex
    assert list(vert["first_node"]) == sorted(vert["first_node"])
    assert not np.any((nv >= 0) & (att >= 0)) and counts[7] == int((att >= 0).sum())
    for v in np.nonzero(att >= 0)[0]:
        r = rec[att[v]]
        assert kinds[att[v]] == jm.KIND_T and v in (2 * r["i"] + r["where_i"], 2 * r["j"] + r["where_j"])
    claim = case["claim"]
    if claim[0] == "size":
        assert n == claim[1] and counts[0] == n
        assert jc.chunks(n) == {1: 1, 2: 1, 64: 1, 65: 1, 256: 1, 257: 2, 300: 2, 513: 3}[n]
        if n >= 2:
            assert counts[1] >= max(1, n // 4) and counts[5] >= max(1, n // 8)
        if n >= 257:                                # a row block's lines pair with lines of a later tile
            assert any(j // 256 > i // 256 for i, j in pairs)
        if n == 513:                                # and with the third tile: the triangular skip starts each row block at its own tile
            assert any(j // 256 - i // 256 == 2 for i, j in pairs) and any(i >= 256 for i, j in pairs)
    elif claim[0] == "corner":
        assert counts == [3, 3, 0, 0, 1, 1, 0, 0] and vert["degree"][0] == 3 and nv.tolist() == [0, -1, 0, -1, 0, -1]
        assert m["rep"][0] == 2 and np.all(np.abs(vert["X"][0]) < 1e-15)
    elif claim[0] == "t":
        assert counts == [2, 0, 1, 0, 0, 0, 0, 1] and att.tolist() == [-1, -1, 0, -1] and (rec["where_i"][0], rec["where_j"][0]) == (jm.INTERIOR, jm.END_P)
        assert claim[1] == 2
    elif claim[0] == "x":
        assert counts == [2, 0, 0, claim[1], 0, 0, 0, 0]
        e = jm.pair_eval(*table_of(case), case["cos_max"])
        assert e is not None and e["kind"] == jm.KIND_X and e["g"] == 0.01
    elif claim[0] == "param":
        _, which, x0, n_rec, where = claim
        t = jm.pair_terms(*table_of(case))
        assert float(t[which]) == x0 and float(t["t" if which == "s" else "s"]) == 0.0 and t["g"] == 0 and len(rec) == n_rec
        if n_rec:
            assert rec["where_" + ("i" if which == "s" else "j")][0] == where and rec["where_" + ("j" if which == "s" else "i")][0] == jm.END_P
            assert kinds[0] == (jm.KIND_T if where == jm.INTERIOR else jm.KIND_L)
    elif claim[0] == "gap":
        t = jm.pair_terms(*table_of(case))
        assert float(t["g"]) == claim[1] and len(rec) == claim[2] and (float(t["g"]) <= max(case["tol"])) == bool(claim[2])
    elif claim[0] == "angle":
        t = jm.pair_terms(*table_of(case))
        assert float(t["b"]) == claim[1] and len(rec) == claim[2] == int(abs(claim[1]) <= case["cos_max"])
        if claim[2]:
            assert kinds[0] == jm.KIND_L
    elif claim[0] == "none":
        assert len(rec) == 0 and counts == [n, 0, 0, 0, 0, 0, 0, 0]
    elif claim[0] == "row":
        _, rep, stays, released = claim
        assert counts[:7] == [5, 4, 0, 0, 1, 1, len(released)] and len(set(m["comp"][[0, 2, 4, 6, 8]].tolist())) == 1
        assert all(m["rep"][v] == rep for v in (0, 2, 4, 6, 8))
        assert np.nonzero(nv == 0)[0].tolist() == stays and all(nv[v] == -1 for v in released)
        P = case["lines"][:, :3]
        assert np.linalg.norm(P[4] - P[0]) > 3 * case["tol"][0]                # the chain spans far more than tol
    elif claim[0] == "rep":
        t = table_of(case)
        assert len({float(t[v >> 1]["L"]) for v in claim[1]}) == 1
        assert all(m["rep"][v] == r for v, r in claim[1].items()) and counts[5] == 1 and vert["degree"][0] == len(claim[1])
    elif claim[0] == "attach":
        _, node, record, n_t = claim
        assert counts[2] == n_t and att[node] == record and counts[7] == 1
        gaps = rec["gap"][kinds == jm.KIND_T]
        assert (gaps[0] == gaps[1]) == (name == "attach_equal_gaps_the_lower_record_wins")
    elif claim[0] == "vertex_not_attached":
        assert counts == [3, 1, claim[1], 0, 1, 1, 0, 0] and nv.tolist() == [0, -1, 0, -1, -1, -1] and np.all(att == -1)
    elif claim[0] == "ineligible":
        t = table_of(case)
        for k in claim[1]:
            assert t[k] is None and k not in rec["i"] and k not in rec["j"] and nv[2 * k] == nv[2 * k + 1] == -1
            assert k // 256 == 0 and 64 <= k < 192
        assert counts[0] == n - len(claim[1]) and len(rec) > 0
    elif claim[0] == "dense":
        assert n == claim[1] and len(rec) == claim[2] == counts[1] and counts == [n, claim[2], 0, 0, 1, 1, 0, 0]
        assert vert["degree"][0] == n and np.bincount(rec["i"]).max() == n - 1 > 256
        assert np.abs(vert["X"][0] - case["lines"][0, :3]).max() < 1e-12
    elif claim[0] == "dense_x":
        assert n == claim[1] and len(rec) == claim[2] == counts[3] and counts == [n, 0, 0, claim[2], 0, 0, 0, 0]
    elif claim[0] == "far":
        assert np.abs(case["lines"]).min() > 0.99 * claim[1] and counts[1] > 16 and counts[5] > 8
    else:
        raise AssertionError(claim)


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model_bit_for_bit(name):
    case = jc.BY_NAME[name]
    got, exp = host(case), jc.model_of(case)
    assert jc.same(got, exp), (name, jc.difference(got, exp))


@pytest.mark.parametrize("name", [r[0] for r in jc.REFUSALS])
def test_refusals(name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in jc.REFUSALS if r[0] == name)
    kw = jc.refusal_arguments(overrides)
    with pytest.raises(capi.L3DError) as e:
        capi.junction_lines_host(kw["lines"], kw["tol"], kw["ext"], cos_max=kw["cos_max"], crossings=kw["crossings"])
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_null_pointers_are_refused_and_an_empty_table_is_fine():
    from line3d_amd import capi
    lib = capi.load_library()
    lines, tol, ext = jc.GOOD["lines"], jc.GOOD["tol"], jc.GOOD["ext"]
    prm = capi.junction_params(0.9)
    nv, na, counts = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(8, np.int32)
    rec, vert, nr, nvert = C.POINTER(capi.JunctionRecord)(), C.POINTER(capi.JunctionVertex)(), C.c_int(0), C.c_int(0)
    good = [capi._p(lines), capi._p(tol), capi._p(ext), C.c_int(2), C.byref(prm), C.byref(rec), C.byref(nr), capi._p(nv), C.byref(vert), C.byref(nvert), capi._p(na),
            capi._p(counts)]
    assert lib.l3d_test_junction_lines_host(*good) == 0
    assert nr.value == 1 and nvert.value == 1 and nv.tolist() == [0, -1, 0, -1] and na.tolist() == [-1] * 4 and counts.tolist() == [2, 1, 0, 0, 1, 1, 0, 0]
    assert (rec[0].i, rec[0].j, rec[0].where_i, rec[0].where_j, rec[0].gap) == (0, 1, 0, 0, 0.0) and (vert[0].first_node, vert[0].degree) == (0, 2)
    lib.l3d_free(rec)
    lib.l3d_free(vert)
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11):
        args = list(good)
        args[i] = None
        assert lib.l3d_test_junction_lines_host(*args) == 1, i
    lib.l3d_junction_last_error.restype = C.c_char_p
    assert b"null" in lib.l3d_junction_last_error()
    out = capi.junction_lines_host(np.zeros((0, 6)), np.zeros(0), np.zeros(0), cos_max=0.9)
    assert out["records"].shape == (0,) and out["vertices"].shape == (0,) and out["node_vertex"].shape == (0,) and out["node_attach"].shape == (0,)
    assert out["counts"].tolist() == [0] * 8


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/junction_asan.cpp: l3d_junction.hpp -- the argument checks, the table, the pair test, the components, the star rule, the vertices and
    the attachments -- and a main of its own, built with AddressSanitizer and UBSan"""
    exe = str(tmp_path / "junction_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "junction_asan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout, r.stdout


def test_facade_compiles(tmp_path):
    src = tmp_path / "facade_junctions.cpp"
    src.write_text('''#include "line3D_amd.hpp"
int use(L3D::Line3D& l)
{
    l.setJunctions();
    L3D::JunctionParams p;
    p.distPx = 6.0; p.extPx = 20.0; p.angleMinDeg = 15.0; p.maxExtRel = 0.3; p.snap = true;
    l.setJunctions(true, p);
    l.setJunctions(false);
    L3D::JunctionStats st;
    const bool a = l.getJunctions(st);
    const bool b = l.save3DLinesAsOBJ("wire.obj");
    int sum = (a ? 1 : 0) + (b ? 2 : 0) + st.eligibleLines + st.lRecords + st.tRecords + st.xRecords + st.components + st.nodesReleased + st.nodesAttached + st.endsMoved + st.movesSkipped;
    for (const L3D::JunctionVertex& v : st.vertices) sum += v.firstNode + v.degree + (int)v.X[0];
    return sum + (int)(st.vertexP.size() + st.vertexQ.size() + st.attachLineP.size() + st.attachLineQ.size());
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "main_vsfm_amd.cpp")])


def _digest(scene):
    import hashlib
    h = hashlib.sha256()
    for v in scene.views:
        for k in ("K", "R", "t", "segments", "gt"):
            h.update(np.ascontiguousarray(v[k]).tobytes())
    h.update(np.ascontiguousarray(scene.segs3d).tobytes())
    return h.hexdigest()


def test_make_scene_boxes_is_deterministic_and_leaves_make_scene_alone():
    from line3d_amd.synth import make_scene, make_scene_boxes
    # make_scene(8, 120, 6, seed=3), the smoke scene, as it was before make_scene_boxes existed
    assert _digest(make_scene(8, 120, 6, seed=3)) == "7f7abf7daf87a5cdbbb103ca80d8cbcc77b65fecf9fab54fbd7cc921c5fef368"
    a, b = make_scene_boxes(6, 3, 4, seed=2), make_scene_boxes(6, 3, 4, seed=2)
    assert _digest(a) == _digest(b) and a.corners.tobytes() == b.corners.tobytes() and _digest(a) != _digest(make_scene_boxes(6, 3, 4, seed=3))
    assert a.segs3d.shape == (36, 6) and a.corners.shape == (24, 3) and a.corner_edges.shape == (24, 3) and len(a.views) == 6
    assert np.abs(a.segs3d[:, [0, 2, 3, 5]]).max() <= 1.0 and np.abs(a.segs3d[:, [1, 4]]).max() <= 0.6          # inside make_scene's volume
    ends = a.segs3d.reshape(-1, 2, 3)
    for c, X in enumerate(a.corners):
        edges = a.corner_edges[c]
        assert len(set(edges.tolist())) == 3 and all(e // 12 == c // 8 for e in edges)
        d = []
        for e in edges:                                   # each of the three edges ends in the corner, and they are mutually perpendicular
            k = int(np.argmin(np.linalg.norm(ends[e] - X, axis=1)))
            assert np.array_equal(ends[e][k], X)
            d.append((ends[e][1 - k] - X) / np.linalg.norm(ends[e][1 - k] - X))
        assert max(abs(np.dot(d[0], d[1])), abs(np.dot(d[0], d[2])), abs(np.dot(d[1], d[2]))) < 1e-12
    for v in a.views:
        assert sorted(v["gt"].tolist()) == list(range(36)) and v["segments"].shape == (36, 4) and len(v["sims"]) >= 2
    assert np.bincount(a.corner_edges.reshape(-1), minlength=36).tolist() == [2] * 36


def test_the_golden_is_what_its_generator_says():
    """the model on the golden's own lines gives the golden's junctions; the share of the corners it recalls is the condition the generator set"""
    g = np.load(os.path.join(HERE, "golden", "junction_small.npz"))
    out = jm.junctions(g["lines"], g["tol"], g["ext"], jc.COS10)
    assert out["records"].tobytes() == g["records"].tobytes() and out["vertices"].tobytes() == g["vertices"].tobytes()
    assert out["node_vertex"].tolist() == g["node_vertex"].tolist() and out["node_attach"].tolist() == g["node_attach"].tolist() and out["counts"].tolist() == g["counts"].tolist()
    assert float(g["margin"]) > 1e-3 and 10 * len(g["recalled"]) >= 8 * len(g["covered"]) and len(g["covered"]) >= 56
    from line3d_amd import capi
    got = capi.junction_lines_host(g["lines"], g["tol"], g["ext"], cos_max=jc.COS10)
    assert jc.same(got, out), jc.difference(got, out)


def test_struct_layout_and_symbols(tmp_path):
    from line3d_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\n'
                   '#define O(t, f) (int)offsetof(t, f)\n'
                   'int main(void) {\n'
                   '  printf("%d %d %d %d\\n", (int)sizeof(l3d_junction_params), O(l3d_junction_params, cos_max), O(l3d_junction_params, crossings), O(l3d_junction_params, pad));\n'
                   '  printf("%d %d %d %d %d %d %d %d %d\\n", (int)sizeof(l3d_junction_record), O(l3d_junction_record, i), O(l3d_junction_record, j), O(l3d_junction_record, where_i),\n'
                   '         O(l3d_junction_record, where_j), O(l3d_junction_record, s), O(l3d_junction_record, t), O(l3d_junction_record, gap), O(l3d_junction_record, X));\n'
                   '  printf("%d %d %d %d\\n", (int)sizeof(l3d_junction_vertex), O(l3d_junction_vertex, X), O(l3d_junction_vertex, first_node), O(l3d_junction_vertex, degree));\n'
                   '  printf("%d %d %d\\n", L3D_JUNCTION_END_P, L3D_JUNCTION_END_Q, L3D_JUNCTION_INTERIOR);\n'
                   '  return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True).stdout.splitlines()]

    def layout(struct, dtype):
        assert C.sizeof(struct) == dtype.itemsize and all(getattr(struct, f).offset == dtype.fields[f][1] for f in dtype.names)
        return [C.sizeof(struct)] + [getattr(struct, f[0]).offset for f in struct._fields_]

    P = capi.JunctionParams
    assert got[0] == [C.sizeof(P), P.cos_max.offset, P.crossings.offset, P.pad.offset] == [16, 0, 8, 12], got[0]
    assert got[1] == layout(capi.JunctionRecord, capi.JUNCTION_RECORD) and got[1][0] == 64, got[1]
    assert got[2] == layout(capi.JunctionVertex, capi.JUNCTION_VERTEX) and got[2][0] == 32, got[2]
    assert got[3] == [capi.JUNCTION_END_P, capi.JUNCTION_END_Q, capi.JUNCTION_INTERIOR] == [jm.END_P, jm.END_Q, jm.INTERIOR]
    assert capi.JUNCTION_RECORD == jm.RECORD and capi.JUNCTION_VERTEX == jm.VERTEX
    lib = capi.load_library()
    missing = [s for s in ("l3d_junction_lines", "l3d_test_junction_lines_host", "l3d_junction_last_error", "l3d_line3d_set_junctions", "l3d_line3d_get_junctions",
                           "l3d_line3d_save_wireframe") if not hasattr(lib, s)]
    assert not missing, missing
    names = lib.l3d_profile_names().decode().split(";")
    for k in ("junc_prepare", "junc_count", "junc_scan", "junc_write", "junc_cc_init", "junc_cc_hook", "junc_cc_compress", "junc_rep", "junc_star", "junc_flag",
              "junc_vscan", "junc_keys", "junc_sort", "junc_vertex", "junc_attach", "junc_finish"):
        assert k in names, k
    p = capi.junction_params()
    assert p.cos_max == jc.COS10 and p.crossings == 0
