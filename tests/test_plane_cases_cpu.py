"""The plane case tables (tests/plane_cases.py) on a machine without a GPU: every table is the case its name claims (asserted with the model of
tests/plane_model.py, the rules of include/line3d_amd.h "PLANES OF 3-D LINES" in numpy), the host entry point l3d_test_plane_lines_host -- the very
functions the kernels run -- equals the model bit for bit on all of them (planes, members, hyp_plane, counts), every refusal comes with its code and
cause, the host code is clean under AddressSanitizer and UBSan (tests/cpp/plane_asan.cpp), the Python mirrors of the plane structs have the header's
layout, the C++ facade's methods and the example driver compile, and tests/golden/planes_small.npz is what the model gives on its own inputs and
meets the conditions its generator set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plane_cases as pc
import plane_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = [c["name"] for c in pc.CASES]


def host(case):
    from line3d_amd import capi
    return capi.plane_lines_host(case["lines"], case["tol"], case["seeds"], cos_max=case["cos_max"], cos_min=case["cos_min"], min_lines=case["min_lines"])


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(name):
    case = pc.BY_NAME[name]
    m = pc.model_of(case)
    n, ms = len(case["lines"]), len(case["seeds"])
    pl, mem, hp, counts = m["planes"], m["members"], m["hyp_plane"], m["counts"].tolist()
    hyp, tab, stay, rep, comp = m["hyp"], m["tab"], m["stay"], m["rep"], m["comp"]
    # what holds for every table
    assert counts[6] == len(pl) and counts[7] == len(mem) and counts[3] - counts[5] == counts[6] and counts[1] - counts[4] == sum(stay)
    assert np.all(np.diff(mem["plane"].astype(np.int64) * (n + 1) + mem["line"]) > 0)
    assert np.bincount(mem["plane"], minlength=len(pl)).tolist() == pl["n_lines"].tolist() and (len(pl) == 0 or pl["n_lines"].min() >= case["min_lines"])
    assert np.bincount(hp[hp >= 0], minlength=len(pl)).tolist() == pl["n_hyp"].tolist() and list(pl["first_hyp"]) == sorted(pl["first_hyp"])
    for k, p in enumerate(pl):
        assert hp[p["rep"]] == k and hp[p["first_hyp"]] == k and abs(np.dot(p["N"], p["N"]) - 1) < 1e-12 and abs(np.dot(p["N"], p["u"])) < 1e-9
        for r in mem[mem["plane"] == k]:                 # the scalar statement of the rule agrees with the elementwise membership
            assert pm.lies_in(tab[r["line"]], list(p["N"]), p["c"])
            assert bool(r["flags"] & pm.SEED) == any(r["line"] in (hyp[h]["i"], hyp[h]["j"]) for h in np.nonzero(hp == k)[0])
    for h in range(ms):                                  # the star rule, by the scalar pair test
        if hyp[h] is not None and rep[h] != h:
            assert bool(stay[h]) == pm.pair_test(tab, hyp[h], hyp[rep[h]], case["cos_min"])
    claim = case["claim"]
    if claim[0] == "size":
        assert (n, ms) == claim[1:] and counts[0] == n and counts[1] == ms and counts[6] >= max(1, ms // 8)
        assert pc.chunks(ms) == {1: 1, 255: 1, 256: 1, 257: 2, 513: 3, 4096: 16}[ms]
        if ms >= 255:
            assert counts[2] >= ms // 2
        if ms >= 257:                                    # hypotheses of one component lie in different tiles
            assert any(comp[h] // 256 != h // 256 for h in range(ms))
        if ms == 4096:
            assert any(h // 256 - comp[h] // 256 >= 8 for h in range(ms)) and counts[4] > 0
    elif claim[0] == "none":
        assert counts == [claim[1], 0, 0, 0, 0, 0, 0, 0] and hp.tolist() == [-1] * ms
    elif claim[0] == "floor":
        assert counts == [4, 4, 6, 1, 0, 0, 1, 4] and [hyp[h]["N"][2] for h in range(4)] == [1.0, 1.0, -1.0, -1.0] and all(hyp[h]["c"] == 0 for h in range(4))
        assert pl["N"][0].tolist() == [0.0, 0.0, 1.0] and pl["c"][0] == 0 and pl["rect"][0].tolist() == [0.0, 2.0, 0.0, 3.0] and mem["flags"].tolist() == [1] * 4
        assert pl["rep"][0] == 0 and pl["u"][0].tolist() == [1.0, 0.0, 0.0] and pl["v"][0].tolist() == [0.0, 1.0, 0.0]
    elif claim[0] == "duplicate":
        assert counts == [4, 3, 3, 1, 0, 0, 1, 4] and hyp[0]["A"] == hyp[1]["A"] and pl["rep"][0] == 0 and pl["n_hyp"][0] == 3
    elif claim[0] == "equal":
        assert hyp[0]["A"] == hyp[1]["A"] == 6.0 and pl["rep"][0] == claim[1] and rep[:2] == [0, 0] and counts[3] == 1
    elif claim[0] == "ineligible":
        _, bad_seeds, bad_lines = claim
        assert all(hyp[h] is None and hp[h] == -1 for h in bad_seeds) and all(tab[k] is None for k in bad_lines)
        assert counts[:2] == [n - len(bad_lines), ms - len(bad_seeds)] and not set(bad_lines) & set(mem["line"].tolist()) and counts[6] == 1
    elif claim[0] == "cos_max":
        t = pm.hypothesis_terms(tab[0], tab[1])
        assert float(t["b"]) == claim[1] and counts[1] == claim[2] and (hyp[0] is not None) == (abs(claim[1]) <= case["cos_max"]) == (claim[2] == 2)
    elif claim[0] == "fan":
        _, r, stays, released = claim
        assert counts[:5] == [6, 5, 4, 1, len(released)] and len(set(comp)) == 1 and all(x == r for x in rep)
        assert np.nonzero(hp == 0)[0].tolist() == stays and all(hp[h] == -1 for h in released) and pl["n_hyp"][0] == 3
        assert not pm.pair_test(tab, hyp[0], hyp[2], case["cos_min"]) and pm.pair_test(tab, hyp[0], hyp[1], case["cos_min"])
        assert mem["line"].tolist() == [0, 2, 3, 4] and mem["flags"].tolist() == [1] * 4          # the outer lines are 12 degrees off the plane: 0.21 > tol
    elif claim[0] == "cube":
        k = claim[1]
        assert counts == [2 * k, 4 * k, 6 * k, k, 0, 0, k, 4 * k] and pl["n_hyp"].tolist() == [4] * k and pl["n_lines"].tolist() == [4] * k
        assert np.bincount(mem["line"], minlength=n).tolist() == [2] * n and mem["flags"].tolist() == [1] * len(mem)
        faces = [(12 * (h // 24)) + pc.CORNER_PAIRS[h % 24][2] for h in range(ms)]                # seeds of one face stay together, of two faces never
        assert all((faces[a] == faces[b]) == (hp[a] == hp[b]) for a in range(ms) for b in range(ms))
        assert np.all(np.abs(pl["N"]).max(axis=1) == 1.0) and np.all(pl["rect"][:, 1] - pl["rect"][:, 0] == 4.0) and np.all(pl["rect"][:, 3] - pl["rect"][:, 2] == 4.0)
    elif claim[0] == "far":
        assert np.abs(case["lines"]).min() > 0.99 * claim[1] and counts[:2] == [96, 192] and counts[6] >= 40 and counts[2] >= 200
    elif claim[0] == "members":
        assert counts[0] == claim[1] and counts[6] == claim[2] and counts[5] == 1 - claim[2] and len(m["cand"][0]["members"]) == claim[1]
    elif claim[0] == "member_distance":
        _, line, dist, is_member = claim
        p = m["cand"][0]
        assert p["N"] == [0.0, 0.0, 1.0] and p["c"] == 0 and float(pm.plane_distance(tab[line]["P"], p["N"], p["c"])) == dist == float(case["lines"][line][2])
        assert (dist <= case["tol"][line]) == is_member == (line in mem["line"].tolist()) and counts[6] == 1
    elif claim[0] == "pair_distance":
        assert float(hyp[1]["c"]) == claim[1] and hyp[0]["c"] == 0 and counts[2] == claim[2] == int(claim[1] <= 0.25) and counts[3] == 2 - claim[2]
        assert float(pm.plane_distance(tab[0]["P"], hyp[1]["N"], hyp[1]["c"])) == claim[1]
    elif claim[0] == "cos_min":
        with np.errstate(all="ignore"):
            nd = float(abs(pm.dot(hyp[0]["N"], hyp[1]["N"])))
        assert nd == claim[1] and counts[2] == claim[2] == int(nd >= case["cos_min"]) and counts[3] == 2 - claim[2]
    else:
        raise AssertionError(claim)


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model_bit_for_bit(name):
    case = pc.BY_NAME[name]
    got, exp = host(case), pc.model_of(case)
    assert pc.same(got, exp), (name, pc.difference(got, exp))


@pytest.mark.parametrize("name", [r[0] for r in pc.REFUSALS])
def test_refusals(name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in pc.REFUSALS if r[0] == name)
    kw = pc.refusal_arguments(overrides)
    with pytest.raises(capi.L3DError) as e:
        capi.plane_lines_host(kw["lines"], kw["tol"], kw["seeds"], cos_max=kw["cos_max"], cos_min=kw["cos_min"], min_lines=kw["min_lines"])
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_null_pointers_are_refused_and_empty_tables_are_fine():
    from line3d_amd import capi
    lib = capi.load_library()
    lines, tol, seeds = pc.GOOD["lines"], pc.GOOD["tol"], pc.GOOD["seeds"]
    prm = capi.plane_params()
    hp, counts = np.zeros(4, np.int32), np.zeros(8, np.int32)
    pl, mem, npl, nm = C.POINTER(capi.Plane)(), C.POINTER(capi.PlaneMember)(), C.c_int(0), C.c_int(0)
    good = [capi._p(lines), capi._p(tol), C.c_int(4), capi._p(seeds), C.c_int(4), C.byref(prm), C.byref(pl), C.byref(npl), C.byref(mem), C.byref(nm), capi._p(hp), capi._p(counts)]
    assert lib.l3d_test_plane_lines_host(*good) == 0
    assert npl.value == 1 and nm.value == 4 and hp.tolist() == [0] * 4 and counts.tolist() == [4, 4, 6, 1, 0, 0, 1, 4]
    assert (pl[0].rep, pl[0].first_hyp, pl[0].n_hyp, pl[0].n_lines, pl[0].c) == (0, 0, 4, 4, 0.0) and [mem[k].line for k in range(4)] == [0, 1, 2, 3]
    lib.l3d_free(pl)
    lib.l3d_free(mem)
    for i in (0, 1, 3, 5, 6, 7, 8, 9, 10, 11):
        args = list(good)
        args[i] = None
        assert lib.l3d_test_plane_lines_host(*args) == 1, i
    lib.l3d_plane_last_error.restype = C.c_char_p
    assert b"null" in lib.l3d_plane_last_error()
    for lines, tol, seeds in ((np.zeros((0, 6)), np.zeros(0), np.zeros((0, 2), np.int32)), (pc.GOOD["lines"], pc.GOOD["tol"], np.zeros((0, 2), np.int32))):
        out = capi.plane_lines_host(lines, tol, seeds)
        assert out["planes"].shape == (0,) and out["members"].shape == (0,) and out["hyp_plane"].shape == (0,) and out["counts"].tolist() == [0] * 8


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/plane_asan.cpp: l3d_plane.hpp -- the argument checks, the tables, the pair test, the components, the star rule, the parameters, the
    members and the extents -- and a main of its own, built with AddressSanitizer and UBSan"""
    exe = str(tmp_path / "plane_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "plane_asan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout, r.stdout


def test_facade_compiles(tmp_path):
    src = tmp_path / "facade_planes.cpp"
    src.write_text('''#include "line3D_amd.hpp"
int use(L3D::Line3D& l)
{
    l.setPlanes();
    L3D::PlaneParams p;
    p.distPx = 6.0; p.angleDeg = 15.0; p.minLines = 4;
    l.setPlanes(true, p);
    l.setPlanes(false);
    L3D::PlaneStats st;
    const bool a = l.getPlanes(st);
    const bool b = l.save3DPlanesAsOBJ("planes.obj");
    int sum = (a ? 1 : 0) + (b ? 2 : 0) + st.eligibleLines + st.eligibleHypotheses + st.hypothesisEdges + st.components + st.hypothesesReleased + st.candidatesDropped + st.memberRecords;
    for (const L3D::Plane& q : st.planes) sum += q.hypotheses + (int)q.lines.size() + (int)q.seed.size() + (int)(q.N[0] + q.c + q.u[0] + q.v[0] + q.rect[0]);
    return sum + (int)st.planesPerLine.size();
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "main_vsfm_amd.cpp")])
    driver = open(os.path.join(ROOT, "examples", "main_vsfm_amd.cpp")).read()
    assert '"--planes"' in driver and '"--planes-obj"' in driver


def test_the_golden_is_what_its_generator_says():
    """the model on the golden's own inputs gives the golden's planes, and so does the host twin; the generator's three conditions hold"""
    from line3d_amd import capi
    g = np.load(os.path.join(HERE, "golden", "planes_small.npz"))
    j = np.load(os.path.join(HERE, "golden", "junction_small.npz"))
    assert g["lines"].tobytes() == j["lines"].tobytes() and g["tol"].tobytes() == j["tol"].tobytes()
    rec = j["records"]
    keep = (rec["where_i"] != 2) | (rec["where_j"] != 2)
    assert g["seeds"].tolist() == np.stack([rec["i"][keep], rec["j"][keep]], axis=1).tolist() and len(g["seeds"]) == 321
    out = pm.planes(g["lines"], g["tol"], g["seeds"], pc.COS10, pc.COS10, 3)
    exp = {k: g[k] for k in pc.KEYS}
    assert pc.same(out, exp), pc.difference(out, exp)
    got = capi.plane_lines_host(g["lines"], g["tol"], g["seeds"], cos_max=pc.COS10, cos_min=pc.COS10, min_lines=3)
    assert pc.same(got, exp), pc.difference(got, exp)
    # face truth from the scene's corners
    from line3d_amd.synth import make_scene_boxes
    shape = [int(x) for x in j["scene"]]
    scene = make_scene_boxes(shape[0], shape[1], shape[2], seed=shape[3])
    fr = pm.face_recall(scene.corners, scene.corner_edges, g["edge_of"], g["line_box"], g["tol"], out)
    assert fr["covered"] == g["covered"].tolist() and fr["recalled"] == g["recalled"].tolist() and fr["corner_ratio"] == float(g["corner_ratio"])
    assert 10 * len(fr["recalled"]) >= 9 * len(fr["covered"]) and len(fr["covered"]) >= 30
    assert not fr["mixed"] and len(g["mixed"]) == 0
    assert fr["corner_ratio"] <= 1.0
    faces = pm.box_faces(scene.corner_edges)
    assert len(faces) == 48 and all(len(cs) == 4 and len(es) == 4 for cs, es in faces)


def test_struct_layout_and_symbols(tmp_path):
    from line3d_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\n'
                   '#define O(t, f) (int)offsetof(t, f)\n'
                   'int main(void) {\n'
                   '  printf("%d %d %d %d %d\\n", (int)sizeof(l3d_plane_params), O(l3d_plane_params, cos_max), O(l3d_plane_params, cos_min), O(l3d_plane_params, min_lines),\n'
                   '         O(l3d_plane_params, pad));\n'
                   '  printf("%d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(l3d_plane), O(l3d_plane, N), O(l3d_plane, c), O(l3d_plane, u), O(l3d_plane, v), O(l3d_plane, rect),\n'
                   '         O(l3d_plane, rep), O(l3d_plane, first_hyp), O(l3d_plane, n_hyp), O(l3d_plane, n_lines));\n'
                   '  printf("%d %d %d %d %d\\n", (int)sizeof(l3d_plane_member), O(l3d_plane_member, plane), O(l3d_plane_member, line), O(l3d_plane_member, flags),\n'
                   '         O(l3d_plane_member, pad));\n'
                   '  printf("%d\\n", L3D_PLANE_SEED);\n'
                   '  return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True).stdout.splitlines()]

    def layout(struct, dtype):
        assert C.sizeof(struct) == dtype.itemsize and all(getattr(struct, f).offset == dtype.fields[f][1] for f in dtype.names)
        return [C.sizeof(struct)] + [getattr(struct, f[0]).offset for f in struct._fields_]

    P = capi.PlaneParams
    assert got[0] == [C.sizeof(P), P.cos_max.offset, P.cos_min.offset, P.min_lines.offset, P.pad.offset] == [24, 0, 8, 16, 20], got[0]
    assert got[1] == layout(capi.Plane, capi.PLANE) and got[1][0] == 128, got[1]
    assert got[2] == layout(capi.PlaneMember, capi.PLANE_MEMBER) and got[2][0] == 16, got[2]
    assert got[3] == [capi.PLANE_SEED] == [pm.SEED]
    assert capi.PLANE == pm.PLANE and capi.PLANE_MEMBER == pm.MEMBER
    lib = capi.load_library()
    missing = [s for s in ("l3d_plane_lines", "l3d_test_plane_lines_host", "l3d_plane_last_error", "l3d_line3d_set_planes", "l3d_line3d_get_planes",
                           "l3d_line3d_save_planes") if not hasattr(lib, s)]
    assert not missing, missing
    names = lib.l3d_profile_names().decode().split(";")
    for k in ("plane_prepare", "plane_hyp", "plane_count", "plane_scan", "plane_write", "plane_cc_init", "plane_cc_hook", "plane_cc_compress", "plane_rep", "plane_star",
              "plane_flag", "plane_cscan", "plane_keys", "plane_sort", "plane_param", "plane_mcount", "plane_keep", "plane_pscan", "plane_mmask", "plane_mscan",
              "plane_mwrite", "plane_seed", "plane_extent", "plane_finish"):
        assert k in names, k
    p = capi.plane_params()
    assert p.cos_max == pc.COS10 and p.cos_min == pc.COS10 and p.min_lines == 3
    header = open(os.path.join(ROOT, "include", "line3d_amd.h")).read()
    assert "PLANES OF 3-D LINES" in header and "PLANES OF 3-D LINES, below" in header
