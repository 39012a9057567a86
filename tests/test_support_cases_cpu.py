"""The support case tables (tests/support_cases.py) on a machine without a GPU: every table is the case its name claims (asserted with the model of
tests/support_model.py, the rules of include/line3d_amd.h "SUPPORT OF 3-D LINES" in numpy), the host entry point l3d_test_support_lines_host -- the
very functions the kernels run -- equals the model bit for bit on all of them (records, cam_start, best, counts), every refusal comes with its code
and cause, the host code is clean under AddressSanitizer and UBSan (tests/cpp/support_asan.cpp, a program of its own), the Python mirrors of
l3d_support_params and l3d_support_record have the header's layout, and on the small scene's golden lines the support is what the feature is for:
members are found again, supporters carry their line's ground-truth id, and a line is supported in several times the views it has members in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import project_model as pm
import support_cases as sc
import support_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = [c["name"] for c in sc.CASES]


def host(case):
    from line3d_amd import capi
    return capi.support_lines_host(case["seg3d"], case["cams"], case["segs"], sc.params_of(case["p"]))


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(name):
    case = sc.BY_NAME[name]
    m = sc.model_of(case)
    claim, p = case["claim"], case["p"]
    rec, start = m["records"], m["cam_start"]
    n, ncam = len(case["seg3d"]), len(case["cams"])
    rows = [[sm.row(cam, s, p["near"], p["margin"]) for s in case["seg3d"]] for cam in case["cams"]]
    n_rows = [sum(r is not None for r in per) for per in rows]
    triples = [(c, int(r["seg3d"]), int(r["seg2d"])) for c in range(ncam) for r in rec[start[c]:start[c + 1]]]
    assert triples == sorted(triples) and len(set(triples)) == len(triples)                 # camera-major, ascending k, ascending j
    assert m["counts"].tolist() == [sum(n_rows), sum(sm.column(g) is not None for s in case["segs"] for g in s), len(rec), int((m["best"] >= 0).sum())]
    if "rows" in claim:
        assert n_rows == claim["rows"]
        for c, k in enumerate(claim["rows"]):
            if k == 0:
                assert start[c] == start[c + 1] and len(case["segs"][c]) > 0
        assert len(rec) > 0                                                                 # the other camera supports
    if claim.get("touch"):
        assert rows[0][0] is None
        sm.row(case["cams"][0], case["seg3d"][0], p["near"], p["margin"])
        assert pm.clip.trace is not None and pm.clip.trace[0] == pm.clip.trace[1]          # the rule ran to its end: t0 == t1
    if "cols" in claim:
        assert [len(s) for s in case["segs"]] == claim["cols"]
    if "rows_min" in claim:
        assert sum(n_rows) >= claim["rows_min"] and (n < 4 or sum(n_rows) < n * ncam)       # some lanes have no row
        assert len(rec) >= claim["records_min"]
        if len(rec):
            for tile in range((max(claim["cols"]) + 255) // 256):                          # every column tile holds a record
                assert any(j // 256 == tile for _, _, j in triples), tile
        if n >= 257:
            assert any(k >= 256 for _, k, _ in triples) and any(k < 64 for _, k, _ in triples)
    if "records" in claim:
        assert triples == claim["records"]
    if "best" in claim:
        assert m["best"].tolist() == claim["best"]
    if "terms" in claim:
        cs, eU, eV, ov, Lm = sm.pair_terms(rows[0][0], sm.column(case["segs"][0][0]))
        got = dict(cs=float(cs), e=float(max(eU, eV)), ov=float(ov), Lm=float(Lm))
        for k, v in claim["terms"].items():
            assert got[k] == v, (k, got[k], v)
        passes = (0, 0, 0) in triples
        if "e" in claim["terms"] and not name.startswith("cos"):
            assert (got["e"] <= p["dist_px"]) == passes
        if "cs" in claim["terms"]:
            assert (got["cs"] >= p["cos_min"]) == passes
        if "ov" in claim["terms"]:
            assert (got["ov"] >= np.float64(p["min_overlap"]) * np.float64(got["Lm"])) == passes
    if "ineligible" in claim:
        for j in range(len(case["segs"][0])):
            assert (sm.column(case["segs"][0][j]) is None) == (j in claim["ineligible"])
        assert m["counts"][1] == claim["cols_eligible"] and all(m["best"][j] == -1 for j in claim["ineligible"])
    if claim.get("clipped"):
        assert rows[0][0]["t"][0] > 0 and rows[0][0]["A"][0] == pytest.approx(-0.5, abs=1e-9)
    if "overlap" in claim:
        assert float(rec["overlap"][0]) == claim["overlap"] and rows[0][0]["La"] < sm.column(case["segs"][0][0])["Lb"]


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model_bit_for_bit(name):
    case = sc.BY_NAME[name]
    assert sc.same(host(case), sc.model_of(case)), name


@pytest.mark.parametrize("name", [r[0] for r in sc.REFUSALS])
def test_refusals(name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in sc.REFUSALS if r[0] == name)
    kw = sc.refusal_arguments(overrides)
    with pytest.raises(capi.L3DError) as e:
        capi.support_lines_host(kw["seg3d"], kw["cams"], kw["segs"], sc.params_of(kw["p"]))
    assert e.value.code == code and word in str(e.value), str(e.value)


@pytest.mark.parametrize("name", [r[0] for r in sc.RAW_REFUSALS])
def test_refusals_of_the_c_call(name):
    from line3d_amd import capi
    lib = capi.load_library()
    lib.l3d_support_last_error.restype = C.c_char_p
    _, change, code, word = next(r for r in sc.RAW_REFUSALS if r[0] == name)
    args, keep = sc.raw_arguments(change)
    rc, out = capi._support_call(lib.l3d_test_support_lines_host, (), *args)
    assert rc == code and out is None and word in lib.l3d_support_last_error().decode(), lib.l3d_support_last_error()


def test_null_outputs_are_refused_and_empty_inputs_are_fine():
    from line3d_amd import capi
    lib = capi.load_library()
    (seg, n, cams, m, cols, start, prm), keep = sc.raw_arguments({})
    rec, cam_start, best, counts = C.POINTER(capi.SupportRecord)(), np.zeros(2, np.int64), np.zeros(1, np.int32), np.zeros(4, np.int64)
    good = [seg, C.c_int(n), cams, C.c_int(m), cols, capi._p(start), C.byref(prm), C.byref(rec), capi._p(cam_start), capi._p(best), capi._p(counts)]
    assert lib.l3d_test_support_lines_host(*good) == 0 and counts.tolist() == [1, 1, 1, 1] and best.tolist() == [0] and cam_start.tolist() == [0, 1]
    assert (rec[0].seg3d, rec[0].seg2d, rec[0].dist, rec[0].overlap) == (0, 0, 1.0, 1.0)
    lib.l3d_free(rec)
    for i in (7, 8, 9, 10):
        args = list(good)
        args[i] = None
        assert lib.l3d_test_support_lines_host(*args) == 1, i
    cam = sc.GOOD["cams"]
    out = capi.support_lines_host(np.zeros((0, 6)), cam, sc.GOOD["segs"])                  # no 3-D segment
    assert len(out["records"]) == 0 and out["cam_start"].tolist() == [0, 0] and out["best"].tolist() == [-1] and out["counts"].tolist() == [0, 0, 0, 0]
    out = capi.support_lines_host(sc.GOOD["seg3d"], [], [])                                # no camera
    assert len(out["records"]) == 0 and out["cam_start"].tolist() == [0] and out["best"].shape == (0,) and out["counts"].tolist() == [0, 0, 0, 0]
    assert sc.same(out, sm.support(sc.GOOD["seg3d"], [], [], 3.0, sc.COS5, 0.5, 1e-3, 0.0))


# ---- the small scene's golden: the oracle's own lines, with and without the diffusion
_scene = {}


def golden(kind):
    """(seg3d (n, 6) one segment per line, the members [(view, segment)] per line, cams, segs per camera, views)"""
    if "scene" not in _scene:
        from line3d_amd.synth import make_scene
        _scene["scene"] = make_scene(32, 100, 6, seed=11)
        _scene["g"] = np.load(os.path.join(HERE, "golden", "merge_small.npz"))
    scene, g = _scene["scene"], _scene["g"]
    pre = kind + "_r0_"
    ids, id_off, pts, pt_off = g[pre + "ids"], g[pre + "id_off"], g[pre + "pts"], g[pre + "pt_off"]
    n = len(id_off) - 1
    return scene, ids, id_off, pts, pt_off, n


def test_golden_arrays_are_there():
    g = np.load(os.path.join(HERE, "golden", "merge_small.npz"))
    for kind in ("plain", "rdd"):
        for k in ("ids", "id_off", "pts", "pt_off"):
            assert kind + "_r0_" + k in g.files, (kind, k, g.files)


@pytest.mark.parametrize("kind", ["plain", "rdd"])
def test_golden_lines_of_the_small_scene(kind):
    """The conditions of the feature, on the model (the host twin is held to the model bit for bit on the same input): at least 95 % of the members
    found again, at least 99 % of the records with their line's majority ground-truth id, and the median number of supported views per line at least
    four times the median number of member views."""
    from line3d_amd import capi
    scene, ids, id_off, pts, pt_off, n = golden(kind)
    views = sorted(scene.views, key=lambda v: int(v["id"]))
    vid = {int(v["id"]): c for c, v in enumerate(views)}
    cams = [(np.asarray(v["K"], np.float64), np.asarray(v["R"], np.float64), np.asarray(v["t"], np.float64), int(v["width"]), int(v["height"])) for v in views]
    segs = [np.asarray(v["segments"], np.float32).reshape(-1, 4) for v in views]
    seg3d = np.asarray(pts, np.float64).reshape(-1, 6)
    line_of = np.repeat(np.arange(n), np.diff(pt_off))
    p = sc.P(dist_px=3.0, cos_min=sc.COS5, min_overlap=0.5, near=1e-6, margin=3.0)
    m = sm.support(seg3d, cams, segs, p["dist_px"], p["cos_min"], p["min_overlap"], p["near"], p["margin"])
    assert sc.same(capi.support_lines_host(seg3d, cams, segs, sc.params_of(p)), m)
    member_of = {}
    for k in range(n):
        for c, s in ids[id_off[k]:id_off[k + 1]]:
            member_of[(vid[int(c)], int(s))] = k
    gt_line = [np.bincount([int(views[vid[int(c)]]["gt"][int(s)]) for c, s in ids[id_off[k]:id_off[k + 1]]]).argmax() for k in range(n)]
    # per line: the (view, segment) pairs any of its 3-D segments reaches
    sup = [set() for _ in range(n)]
    for c in range(len(cams)):
        r = m["records"][m["cam_start"][c]:m["cam_start"][c + 1]]
        for k3, j in zip(r["seg3d"].tolist(), r["seg2d"].tolist()):
            sup[line_of[k3]].add((c, j))
    records = sum(len(s) for s in sup)
    right = sum(1 for k in range(n) for c, j in sup[k] if int(views[c]["gt"][j]) == gt_line[k])
    found = sum(1 for key, k in member_of.items() if key in sup[k])
    mviews = [len({vid[int(c)] for c, _ in ids[id_off[k]:id_off[k + 1]]}) for k in range(n)]
    sviews = [len({c for c, _ in sup[k]}) for k in range(n)]
    on_a_line = {key for s in sup for key in s}
    print("%s: %d lines, %d 3-D segments, member views median %g, supported views median %g / min %d, %d records, %d with the line's ground-truth id (%.2f %%), "
          "%d of %d members found again (%.2f %%), %d of %d segments on some line"
          % (kind, n, len(seg3d), np.median(mviews), np.median(sviews), min(sviews), records, right, 100.0 * right / records, found, len(member_of),
             100.0 * found / len(member_of), len(on_a_line), sum(len(s) for s in segs)))
    assert found >= 0.95 * len(member_of)
    assert right >= 0.99 * records
    assert np.median(sviews) >= 4 * np.median(mviews)


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/support_asan.cpp: l3d_support.hpp (with l3d_project.hpp under it) -- the argument checks, rows, columns, the pair test, the best rows,
    the sizing rules -- and a main of its own, built with AddressSanitizer and UBSan"""
    exe = str(tmp_path / "support_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "support_asan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout, r.stdout


def test_struct_layout_and_symbols(tmp_path):
    from line3d_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(l3d_support_params), offsetof(l3d_support_params, dist_px), offsetof(l3d_support_params, cos_min),\n'
                   '    offsetof(l3d_support_params, min_overlap), offsetof(l3d_support_params, near_z), offsetof(l3d_support_params, margin));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(l3d_support_record), offsetof(l3d_support_record, seg3d), offsetof(l3d_support_record, seg2d),\n'
                   '    offsetof(l3d_support_record, dist), offsetof(l3d_support_record, overlap)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    P, R = capi.SupportParams, capi.SupportRecord
    assert got[:6] == [C.sizeof(P), P.dist_px.offset, P.cos_min.offset, P.min_overlap.offset, P.near_z.offset, P.margin.offset], got
    assert got[6:] == [C.sizeof(R), R.seg3d.offset, R.seg2d.offset, R.dist.offset, R.overlap.offset] == [16, 0, 4, 8, 12], got
    assert capi.SUPPORT_RECORD.itemsize == 16 and [capi.SUPPORT_RECORD.fields[k][1] for k in ("seg3d", "seg2d", "dist", "overlap")] == [0, 4, 8, 12]
    lib = capi.load_library()
    missing = [s for s in ("l3d_support_lines", "l3d_support_lines_device", "l3d_test_support_lines_host", "l3d_support_last_error") if not hasattr(lib, s)]
    assert not missing, missing
    names = lib.l3d_profile_names().decode().split(";")
    for k in ("sup_prepare", "sup_count", "sup_scan", "sup_write", "sup_best"):
        assert k in names, k
    p = capi.support_params()
    assert (p.dist_px, p.cos_min, p.min_overlap, p.near_z, p.margin) == (3.0, sc.COS5, 0.5, 1e-6, 3.0)


def test_line_support_layout_and_object_symbols(tmp_path):
    from line3d_amd import capi
    src = tmp_path / "layout_line.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(l3d_line_support), offsetof(l3d_line_support, view_id), offsetof(l3d_line_support, seg),\n'
                   '    offsetof(l3d_line_support, seg3d), offsetof(l3d_line_support, dist), offsetof(l3d_line_support, overlap), offsetof(l3d_line_support, flags));\n'
                   '  printf("%d %d %d\\n", L3D_SUPPORT_MEMBER, L3D_SUPPORT_MEMBER_ELSEWHERE, L3D_SUPPORT_BEST); return 0; }\n')
    exe = str(tmp_path / "layout_line")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    R = capi.LineSupport
    assert got[:7] == [C.sizeof(R), R.view_id.offset, R.seg.offset, R.seg3d.offset, R.dist.offset, R.overlap.offset, R.flags.offset] == [24, 0, 4, 8, 12, 16, 20], got
    assert got[7:] == [capi.SUPPORT_MEMBER, capi.SUPPORT_MEMBER_ELSEWHERE, capi.SUPPORT_BEST]
    assert capi.LINE_SUPPORT.itemsize == 24 and [capi.LINE_SUPPORT.fields[k][1] for k in ("view_id", "seg", "seg3d", "dist", "overlap", "flags")] == [0, 4, 8, 12, 16, 20]
    lib = capi.load_library()
    missing = [s for s in ("l3d_line3d_gather_support", "l3d_line3d_set_support", "l3d_line3d_get_support") if not hasattr(lib, s)]
    assert not missing, missing


def test_facade_compiles(tmp_path):
    src = tmp_path / "facade_support.cpp"
    src.write_text('''#include "line3D_amd.hpp"
int use(L3D::Line3D& l)
{
    l.setSupport();
    l.setSupport(true, 2.0, 4.0, 0.6);
    l.setSupport(false);
    L3D::SupportParams p;
    p.distPx = 2.0; p.angleDeg = 4.0; p.minOverlap = 0.25; p.nearZ = 1e-3; p.margin = 5.0;
    std::vector<std::vector<L3D::LineSupport> > perLine;
    const bool a = l.gatherSupport(perLine);
    const bool b = l.gatherSupport(perLine, p);
    L3D::SupportStats st;
    const bool c = l.getSupport(st);
    long long sum = st.records + st.membersFound + st.membersNotFound + st.segmentsUnclaimed + (long long)(st.membersBefore.size() + st.membersAdded.size() + st.viewsBefore.size() + st.viewsAfter.size());
    for (auto& line : perLine)
        for (auto& r : line) sum += r.viewID + r.seg + r.seg3D + (r.member ? 1 : 0) + (r.memberElsewhere ? 1 : 0) + (r.best ? 1 : 0) + (r.dist + r.overlap > 0.0f ? 1 : 0);
    return (a ? 1 : 0) + (b ? 2 : 0) + (c ? 4 : 0) + (int)sum;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
