"""The merge case tables (tests/merge_cases.py) on a machine without a GPU: every table is the case its name claims (asserted with the model of
tests/merge_model.py, the rules of include/line3d_amd.h "MERGING DUPLICATE LINES" in numpy), the host entry point l3d_test_merge_lines_host -- the
very functions the kernels run -- equals the model bit for bit on all of them and on the lines of the benchmark scene's golden, every refusal comes
with its code and cause, the host code is clean under AddressSanitizer and UBSan (tests/cpp/merge_asan.cpp), the Python mirror of l3d_merge_params
has the header's layout, and the C++ facade's methods compile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merge_cases as mc
import merge_model as mm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = [c["name"] for c in mc.CASES]


def host(case):
    from line3d_amd import capi
    return capi.merge_lines_host(case["lines"], case["tol"], cos_min=case["cos_min"], max_gap=case["max_gap"])


def terms_of(case):
    """|dot|, max(e_P, e_Q), overlap of lines 0 and 1 of a two-line table, a chosen by the rule"""
    t = [mm.prepare(case["lines"][k], case["tol"][k]) for k in (0, 1)]
    a, b = (t[0], t[1]) if t[0][3] >= t[1][3] else (t[1], t[0])
    c, eP, eQ, ov = mm.pair_terms(a, b)
    return dict(c=float(c), e=float(max(eP, eQ)), ov=float(ov))


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(name):
    case = mc.BY_NAME[name]
    m = mc.model_of(case)
    n = len(case["lines"])
    group, pairs, counts = m["group"], m["pairs"], m["counts"].tolist()
    assert len(group) == n and all(group[group[k]] == group[k] <= k for k in range(n))
    assert all(i < j for i, j in pairs.tolist()) and pairs.tolist() == sorted(pairs.tolist())
    claim = case["claim"]
    if claim[0] == "size":
        assert n == claim[1] and counts[0] == n
        if n >= 2:
            assert len(pairs) >= n // 2 and counts[3] >= 1
        if n >= 257:                                # a row block's lines pair with lines of a later tile
            assert any(j // 256 > i // 256 for i, j in pairs.tolist())
        if n == 513:                                # and with the third tile: the triangular skip starts each row block at its own tile
            assert any(j // 256 - i // 256 == 2 for i, j in pairs.tolist()) and any(i >= 256 for i, j in pairs.tolist())
    elif claim[0] == "one_group":
        assert n == claim[1] and len(pairs) == claim[2] and (group == 0).all() and counts == [n, 1, 0, 1]
        assert np.bincount(pairs[:, 0]).max() == n - 1 > 128
    elif claim[0] == "terms":
        assert n == 2 and len(pairs) == claim[1] and counts == [2, claim[1], 0, claim[1]]
        got = terms_of(case)
        for k, v in claim[2].items():
            assert got[k] == v, (k, got[k], v)
        if "e" in claim[2]:                         # the decision is taken at the tolerance
            assert (got["e"] <= max(case["tol"])) == bool(claim[1])
        if "c" in claim[2] and "e" not in claim[2]:
            assert (got["c"] >= case["cos_min"]) == bool(claim[1])
        if "ov" in claim[2]:
            Lb = min(mm.prepare(case["lines"][k], 0.0)[3] for k in (0, 1))
            assert (got["ov"] >= -(case["max_gap"] * Lb)) == bool(claim[1])
    elif claim[0] == "equal_L":
        t = [mm.prepare(case["lines"][k], case["tol"][k]) for k in (0, 1)]
        assert t[0][3] == t[1][3] and len(pairs) == claim[1] == 0
        assert not mm.pair_test(t[0], t[1], case["cos_min"], case["max_gap"])
        # with the other line as a the pair would pass: the tie rule decides this table
        c, eP, eQ, ov = mm.pair_terms(t[1], t[0])
        assert c >= case["cos_min"] and max(eP, eQ) <= case["tol"][0] and ov >= 0
    elif claim[0] == "rep":
        assert m["rep"].tolist() == claim[1]
        assert any(m["rep"][k] != m["comp"][k] for k in range(n)) == (name == "representative_is_not_the_lowest_index")
    elif claim[0] == "release":
        assert group.tolist() == claim[1] and counts == [3] + claim[2][1:] and len(pairs) == 2 and len(set(m["comp"].tolist())) == 1
    elif claim[0] == "ineligible":
        for k in claim[1]:
            assert mm.prepare(case["lines"][k], case["tol"][k]) is None and group[k] == k and k not in pairs
            assert k // 256 == 0 and 64 <= k < 192
        assert counts[0] == n - len(claim[1]) and len(pairs) > 0
    elif claim[0] == "far":
        assert np.abs(case["lines"]).min() > 0.99 * claim[1] and 0 < len(pairs) and counts[3] == 16 and counts[2] == 0
    else:
        raise AssertionError(claim)


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model_bit_for_bit(name):
    case = mc.BY_NAME[name]
    assert mc.same(host(case), mc.model_of(case)), name


@pytest.mark.parametrize("name", [r[0] for r in mc.REFUSALS])
def test_refusals(name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in mc.REFUSALS if r[0] == name)
    kw = mc.refusal_arguments(overrides)
    with pytest.raises(capi.L3DError) as e:
        capi.merge_lines_host(kw["lines"], kw["tol"], cos_min=kw["cos_min"], max_gap=kw["max_gap"])
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_null_pointers_are_refused_and_an_empty_table_is_fine():
    from line3d_amd import capi
    lib = capi.load_library()
    lines, tol = mc.GOOD["lines"], mc.GOOD["tol"]
    prm = capi.merge_params(0.9, 0.0)
    group, counts = np.zeros(2, np.int32), np.zeros(4, np.int32)
    pairs, k = C.POINTER(C.c_int32)(), C.c_int(0)
    good = [capi._p(lines), capi._p(tol), C.c_int(2), C.byref(prm), capi._p(group), C.byref(pairs), C.byref(k), capi._p(counts)]
    assert lib.l3d_test_merge_lines_host(*good) == 0 and k.value == 1 and group.tolist() == [0, 0] and counts.tolist() == [2, 1, 0, 1]
    lib.l3d_free(pairs)
    for i in (0, 1, 3, 4, 5, 6, 7):
        args = list(good)
        args[i] = None
        assert lib.l3d_test_merge_lines_host(*args) == 1, i
    out = capi.merge_lines_host(np.zeros((0, 6)), np.zeros(0), cos_min=0.9)
    assert out["group"].shape == (0,) and out["pairs"].shape == (0, 2) and out["counts"].tolist() == [0, 0, 0, 0]


# ---- the benchmark scene's golden: the oracle's own lines, with and without the diffusion
_scene = {}


def golden_lines(kind):
    """lines (n, 6), tol (n,), the majority ground-truth id per line"""
    if "scene" not in _scene:
        from line3d_amd.synth import make_scene
        _scene["scene"] = make_scene(64, 2000, 12, seed=20260)
        _scene["g"] = np.load(os.path.join(HERE, "golden", "config2_full.npz"))
    scene, g = _scene["scene"], _scene["g"]
    ids, id_off, pts, pt_off = g[kind + "_ids"], g[kind + "_id_off"], g[kind + "_pts"], g[kind + "_pt_off"]
    n = len(id_off) - 1
    lines = np.hstack([pts[pt_off[:-1], :3], pts[pt_off[1:] - 1, 3:]])
    views = {int(v["id"]): v for v in scene.views}
    tol = np.array([mm.line_tol(lines[k, :3], lines[k, 3:], ids[id_off[k]:id_off[k + 1]], views, 4.0) for k in range(n)], np.float64)
    gt = np.array([np.bincount([int(views[int(c)]["gt"][int(s)]) for c, s in ids[id_off[k]:id_off[k + 1]]]).argmax() for k in range(n)])
    return lines, tol, gt


@pytest.mark.parametrize("kind", ["plain", "rdd"])
def test_golden_lines_of_the_benchmark_scene(kind):
    from line3d_amd import capi
    lines, tol, gt = golden_lines(kind)
    n = len(lines)
    got = capi.merge_lines_host(lines, tol, cos_min=mc.COS5, max_gap=0.0)
    exp = mm.group_lines(lines, tol, mc.COS5, 0.0)
    assert mc.same(got, exp)
    group = got["group"]
    sizes = np.bincount(group, minlength=n)
    remaining = int((sizes > 0).sum())
    mixed = sum(1 for k in np.nonzero(sizes >= 2)[0] if len(set(gt[group == k].tolist())) > 1)
    print("%s: %d lines, %d pairs, %d remain after one grouping, %d released, %d groups of two or more, %d of them mix ground-truth ids"
          % (kind, n, len(got["pairs"]), remaining, got["counts"][2], got["counts"][3], mixed))
    assert mixed == 0
    if kind == "plain":
        assert 3 * remaining < n


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/merge_asan.cpp: l3d_merge.hpp -- the argument checks, the table, the pair test, the components, the star rule -- and a main of its
    own, built with AddressSanitizer and UBSan"""
    exe = str(tmp_path / "merge_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "merge_asan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout, r.stdout


def test_struct_layout_and_symbols(tmp_path):
    from line3d_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(l3d_merge_params), offsetof(l3d_merge_params, cos_min), offsetof(l3d_merge_params, max_gap)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    P = capi.MergeParams
    assert got == [C.sizeof(P), P.cos_min.offset, P.max_gap.offset], got
    lib = capi.load_library()
    missing = [s for s in ("l3d_merge_lines", "l3d_test_merge_lines_host", "l3d_merge_last_error", "l3d_line3d_set_merging", "l3d_line3d_get_merging") if not hasattr(lib, s)]
    assert not missing, missing
    names = lib.l3d_profile_names().decode().split(";")
    for k in ("merge_prepare", "merge_count", "merge_scan", "merge_write", "merge_rep", "merge_star", "merge_group"):
        assert k in names, k
    p = capi.merge_params()
    assert p.cos_min == mc.COS5 and p.max_gap == 0.0


def test_facade_compiles(tmp_path):
    src = tmp_path / "facade_merge.cpp"
    src.write_text('''#include "line3D_amd.hpp"
int use(L3D::Line3D& l)
{
    l.setMerging();
    l.setMerging(true, 8.0, 3.0, 0.1, 2);
    l.setMerging(false);
    L3D::MergeStats st;
    std::vector<int> final_index, n_sources;
    const bool a = l.getMerging(st);
    const bool b = l.getMerging(st, &final_index, &n_sources);
    return (a ? 1 : 0) + (b ? 2 : 0) + st.linesBefore + st.linesAfter + st.rounds + st.pairsFirstRound + st.groupsMerged + st.linesReleased + st.emptyRefits;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
