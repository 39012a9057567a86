"""The refinement's case table (tests/refine_cases.py) on a machine without a GPU: every case is what its name claims (asserted with the model of
tests/refine_model.py), the model's Jacobian matches central differences and recovers a noise-free truth, the host entry point l3d_test_refine_host -- the
very functions the kernel runs, with 64 lanes one after the other -- agrees with the model within the measured tolerance
(tests/golden/refine_tolerance.json, written by tests/golden/make_golden_refine.py), its bytes do not depend on a group's position, and the C++ facade's
methods compile."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import refine_cases as rc
import refine_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = rc.tolerance()
NAMES = [c["name"] for c in rc.CASES]


def _host(case):
    from line3d_amd import capi
    return capi.refine_lines_host(*rc.args_of(case))


def test_case_table_covers_the_member_counts_and_launch_shapes():
    assert [int(rc.BY_NAME["members_%d" % n]["group_start"][1]) for n in rc.MEMBER_COUNTS] == [4, 5, 63, 64, 65, 127, 128, 129, 300]
    assert {rc.BY_NAME[k]["n_groups"] for k in ("members_4", "groups_4", "groups_5")} == {1, 4, 5}
    for c in rc.CASES:
        for sl in rc.group_slices(c):
            assert np.all(np.diff(c["member_cam"][sl]) >= 0), "%s: members in key order" % c["name"]
    assert sorted(set(TOL["cases"])) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_tolerance_conditions(name):
    """no case needs more than 1e-6 in any quantity, and adjacent sort keys differ by more than 1000 times the end-point tolerance (model alone)"""
    case = rc.BY_NAME[name]
    for g, m in enumerate(rc.model_of(case)):
        tol = TOL["cases"][name][g]
        if tol is None:
            assert m["status"] == 2
            continue
        assert max(tol["tolerance"].values()) <= 1e-6, "%s group %d is ill-conditioned: %r" % (name, g, tol["tolerance"])
        gap = float(np.diff(np.sort(m["t"])).min() / rc.extent_of(case, g))
        assert gap > 1000 * tol["tolerance"]["points"], "%s group %d: key gap %.3g" % (name, g, gap)


def test_same_camera_and_three_camera_cases():
    c = rc.BY_NAME["same_camera_2_3"]
    counts = np.bincount(c["member_cam"])
    assert len(counts) >= 4 and 2 in counts and 3 in counts
    c = rc.BY_NAME["three_cameras"]
    assert len(set(c["member_cam"].tolist())) == 3
    m = rc.model_of(c)[0]
    assert len(m["segs"]) == 1, "three cameras: the sweep opens once, at the threshold, and closes"


def test_noise_free_truth_comes_back():
    """Bounds: the 2-D coordinates are float32 (below 1024: half an ulp is 2^-15 px per coordinate, 4.4e-5 px per point), so the true line has an rms of at
    most 4.4e-5 px and the minimum no more; a point error of 4.4e-5 px at focal length 800 px and depth 6 is 3.3e-7 units, 1.7e-7 of the extent 2 -- 1e-6
    leaves a factor 6 for the conditioning of the cameras' geometry.  The start was 2 degrees (3.5e-2 rad) and 1 % of the extent off."""
    c = rc.BY_NAME["noise_free_perturbed"]
    m = rc.model_of(c)[0]
    L0, e, E = c["truth"][0]
    start, _ = rm.line_of_points(c["member_pts"].reshape(-1, 3)), None
    assert np.linalg.norm(np.cross(start[1], e)) > 3e-2 and np.linalg.norm(np.cross(start[0] - L0, e)) > 5e-3 * E
    assert m["status"] == 0 and m["rms_after"] <= 4.4e-5 < m["rms_before"]
    assert np.linalg.norm(np.cross(m["line"][3:], e)) <= 1e-6
    assert np.linalg.norm(np.cross(m["line"][:3] - L0, e)) <= 1e-6 * E
    assert all(b <= a for a, b in zip(m["costs"], m["costs"][1:])), "the cost never rises"


def test_noise_and_outlier_cases():
    m = rc.model_of(rc.BY_NAME["noise_half_px"])[0]
    assert m["status"] == 0 and 0.3 < m["rms_after"] < 0.8 and m["rms_after"] < m["rms_before"]
    c2, c0 = rc.BY_NAME["outlier_huber_2"], rc.BY_NAME["outlier_huber_0"]
    assert c2["member_seg"].tobytes() == c0["member_seg"].tobytes() and (c2["huber_px"], c0["huber_px"]) == (2.0, 0.0)
    L0, e, E = c2["truth"][0]
    r, _ = rm.residuals([rm.camera_parts(P) for P in c2["cameras"]], c2["member_cam"], c2["member_seg"].astype(np.float64), L0, e)
    assert np.all(np.abs(r[c2["outlier_member"]]) > 38) and np.abs(np.delete(r, c2["outlier_member"], 0)).max() < 2, "one member 40 px off the line"
    m2, m0 = rc.model_of(c2)[0], rc.model_of(c0)[0]
    off = lambda m: np.linalg.norm(np.cross(m["line"][:3] - L0, e)) / E + np.linalg.norm(np.cross(m["line"][3:], e))   # noqa: E731
    assert off(m2) < 0.2 * off(m0), "the Huber loss keeps the outlier from pulling the line"


def test_scale_cases():
    assert np.linalg.norm(rc.BY_NAME["far_from_origin"]["truth"][0][0]) > 1e4
    assert rc.BY_NAME["extent_1e-3"]["truth"][0][2] == 1e-3
    for name in ("far_from_origin", "extent_1e-3"):
        m = rc.model_of(rc.BY_NAME[name])[0]
        assert m["status"] == 0 and m["rms_after"] < 0.5 < m["rms_before"]


def test_camera_on_line_is_dropped_and_the_rest_refine():
    c = rc.BY_NAME["camera_on_line"]
    cams = [rm.camera_parts(P) for P in c["cameras"]]
    Pc, d = rm.line_of_points(c["member_pts"].reshape(-1, 3))
    assert Pc.tobytes() == np.zeros(3).tobytes() and np.all(np.abs(d) == [1, 0, 0]), "the start is the x axis without a rounding"
    lines = rm.member_lines(cams, c["member_cam"], Pc, d)
    assert [ln[4] for ln in lines] == [i == c["dropped_member"] for i in range(len(lines))]
    assert lines[c["dropped_member"]][3] < rm.N2_MIN
    m = rc.model_of(c)[0]
    assert m["dropped_start"] == 1 and m["status"] == 0 and m["rms_after"] < 1e-3 * m["rms_before"]


def test_parallel_ray_takes_the_fallback():
    c = rc.BY_NAME["parallel_ray"]
    m = rc.model_of(c)[0]
    p = c["parallel_point"]
    assert not m["by_ray"][p] and m["den_rel"][p] <= rm.PARALLEL and np.all(np.delete(m["by_ray"], p)) and np.delete(m["den_rel"], p).min() > 1e-3
    X = c["member_pts"].reshape(-1, 3)[p]
    assert m["t"][p] == float(m["line"][3:] @ (X - m["line"][:3]))


def test_one_centre_is_singular_but_finite():
    c = rc.BY_NAME["one_centre"]
    C = np.array([rm.camera_parts(P)[3] for P in c["cameras"]])
    assert np.abs(C - C[0]).max() < 1e-9
    cams = [rm.camera_parts(P) for P in c["cameras"]]
    Pc, d = rm.line_of_points(c["member_pts"].reshape(-1, 3))
    H = rm.evaluate(cams, c["member_cam"], c["member_seg"].astype(np.float64), Pc, d, 2.0)["H"]
    w = np.linalg.eigvalsh(H)
    assert w[1] < 1e-9 * w[3], "H is singular in two directions: %r" % w
    m = rc.model_of(c)[0]
    assert m["status"] in (0, 1) and np.all(np.isfinite(m["line"])) and m["costs"][-1] <= m["costs"][0]


def test_nan_and_iteration_cases():
    c = rc.BY_NAME["nan_in_points"]
    assert np.isnan(c["member_pts"][rc.group_slices(c)[c["nan_group"]]]).sum() == 1
    assert [m["status"] for m in rc.model_of(c)] == [0, 2, 0]
    m0, m1 = rc.model_of(rc.BY_NAME["max_iterations_0"])[0], rc.model_of(rc.BY_NAME["max_iterations_1"])[0]
    assert (m0["iterations"], m0["status"], m1["iterations"], m1["status"]) == (0, 1, 1, 0) and m0["rms_after"] == m0["rms_before"] and m1["rms_after"] < m1["rms_before"]


@pytest.mark.parametrize("name", ["members_5", "noise_half_px", "outlier_huber_2"])
def test_model_jacobian_matches_central_differences(name):
    """step 1e-6 in units of the scene (extent 2): truncation ~ h^2 |r'''| and cancellation ~ 2^-53 |r| / h ~ 1e-7 px per unit, against entries of 1e2..1e3"""
    c = rc.BY_NAME[name]
    cams = [rm.camera_parts(P) for P in c["cameras"]]
    seg = c["member_seg"].astype(np.float64)
    A, d = rm.line_of_points(c["member_pts"].reshape(-1, 3))
    J = rm.jacobian(cams, c["member_cam"], seg, A, d)
    h = 1e-6
    for i in range(4):
        dp = np.zeros(4)
        dp[i] = h
        rp, _ = rm.residuals(cams, c["member_cam"], seg, *rm.apply(A, d, dp))
        rn, _ = rm.residuals(cams, c["member_cam"], seg, *rm.apply(A, d, -dp))
        assert np.abs((rp - rn) / (2 * h) - J[:, :, i]).max() <= 1e-5 * np.abs(J[:, :, i]).max()


@pytest.mark.parametrize("name", NAMES)
def test_host_entry_point_agrees_with_the_model(name):
    case = rc.BY_NAME[name]
    rc.check_against_model(case, _host(case))


def test_host_bytes_do_not_depend_on_the_position():
    outs = {k: _host(rc.BY_NAME["position_" + k]) for k in ("first", "middle", "last")}
    ref = None
    for k, out in outs.items():
        g = rc.per_group(out, rc.BY_NAME["position_" + k]["probe_at"])
        b = b"".join(np.asarray(g[q]).tobytes() for q in ("line", "rms_before", "rms_after", "iterations", "status", "segs"))
        ref = b if ref is None else ref
        assert b == ref, k
    c = rc.BY_NAME["nan_in_points"]
    out, alone = _host(c), _host(rc.BY_NAME[c["clean_name"]])
    for g, ga in ((0, 0), (2, 1)):
        a, b = rc.per_group(out, g), rc.per_group(alone, ga)
        assert all(np.asarray(a[q]).tobytes() == np.asarray(b[q]).tobytes() for q in a), "the groups beside the NaN are untouched"


def test_host_entry_point_refusals_and_empty_call():
    from line3d_amd import capi
    c = rc.BY_NAME["members_5"]
    gs, mc, ms, mp, cams, it, hub = rc.args_of(c)
    out = capi.refine_lines_host(np.zeros(1, np.int32), mc[:0], ms[:0], mp[:0], cams, it, hub)
    assert len(out["line"]) == 0 and len(out["segs"]) == 0
    bad_cam = cams.copy()
    bad_cam[1, 2, 3] = np.inf
    for args in ((np.array([1, 5], np.int32), mc, ms, mp, cams, it, hub), (np.array([0, 5, 3], np.int32), mc, ms, mp, cams, it, hub),
                 (gs, mc + len(cams), ms, mp, cams, it, hub), (gs, mc - 1, ms, mp, cams, it, hub), (gs, mc, ms, mp, cams, -1, hub), (gs, mc, ms, mp, cams, it, -0.5),
                 (gs, mc, ms, mp, bad_cam, it, hub)):
        with pytest.raises(capi.L3DError) as e:
            capi.refine_lines_host(*args)
        assert e.value.code == 1


FACADE_SRC = r'''
#include "line3D_amd.hpp"
int main() {
    L3D::Line3D line3D("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false);
    line3D.setRefinement(true);
    line3D.setRefinement(true, 30, 1.5);
    line3D.compute3Dmodel(false);
    std::vector<double> before, after;
    std::vector<int> status;
    const bool ok = line3D.getRefinement(before, after, status);
    return ok ? (int)status.size() : 0;
}
'''


def test_facade_refinement_methods_compile():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.cpp")
        open(src, "w").write(FACADE_SRC)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])
