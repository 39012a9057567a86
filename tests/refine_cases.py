"""Crafted groups for the line refinement (l3d_refine_lines / l3d_test_refine_host), each named for what it exercises.  A case is a dict of the call's
arguments (group_start, member_cam, member_seg float32, member_pts, cameras, max_iterations, huber_px) plus, per group, what it was built from
(`truth`: point, unit direction, extent) and the facts tests/test_refine_cases_cpu.py asserts about it with the model.

A group observes a 3-D line of extent E from cameras K [R | t] (focal length 800 px, principal point (512, 384)) on a ring of radius 3 E around it.
Member m covers a stretch [s1, s2] of the line; its 2-D segment is the projection of the two end points (+ pixel noise, rounded to float32), its
hypothesis points are the 3-D end points (+ noise: the scatter of two-view triangulations) or lie on a deliberately perturbed line.  The 2 n end-point
parameters of a group come from a grid of 2 n distinct values: no two sort keys tie."""
import numpy as np

F_PX, PP = 800.0, (512.0, 384.0)
K = np.array([[F_PX, 0, PP[0]], [0, F_PX, PP[1]], [0, 0, 1.0]])
MEMBER_COUNTS = [4, 5, 63, 64, 65, 127, 128, 129, 300]


def look_at(C, target, up=(0.0, 0.0, 1.0)):
    """P = K [R | -R C] of a camera at C looking at target"""
    z = np.asarray(target, float) - C
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, float))
    if np.linalg.norm(x) < 1e-6:
        x = np.cross(z, np.array([0.0, 1.0, 0.0]))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.hstack([K @ R, (-K @ R @ C)[:, None]])


def project(P, X):
    h = P[:, :3] @ X + P[:, 3]
    return h[:2] / h[2]


def rotate(v, axis, angle):
    axis = axis / np.linalg.norm(axis)
    return v * np.cos(angle) + np.cross(axis, v) * np.sin(angle) + axis * (axis @ v) * (1 - np.cos(angle))


def ring_cameras(rng, L0, e, E, n_cams):
    """cameras around the line: azimuths spread over 200 degrees, shifted along the line, all looking at its middle"""
    u = np.cross(e, [0.0, 0.0, 1.0] if abs(e[2]) < 0.9 else [1.0, 0.0, 0.0])
    u = u / np.linalg.norm(u)
    v = np.cross(e, u)
    cams = []
    for c in range(n_cams):
        az = np.deg2rad(-100 + 200 * (c + 0.5) / n_cams + rng.uniform(-5, 5))
        C = L0 + 3 * E * (np.cos(az) * u + np.sin(az) * v) + e * E * rng.uniform(-0.8, 0.8)
        cams.append(look_at(C, L0 + e * E * rng.uniform(-0.1, 0.1)))
    return cams


def stretches(rng, n, E):
    """(s1, s2) per member from a grid of 2 n distinct parameters: starts from the lower half, ends from the upper half -- every member covers the middle"""
    grid = ((np.arange(2 * n) + 0.5) / (2 * n) - 0.5) * E
    lo = rng.permutation(np.arange(0, n))
    hi = rng.permutation(np.arange(n, 2 * n))
    return np.stack([grid[lo], grid[hi]], axis=1)


def make_group(seed, n, n_cams, E=2.0, L0=(0.3, -0.2, 0.1), e=(0.8, 0.5, 0.33), noise_px=0.3, noise_3d=0.01, start=None, cams=None, member_cam=None):
    """start: None -- hypothesis points = true points + noise_3d * E gaussian; (angle_deg, shift) -- points ON the true line rotated by angle about its middle
    and shifted by shift * E"""
    rng = np.random.default_rng(seed)
    L0, e = np.asarray(L0, float), np.asarray(e, float)
    e = e / np.linalg.norm(e)
    cams = ring_cameras(rng, L0, e, E, n_cams) if cams is None else cams
    mc = np.sort(np.arange(n) % len(cams)) if member_cam is None else np.asarray(member_cam)
    st = stretches(rng, n, E)
    seg, pts = np.zeros((n, 4), np.float32), np.zeros((n, 6))
    if start is not None:
        ax = np.cross(e, [0.0, 0.0, 1.0])
        e2 = rotate(e, ax, np.deg2rad(start[0]))
        off = start[1] * E * ax / np.linalg.norm(ax)
    for m in range(n):
        for j in range(2):
            X = L0 + st[m, j] * e
            seg[m, 2 * j:2 * j + 2] = (project(cams[mc[m]], X) + noise_px * rng.standard_normal(2)).astype(np.float32)
            pts[m, 3 * j:3 * j + 3] = X + noise_3d * E * rng.standard_normal(3) if start is None else L0 + off + st[m, j] * e2
    return {"member_cam": mc.astype(np.int32), "member_seg": seg, "member_pts": pts, "cameras": np.array(cams), "truth": (L0, e, E)}


def pack(name, groups, max_iterations=20, huber_px=2.0, **facts):
    """groups with a camera table each -> one call's arguments"""
    gs, mc, ms, mp, cams, off = [0], [], [], [], [], 0
    for g in groups:
        mc.append(g["member_cam"] + off)
        ms.append(g["member_seg"])
        mp.append(g["member_pts"])
        cams.append(g["cameras"])
        off += len(g["cameras"])
        gs.append(gs[-1] + len(g["member_cam"]))
    case = {"name": name, "group_start": np.array(gs, np.int32), "member_cam": np.concatenate(mc).astype(np.int32), "member_seg": np.concatenate(ms).astype(np.float32),
            "member_pts": np.concatenate(mp), "cameras": np.concatenate(cams), "max_iterations": max_iterations, "huber_px": huber_px,
            "truth": [g["truth"] for g in groups], "n_groups": len(groups)}
    case.update(facts)
    return case


def _exact_axis_group(n, cam_special, special_segs, seed):
    """a group whose START is exactly the x axis through the origin: hypothesis points on the axis at dyadic parameters, mirrored so that their sum is exactly 0
    (line_of_points then gives Pc = 0 and dir = (1, 0, 0) without a rounding).  The 2-D segments observe the TRUE line: the axis rotated by 2 degrees and shifted.
    cam_special: a camera with small-integer or exactly parallel geometry, appended as the LAST camera; special_segs: its members' (s1, s2) or explicit 2-D segments"""
    rng = np.random.default_rng(seed)
    E, L0, e0 = 2.0, np.zeros(3), np.array([1.0, 0.0, 0.0])
    cams = ring_cameras(rng, L0, e0, E, 5) + [cam_special]
    half = n // 2
    a = (rng.permutation(np.arange(8, 8 + 2 * half))[:half] * 32 + 1) / 1024.0            # distinct dyadic values in (0, 1)
    b = (rng.permutation(np.arange(8, 8 + 2 * half))[:half] * 32 + 3) / 1024.0
    st = np.concatenate([np.stack([-a, b], 1), np.stack([-b, a], 1)])                     # mirrored pairs: every coordinate has its negative in the set
    n = len(st)
    mc = np.sort(np.arange(n) % 5)
    e_true = rotate(e0, np.array([0.0, 0.3, 1.0]), np.deg2rad(2.0))
    off = np.array([0.0, 0.012, -0.016])                                                   # 1 % of the extent
    seg, pts = np.zeros((n, 4), np.float32), np.zeros((n, 6))
    for m in range(n):
        for j in range(2):
            pts[m, 3 * j] = st[m, j]
            seg[m, 2 * j:2 * j + 2] = project(cams[mc[m]], off + st[m, j] * e_true).astype(np.float32)
    return {"member_cam": mc.astype(np.int32), "member_seg": seg, "member_pts": pts, "cameras": np.array(cams), "truth": (off, e_true, E)}, special_segs


def _camera_on_line_case():
    # the camera of integer entries at C = (4, 0, 0) looking along -x: x axis (0, 1, 0), y axis (0, 0, -1), z axis (-1, 0, 0).  M's first column g = (-512, -384, -1);
    # p4 = -M C = -4 g exactly.  At the start (A = 0, d = e_x): p = p4 = -4 g, so l = p x g = 0 without a rounding: n2 = 0, the member is dropped
    R = np.array([[0.0, 1, 0], [0, 0, -1], [-1, 0, 0]])
    C = np.array([4.0, 0, 0])
    P = np.hstack([K @ R, (-K @ R @ C)[:, None]])
    g, _ = _exact_axis_group(12, P, None, 71)
    # one more member, of that camera, at the end of the list (its camera index 5 is the largest: key order holds); its points mirror each other
    s = (-0.40625, 0.40625)
    off, e_true, _ = g["truth"]
    seg = np.concatenate([project(P, off + s[0] * e_true), project(P, off + s[1] * e_true)]).astype(np.float32)
    g["member_cam"] = np.append(g["member_cam"], 5).astype(np.int32)
    g["member_seg"] = np.vstack([g["member_seg"], seg[None]])
    g["member_pts"] = np.vstack([g["member_pts"], [[s[0], 0, 0, s[1], 0, 0]]])
    return pack("camera_on_line", [g], dropped_member=len(g["member_cam"]) - 1)


def _parallel_ray_case():
    # a camera whose z axis is (0.8, 0.6, 0): the direction e_x has the vanishing point (800 * 0.6 / 0.8 + 512, 384) = (1112, 384), exact in float32.  The group
    # starts exactly on the x axis (as in camera_on_line) and makes no trial (max_iterations 0), so the line the points are taken onto has d = e_x without a
    # rounding; one member of that camera has its second end point AT the vanishing point: its viewing ray is parallel to the line, den <= 1e-12 q.q, and t falls
    # back to d . (X - A).  (A refined direction is only known to about 1e-7 rad, and 1e-12 in den / q.q is 1e-6 rad: a case that iterates could land on either
    # side.  With noise-free 2-D data the relative difference of rms_after is ill-conditioned as well.)
    R = np.array([[0.6, -0.8, 0], [0, 0, -1.0], [0.8, 0.6, 0]])
    C = np.array([-2.0, -5.0, 0.5])
    P = np.hstack([K @ R, (-K @ R @ C)[:, None]])
    g, _ = _exact_axis_group(12, P, None, 72)
    s = (-0.40625, 0.40625)
    off, e_true, _ = g["truth"]
    seg = np.concatenate([project(P, off + s[0] * e_true), [1112.0, 384.0]]).astype(np.float32)
    g["member_cam"] = np.append(g["member_cam"], 5).astype(np.int32)
    g["member_seg"] = np.vstack([g["member_seg"], seg[None]])
    g["member_pts"] = np.vstack([g["member_pts"], [[s[0], 0, 0, s[1], 0, 0]]])
    return pack("parallel_ray", [g], max_iterations=0, parallel_point=2 * (len(g["member_cam"]) - 1) + 1)


def _one_centre_case():
    rng = np.random.default_rng(73)
    L0, e, E = np.array([0.3, -0.2, 0.1]), np.array([0.8, 0.5, 0.33]) / np.linalg.norm([0.8, 0.5, 0.33]), 2.0
    C = L0 + np.array([1.0, -5.0, 2.0])
    cams = [look_at(C, L0 + e * s + 0.3 * rng.standard_normal(3)) for s in (-0.4, -0.2, 0.0, 0.2, 0.4)]
    return pack("one_centre", [make_group(73, 10, 5, cams=cams)])


def _outlier_group():
    g = make_group(61, 12, 5, noise_px=0.3)
    # member 7's 2-D segment is another line's: 40 px aside
    s = g["member_seg"][7].astype(np.float64)
    nrm = np.array([-(s[3] - s[1]), s[2] - s[0]])
    nrm = 40.0 * nrm / np.linalg.norm(nrm)
    g["member_seg"][7] = (s + np.concatenate([nrm, nrm])).astype(np.float32)
    return g


def build_cases():
    cases = []
    for n in MEMBER_COUNTS:                                             # the lane stride, the LDS bound on both sides, the global scratch
        cases.append(pack("members_%d" % n, [make_group(100 + n, n, min(12, max(4, n // 2)))]))
    singles = [make_group(200 + i, n, 5) for i, n in enumerate([6, 9, 70, 130, 7])]
    cases.append(pack("groups_4", singles[:4]))                        # one full workgroup
    cases.append(pack("groups_5", singles))                            # ... and one wave of the next
    probe = make_group(300, 66, 6)
    cases.append(pack("position_first", [probe] + singles[:4], probe_at=0))
    cases.append(pack("position_middle", singles[:2] + [probe] + singles[2:4], probe_at=2))
    cases.append(pack("position_last", singles[:4] + [probe], probe_at=4))
    cases.append(pack("same_camera_2_3", [make_group(41, 9, 5, member_cam=[0, 0, 1, 1, 1, 2, 3, 4, 4])]))
    cases.append(pack("three_cameras", [make_group(42, 5, 3, member_cam=[0, 0, 1, 2, 2])]))
    cases.append(pack("noise_free_perturbed", [make_group(43, 14, 6, noise_px=0.0, start=(2.0, 0.01))], noise_free=True))
    cases.append(pack("noise_half_px", [make_group(44, 20, 6, noise_px=0.5)]))
    cases.append(pack("outlier_huber_2", [_outlier_group()], huber_px=2.0, outlier_member=7))
    cases.append(pack("outlier_huber_0", [_outlier_group()], huber_px=0.0, outlier_member=7))
    cases.append(pack("far_from_origin", [make_group(45, 12, 5, L0=(1.0e4, -2.0e4, 5.0e3))]))
    cases.append(pack("extent_1e-3", [make_group(46, 12, 5, E=1e-3, L0=(3e-4, -2e-4, 1e-4))]))
    cases.append(_camera_on_line_case())
    cases.append(_parallel_ray_case())
    cases.append(_one_centre_case())
    nan_groups = [make_group(51, 8, 5), make_group(52, 10, 5), make_group(53, 8, 5)]
    clean = pack("nan_neighbours_alone", [nan_groups[0], nan_groups[2]])
    nan_groups[1]["member_pts"][3, 4] = np.nan
    cases.append(pack("nan_in_points", nan_groups, nan_group=1, clean_name="nan_neighbours_alone"))
    cases.append(clean)
    cases.append(pack("max_iterations_0", [make_group(54, 10, 5)], max_iterations=0))
    cases.append(pack("max_iterations_1", [make_group(54, 10, 5)], max_iterations=1))
    return cases


CASES = build_cases()
BY_NAME = {c["name"]: c for c in CASES}


def args_of(case):
    return (case["group_start"], case["member_cam"], case["member_seg"], case["member_pts"], case["cameras"], case["max_iterations"], case["huber_px"])


def group_slices(case):
    gs = case["group_start"]
    return [slice(int(gs[g]), int(gs[g + 1])) for g in range(case["n_groups"])]


def extent_of(case, g):
    return float(case["truth"][g][2])


def reordered(case, g, order):
    """group g of the case alone, its members in another order (an index array)"""
    sl = group_slices(case)[g]
    idx = np.arange(sl.start, sl.stop)[np.asarray(order)]
    return (np.array([0, len(idx)], np.int32), case["member_cam"][idx], case["member_seg"][idx], case["member_pts"][idx], case["cameras"], case["max_iterations"], case["huber_px"])


_MODEL_CACHE = {}


def model_of(case):
    """the model's result per group, computed once per distinct group (the position cases share theirs)"""
    import refine_model as rm
    out = []
    for sl in group_slices(case):
        key = (case["member_cam"][sl].tobytes(), case["member_seg"][sl].tobytes(), case["member_pts"][sl].tobytes(), case["cameras"].tobytes(), case["max_iterations"], case["huber_px"])
        if key not in _MODEL_CACHE:
            _MODEL_CACHE[key] = rm.refine_group(case["member_cam"][sl], case["member_seg"][sl], case["member_pts"][sl], case["cameras"], case["max_iterations"], case["huber_px"])
        out.append(_MODEL_CACHE[key])
    return out


QUANTITIES = ("angle", "offset", "rms", "points")


def differences(a, b, extent):
    """two results of one group (dicts with line, rms_after, segs) -> the four compared quantities: angle between the directions (sine), distance of the As over the
    extent, relative difference of rms_after, largest difference of an emitted end-point coordinate over the extent (inf when the counts differ)"""
    la, lb = np.asarray(a["line"]), np.asarray(b["line"])
    sa, sb = np.asarray(a["segs"]).reshape(-1, 6), np.asarray(b["segs"]).reshape(-1, 6)
    ra, rb = float(a["rms_after"]), float(b["rms_after"])
    return {"angle": float(np.linalg.norm(np.cross(la[3:], lb[3:]))), "offset": float(np.linalg.norm(la[:3] - lb[:3]) / extent),
            "rms": abs(ra - rb) / max(abs(ra), abs(rb)) if max(abs(ra), abs(rb)) > 0 else 0.0,
            "points": (float(np.abs(sa - sb).max() / extent) if len(sa) else 0.0) if len(sa) == len(sb) else float("inf")}


_TOL = None


def tolerance():
    """tests/golden/refine_tolerance.json (written by tests/golden/make_golden_refine.py)"""
    global _TOL
    if _TOL is None:
        import json
        import os
        _TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_tolerance.json")))
    return _TOL


def per_group(out, g):
    """group g of a product result as the model's dict"""
    k0 = int(out["seg_count"][:g].sum())
    return {"line": out["line"][g], "rms_before": out["rms_before"][g], "rms_after": out["rms_after"][g], "iterations": int(out["iterations"][g]),
            "status": int(out["status"][g]), "segs": out["segs"][k0:k0 + int(out["seg_count"][g])]}


def check_against_model(case, out):
    """a product result (host or device) against the model, within the recorded tolerance; segment counts and status equal"""
    for g, m in enumerate(model_of(case)):
        got, tol = per_group(out, g), tolerance()["cases"][case["name"]][g]
        what = "%s group %d" % (case["name"], g)
        assert got["status"] == m["status"], what
        assert len(got["segs"]) == len(m["segs"]), what
        if tol is None:                                                 # not finite: status 2, nothing emitted, NaN line
            assert got["status"] == 2 and np.all(np.isnan(got["line"])) and np.isnan(got["rms_after"]) and got["iterations"] == 0, what
            continue
        assert abs(got["rms_before"] - m["rms_before"]) <= tol["tolerance"]["rms"] * m["rms_before"] + 1e-300, what
        d = differences(got, m, extent_of(case, g))
        for q in QUANTITIES:
            assert d[q] <= tol["tolerance"][q], "%s: %s differs by %.3g, tolerance %.3g" % (what, q, d[q], tol["tolerance"][q])
