"""Crafted (camera, segment) sets for the projection (l3d_project_lines / l3d_test_project_lines_host; include/line3d_amd.h, "PROJECTION AND
OVERLAYS", 1), each built to be the case its name claims.  CASES: dict(name, seg3d (n, 6) float64, cams [(K, R, t, width, height)], near, margin,
claim) -- claim: (kind, ...) that tests/test_project_cases_cpu.py holds the case to, by the model of tests/project_model.py:
  ("counts", [per camera])        the outputs per camera
  ("flags", [flags])              exactly these flags, in output order
  ("exact", [[x1, y1, x2, y2]])   exactly these segments
  ("touch",)                      one pair, dropped with t0 == t1 after the four edges
REFUSALS: (name, keyword overrides of a good call, status, a word of the message)."""
import numpy as np

import project_model as pm

I3 = np.eye(3)
Z3 = np.zeros(3)


def cam(K=None, R=None, t=None, width=64, height=48, f=100.0):
    K = np.array([[f, 0.0, 32.0], [0.0, f, 24.0], [0.0, 0.0, 1.0]]) if K is None else np.asarray(K, np.float64)
    return (K, I3 if R is None else np.asarray(R, np.float64), Z3 if t is None else np.asarray(t, np.float64), width, height)


UNIT = cam(K=np.eye(3))                        # u = x / z, v = y / z: pixel values can be hit exactly


def _segs(*rows):
    return np.array(rows, np.float64).reshape(-1, 6)


def _roty(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _cloud(n, seed):
    """n segments in a box around the optical axes of the three cameras of _rig: some in view, some outside the images, some behind"""
    rng = np.random.default_rng(seed)
    P = rng.uniform([-3.0, -2.0, -2.0], [3.0, 2.0, 8.0], (n, 3))
    Q = P + rng.uniform(-1.5, 1.5, (n, 3))
    return np.concatenate([P, Q], axis=1)


def _rig():
    return [cam(), cam(R=_roty(0.3), t=[0.4, 0.0, 0.2], width=80, height=60), cam(K=[[90.0, 2.0, 30.5], [0.0, 95.0, 20.25], [0.0, 0.0, 1.0]], R=_roty(-0.25), t=[-0.3, 0.1, 0.0])]


CASES = [
    # ---- the near plane
    dict(name="near_both_behind", seg3d=_segs([0, 0, -1, 0.1, 0, -2]), cams=[cam()], near=1e-3, margin=0.0, claim=("counts", [0])),
    dict(name="near_p_behind", seg3d=_segs([0, 0, -1, 0.1, 0, 2]), cams=[cam()], near=1e-3, margin=0.0, claim=("flags", [1])),
    dict(name="near_q_behind", seg3d=_segs([0.1, 0, 2, 0, 0, -1]), cams=[cam()], near=1e-3, margin=0.0, claim=("flags", [2])),
    dict(name="near_z_exactly_near", seg3d=_segs([0, 0, 0.5, 0.1, 0, 2]), cams=[cam()], near=0.5, margin=0.0, claim=("flags", [0])),
    dict(name="near_through_the_centre", seg3d=_segs([-1, -1, -1, 1, 1, 1]), cams=[cam()], near=1e-3, margin=0.0, claim=("counts", [0])),
    # ---- the rectangle
    dict(name="rect_on_the_left_border", seg3d=_segs([-0.5, 1, 1, -0.5, 5, 1]), cams=[UNIT], near=1e-3, margin=0.0, claim=("exact", [[-0.5, 1, -0.5, 5]])),
    dict(name="rect_left_of_the_border", seg3d=_segs([-0.75, 1, 1, -0.75, 5, 1]), cams=[UNIT], near=1e-3, margin=0.0, claim=("counts", [0])),
    dict(name="rect_through_a_corner", seg3d=_segs([-1.5, 0.5, 1, 0.5, -1.5, 1]), cams=[UNIT], near=1e-3, margin=0.0, claim=("touch",)),
    dict(name="rect_crosses_four_borders", seg3d=_segs([-100, -80, 1, 200, 150, 1]), cams=[UNIT], near=1e-3, margin=0.0, claim=("flags", [3])),
    dict(name="rect_margin_keeps", seg3d=_segs([-5, 5, 1, -3, 20, 1]), cams=[UNIT], near=1e-3, margin=10.0, claim=("exact", [[-5, 5, -3, 20]])),
    dict(name="rect_no_margin_drops", seg3d=_segs([-5, 5, 1, -3, 20, 1]), cams=[UNIT], near=1e-3, margin=0.0, claim=("counts", [0])),
    # ---- inputs
    dict(name="input_p_equals_q", seg3d=_segs([0.1, 0.1, 2, 0.1, 0.1, 2]), cams=[cam()], near=1e-3, margin=0.0, claim=("counts", [0])),
    dict(name="input_1e12", seg3d=_segs([1e12, 0, 1e12, 0, 1e12, 1e12]), cams=[cam(f=10.0)], near=1e-3, margin=0.0, claim=("exact", [[42, 24, 32, 34]])),
    dict(name="input_nan_inf", seg3d=_segs([np.nan, 0, 2, 0.1, 0, 2], [0, 0, 2, np.inf, 0, 2], [0, 0, 2, 0.1, 0, -np.inf], [0, 0, 2, 0.1, 0, 2]), cams=[cam()],
         near=1e-3, margin=0.0, claim=("counts", [1])),
    dict(name="input_skewed_k", seg3d=_segs([0, 0, 2, 0.2, 0.2, 2], [-0.3, 0.1, 1, 0.3, 0.2, 3]), cams=[cam(K=[[100.0, 7.0, 32.0], [0.0, 90.0, 24.0], [0.0, 0.0, 1.0]])],
         near=1e-3, margin=0.0, claim=("counts", [2])),
    # ---- sizes
    dict(name="size_1x1", seg3d=_segs([0, 0, 2, 0.1, 0.1, 2]), cams=[cam()], near=1e-3, margin=0.0, claim=("counts", [1])),
    dict(name="size_empty_row", seg3d=_cloud(70, 11), cams=[cam(), cam(R=_roty(np.pi), t=[0.0, 0.0, -20.0]), cam(R=_roty(0.2))], near=1e-3, margin=0.0, claim=("empty_row", 1)),
    dict(name="size_n0", seg3d=np.zeros((0, 6)), cams=_rig()[:2], near=1e-3, margin=0.0, claim=("counts", [0, 0])),
    dict(name="size_m0", seg3d=_cloud(5, 3), cams=[], near=1e-3, margin=0.0, claim=("counts", [])),
] + [dict(name="size_3x%d" % n, seg3d=_cloud(n, 100 + n), cams=_rig(), near=1e-3, margin=2.0, claim=("mixed",)) for n in (63, 64, 65, 128, 129, 130)]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def same(got, want):
    """two results (seg2d, src_index, flags, cam_start) agree in every byte"""
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]))


_MODEL = {}


def model_of(case):
    """the model's result for a case, computed once"""
    if case["name"] not in _MODEL:
        _MODEL[case["name"]] = pm.project(case["seg3d"], case["cams"], case["near"], case["margin"])
    return _MODEL[case["name"]]


_GOOD = dict(seg3d=_segs([0, 0, 2, 0.1, 0.1, 2]), cams=[cam()], near=1e-3, margin=0.0)


def _bad_cam(**kw):
    K, R, t, w, h = cam()
    K = K.copy()
    if "k_row" in kw:
        K[2] = kw["k_row"]
    return [(K, R, t, kw.get("width", w), kw.get("height", h))]


REFUSALS = [
    ("k_third_row", dict(cams=_bad_cam(k_row=[0.0, 0.0, 2.0])), 1, "third row"),
    ("k_third_row_skewed", dict(cams=_bad_cam(k_row=[1e-9, 0.0, 1.0])), 1, "third row"),
    ("size_zero_width", dict(cams=_bad_cam(width=0)), 1, "size"),
    ("size_negative_height", dict(cams=_bad_cam(height=-3)), 1, "size"),
    ("near_zero", dict(near=0.0), 1, "near"),
    ("near_negative", dict(near=-1.0), 1, "near"),
    ("near_nan", dict(near=float("nan")), 1, "near"),
    ("near_inf", dict(near=float("inf")), 1, "near"),
    ("margin_negative", dict(margin=-0.5), 1, "margin"),
    ("margin_nan", dict(margin=float("nan")), 1, "margin"),
    ("margin_huge", dict(margin=2.0 ** 31), 1, "margin"),
]


def refusal_arguments(overrides):
    kw = dict(_GOOD)
    kw.update(overrides)
    return kw
