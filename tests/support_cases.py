"""Crafted inputs for the support search (l3d_support_lines / l3d_test_support_lines_host; include/line3d_amd.h, "SUPPORT OF 3-D LINES"), each built to be
the case its name claims.  CASES: dict(name, seg3d (n, 6) float64, cams [(K, R, t, width, height)], segs [one (k, 4) float32 array per camera], p:
dict(dist_px, cos_min, min_overlap, near, margin), claim) -- claim: a dict that tests/test_support_cases_cpu.py holds the case to, by the model of
tests/support_model.py:
  rows=[per camera]      the rows per camera            cols=[per camera]        the columns per camera
  records=[(c, k, j)]    exactly these records          best=[...]               exactly this best array
  terms=dict(...)        exact values of row 0 against column 0 of camera 0: cs, e (the larger), ov, Lm
  ineligible=[j]         these columns of camera 0 are not eligible
  clipped=True           row 0 of camera 0 has t0 > 0
  rows_min / records_min lower bounds, for the sized tables
REFUSALS: (name, keyword overrides of a good call, status, a word of the message)."""
import math

import numpy as np

import project_cases as pc
import support_model as sm

F = np.float64
COS5 = math.cos(5.0 * math.pi / 180.0)
UNIT = pc.UNIT                                 # K = I, 64 x 48: a point (x, y, 1) has the pixel (x, y) exactly
up = lambda x: float(np.nextafter(F(x), F(np.inf)))
down = lambda x: float(np.nextafter(F(x), F(-np.inf)))

CASES = []


def P(dist_px=3.0, cos_min=COS5, min_overlap=0.5, near=1e-3, margin=0.0):
    return dict(dist_px=dist_px, cos_min=cos_min, min_overlap=min_overlap, near=near, margin=margin)


def case(name, seg3d, cams, segs, p, **claim):
    CASES.append(dict(name=name, seg3d=np.array(seg3d, F).reshape(-1, 6), cams=list(cams), segs=[np.array(s, np.float32).reshape(-1, 4) for s in segs], p=p, claim=claim))


def flat(*rows):
    """3-D segments in the plane z = 1 from (x1, y1, x2, y2): their pixels in UNIT are these numbers"""
    return [[r[0], r[1], 1.0, r[2], r[3], 1.0] for r in rows]


def _rig(m):
    """m cameras looking down +z from slightly different places, 64 x 48"""
    return [pc.cam(t=[0.05 * c - 0.1, 0.02 * c, 0.1 * c], f=60.0 + 5.0 * c) for c in range(m)]


def _table(n, col_counts, seed, supported=0.6, p=None):
    """n 3-D segments in front of len(col_counts) cameras (n >= 4: some behind them); camera c gets col_counts[c] 2-D segments: noisy stretches of
    projected rows (records exist) and random ones"""
    rng = np.random.default_rng(seed)
    p = p or P()
    A = rng.uniform([-0.4, -0.3, 1.0], [0.4, 0.3, 2.0], (n, 3))
    seg3d = np.concatenate([A, A + rng.uniform(-0.5, 0.5, (n, 3))], axis=1)
    seg3d[3::7, 2] = -1.0
    seg3d[3::7, 5] = -2.0                          # every seventh behind every camera: lanes without a row
    cams = _rig(len(col_counts))
    segs = []
    for cam, k in zip(cams, col_counts):
        rows = [r for r in (sm.row(cam, s, p["near"], p["margin"]) for s in seg3d) if r is not None]
        out = np.zeros((k, 4), np.float32)
        for j in range(k):
            if rows and (j < 2 or j == k - 1 or rng.random() < supported):
                r = rows[-1] if j == 0 else rows[0] if j == 1 else rows[int(rng.integers(len(rows)))]      # (the last and the first row are supported, and so is the last column)
                a, b = np.sort(rng.uniform(0.0, 1.0, 2))
                b = max(b, a + 0.3)
                forced = j < 2 or j == k - 1
                if forced:
                    a, b = 0.2, 0.8
                X = np.array(r["A"], F)[None] + np.array([[a], [b]]) * (np.array(r["B"], F) - np.array(r["A"], F))[None]
                out[j] = (X + rng.normal(0.0, 0.05 if forced else 0.4, (2, 2))).reshape(4)
            else:
                out[j] = rng.uniform([0, 0, 0, 0], [64, 48, 64, 48])
        segs.append(out)
    return seg3d, cams, segs, p


# ---- sizes: the rows of a workgroup and a wave, the column tiles
for n in (1, 63, 64, 65, 257):
    s3, cams, segs, p = _table(n, [40], 100 + n)
    case("rows_%d" % n, s3, cams, segs, p, rows_min=(n * 3) // 4, records_min=1 if n > 1 else 0, cols=[40])
for k in (0, 1, 255, 256, 257, 513):
    s3, cams, segs, p = _table(20, [k], 200 + k, supported=1.0 if k == 1 else 0.6)
    case("columns_%d" % k, s3, cams, segs, p, rows_min=15, records_min=min(k, 1), cols=[k])
s3, cams, segs, p = _table(70, [130, 0, 300], 31)
case("three_cameras_one_without_segments", s3, cams, segs, p, rows_min=150, records_min=50, cols=[130, 0, 300])

# ---- a camera for which every row is dropped (the other camera keeps the call from being empty)
_two = flat([2, 5, 30, 5], [3, 20, 40, 22])
_cols2 = [[2, 5, 30, 5], [3, 20, 40, 22], [10, 10, 20, 10]]
case("every_row_behind_the_near_plane", _two, [pc.cam(K=np.eye(3), R=pc._roty(np.pi)), UNIT], [_cols2, _cols2], P(), rows=[0, 2])
case("every_row_outside_the_rectangle", flat([-30, 5, -5, 5], [3, 60, 40, 70]), [UNIT, pc.cam(K=np.eye(3), width=200, height=200)], [_cols2, [[3, 60, 40, 70]]], P(margin=1.0), rows=[0, 1])
case("every_row_touches_a_corner_only", [[-1.5, 0.5, 1, 0.5, -1.5, 1]], [UNIT, pc.cam(K=np.eye(3), t=[2.0, 2.0, 0.0])], [_cols2, [[0.5, 2.5, 2.5, 0.5]]], P(), rows=[0, 1], touch=True)

# ---- the three decisions at their edges, both outcomes.  Row 0: (0, 0) -> (16, 0), so A = (0, 0), da = (1, 0), La = 16, all exact
ROW = flat([0, 0, 16, 0])
case("e_equals_dist_px_passes", ROW, [UNIT], [[[2, 3, 10, 3]]], P(dist_px=3.0), records=[(0, 0, 0)], terms=dict(e=3.0))
case("e_one_ulp_above_dist_px_fails", ROW, [UNIT], [[[2, 3, 10, 3]]], P(dist_px=down(3.0)), records=[], terms=dict(e=3.0))
case("e_of_the_second_end_decides", ROW, [UNIT], [[[2, 1, 10, 3]]], P(dist_px=down(3.0), cos_min=0.5), records=[], terms=dict(e=3.0))
# db = (3 / 5, 4 / 5): the cosine is the double 3 / 5
case("cosine_equals_cos_min_passes", ROW, [UNIT], [[[4, 0, 7, 4]]], P(dist_px=5.0, cos_min=3.0 / 5.0), records=[(0, 0, 0)], terms=dict(cs=3.0 / 5.0))
case("cosine_one_ulp_below_cos_min_fails", ROW, [UNIT], [[[4, 0, 7, 4]]], P(dist_px=5.0, cos_min=up(3.0 / 5.0)), records=[], terms=dict(cs=3.0 / 5.0))
case("cosine_is_taken_as_absolute_value", ROW, [UNIT], [[[7, 4, 4, 0]]], P(dist_px=5.0, cos_min=3.0 / 5.0), records=[(0, 0, 0)], terms=dict(cs=3.0 / 5.0))
# sU = 12, sV = 20: ov = 16 - 12 = 4, Lb = 8, Lm = 8; 0.5 x 8 = 4 exactly
case("overlap_equals_min_overlap_times_Lm_passes", ROW, [UNIT], [[[12, 1, 20, 1]]], P(min_overlap=0.5), records=[(0, 0, 0)], terms=dict(ov=4.0, Lm=8.0))
case("overlap_one_ulp_below_fails", ROW, [UNIT], [[[12, 1, 20, 1]]], P(min_overlap=up(0.5)), records=[], terms=dict(ov=4.0, Lm=8.0))

# ---- columns that are not eligible, between good ones
case("ineligible_columns", ROW, [UNIT], [[[2, 1, 10, 1], [5, 0, 5, 0], [np.nan, 0, 9, 0], [2, 0, np.inf, 0], [2, -1, 10, -1], [1, 0, 2, -np.inf]]], P(),
     records=[(0, 0, 0), (0, 0, 4)], ineligible=[1, 2, 3, 5], cols_eligible=2)

# ---- a row clipped by the rectangle: the supporter on the kept part passes, the one on the clipped part fails
case("clipped_row", flat([-20.5, 10, 40, 10]), [UNIT], [[[5, 10, 30, 10], [-18, 10, -4, 10]]], P(), records=[(0, 0, 0)], clipped=True)

# ---- the best row: two rows tied in dist for column 0 (the lower k wins); for column 1 the later row is nearer
case("best_row_tie_and_order", flat([0, 0, 16, 0], [0, 0, 16, 0], [0, 2, 16, 2]), [UNIT], [[[2, 1, 10, 1], [2, 2.5, 10, 2.5]]], P(),
     records=[(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 2, 0), (0, 2, 1)], best=[0, 2])

# ---- parameters at 0
case("dist_px_zero", ROW, [UNIT], [[[2, 0, 10, 0], [2, 2.0 ** -20, 10, 0]]], P(dist_px=0.0), records=[(0, 0, 0)], terms=dict(e=0.0))
case("min_overlap_zero", ROW, [UNIT], [[[16, 0, 20, 0], [18, 0, 22, 0]]], P(min_overlap=0.0), records=[(0, 0, 0)], terms=dict(ov=0.0))
case("cos_min_zero", ROW, [UNIT], [[[8, -1, 8, 1]]], P(cos_min=0.0, min_overlap=0.0), records=[(0, 0, 0)], terms=dict(cs=0.0, ov=0.0))

# ---- a 2-D segment longer than the projected line: Lm is La
case("segment_longer_than_the_projected_line", flat([4, 0, 8, 0]), [UNIT], [[[0, 0.5, 16, 0.5]]], P(), records=[(0, 0, 0)], terms=dict(ov=4.0, Lm=4.0), overlap=1.0)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def model_of(case):
    """the model's result for a case, computed once"""
    if "model" not in case:
        p = case["p"]
        case["model"] = sm.support(case["seg3d"], case["cams"], case["segs"], p["dist_px"], p["cos_min"], p["min_overlap"], p["near"], p["margin"])
    return case["model"]


def params_of(p):
    from line3d_amd import capi
    return capi.support_params(dist_px=p["dist_px"], cos_min=p["cos_min"], min_overlap=p["min_overlap"], near_z=p["near"], margin=p["margin"])


def same(got, exp):
    """bit for bit: records, cam_start, best, counts"""
    kinds = dict(records=sm.RECORD, cam_start=np.int64, best=np.int32, counts=np.int64)
    return all(np.asarray(got[k]).dtype == kinds[k] and np.asarray(got[k]).shape == np.asarray(exp[k]).shape
               and np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes() for k in kinds)


# (name, overrides of a good call, code, a word of the cause)
GOOD = dict(seg3d=np.array(ROW, F), cams=[UNIT], segs=[np.array([[2, 1, 10, 1]], np.float32)], p=P())


def _bad_cam(**kw):
    K, R, t, w, h = UNIT
    K = np.array(K, F)
    if "k_row" in kw:
        K[2] = kw["k_row"]
    return [(K, R, t, kw.get("width", w), kw.get("height", h))]


REFUSALS = [
    ("dist_px_negative", dict(p=P(dist_px=-1.0)), 1, "dist_px"),
    ("dist_px_nan", dict(p=P(dist_px=float("nan"))), 1, "dist_px"),
    ("dist_px_infinite", dict(p=P(dist_px=float("inf"))), 1, "dist_px"),
    ("cos_min_above_one", dict(p=P(cos_min=1.5)), 1, "cos_min"),
    ("cos_min_negative", dict(p=P(cos_min=-0.1)), 1, "cos_min"),
    ("cos_min_nan", dict(p=P(cos_min=float("nan"))), 1, "cos_min"),
    ("min_overlap_above_one", dict(p=P(min_overlap=1.01)), 1, "min_overlap"),
    ("min_overlap_negative", dict(p=P(min_overlap=-0.5)), 1, "min_overlap"),
    ("min_overlap_nan", dict(p=P(min_overlap=float("nan"))), 1, "min_overlap"),
    ("k_third_row", dict(cams=_bad_cam(k_row=[0.0, 0.0, 2.0])), 1, "third row"),
    ("size_zero_width", dict(cams=_bad_cam(width=0)), 1, "size"),
    ("near_zero", dict(p=P(near=0.0)), 1, "near"),
    ("near_nan", dict(p=P(near=float("nan"))), 1, "near"),
    ("margin_negative", dict(p=P(margin=-0.5)), 1, "margin"),
    ("margin_huge", dict(p=P(margin=2.0 ** 31)), 1, "margin"),
]


def refusal_arguments(overrides):
    kw = dict(GOOD)
    kw.update(overrides)
    return kw


# refusals that only the C call can be given: (name, what to change in raw_arguments(), code, a word of the cause)
RAW_REFUSALS = [
    ("negative_n", dict(n=-1), 1, "negative count"),
    ("negative_m", dict(m=-1), 1, "negative count"),
    ("null_seg3d", dict(seg3d=None), 1, "null input"),
    ("null_cameras", dict(cams=None), 1, "null input"),
    ("null_seg_start", dict(start=None), 1, "seg_start"),
    ("seg_start_not_from_zero", dict(start=np.array([1, 2], np.int64)), 1, "begin at 0"),
    ("seg_start_descends", dict(start=np.array([0, 1, 0], np.int64), m=2, two_cams=True), 1, "descends"),
    ("null_seg2d", dict(cols=None), 1, "2-D segments"),
    ("null_params", dict(prm=None), 1, "null parameters"),
]


def raw_arguments(change):
    """(seg_ptr, n, cams, m, seg2d_ptr, start, prm) for capi._support_call: a good call with one thing changed"""
    from line3d_amd import capi
    keep = {}
    keep["s"] = np.ascontiguousarray(GOOD["seg3d"], F)
    keep["cols"] = np.ascontiguousarray(GOOD["segs"][0], np.float32)
    keep["cams"] = capi.cameras([UNIT, UNIT] if change.get("two_cams") else [UNIT])
    a = dict(seg3d=capi._p(keep["s"]), n=1, cams=keep["cams"], m=1, cols=capi._p(keep["cols"]), start=np.array([0, 1], np.int64), prm=params_of(GOOD["p"]))
    a.update({k: v for k, v in change.items() if k != "two_cams"})
    return (a["seg3d"], a["n"], a["cams"], a["m"], a["cols"], a["start"], a["prm"]), keep
