"""Crafted tables for the junctions of 3-D lines (include/line3d_amd.h, "JUNCTIONS OF 3-D LINES"), each named for the case it is;
tests/test_junction_cases_cpu.py checks with the model that every table is what its name claims.  The decision points are built from exactly
representable numbers: a probe line along x and a second line along y whose foot on the probe's axis is the tested parameter, exactly."""
import math

import numpy as np

import junction_model as jm

F = np.float64
COS10 = math.cos(10.0 * math.pi / 180.0)
up = lambda x: float(np.nextafter(F(x), F(np.inf)))
dn = lambda x: float(np.nextafter(F(x), F(-np.inf)))

CASES = []


def case(name, lines, tol, ext, claim, cos_max=COS10, crossings=0):
    lines = np.asarray(lines, F).reshape(-1, 6)
    tol = np.full(len(lines), tol, F) if np.isscalar(tol) else np.asarray(tol, F)
    ext = np.full(len(lines), ext, F) if np.isscalar(ext) else np.asarray(ext, F)
    assert len(tol) == len(lines) == len(ext)
    CASES.append(dict(name=name, lines=lines, tol=tol, ext=ext, cos_max=float(cos_max), crossings=int(crossings), claim=claim))


def chunks(n):
    """the column chunks of the device search (junction::chunks)"""
    tiles = (n + 255) // 256
    if tiles >= 512:
        return 1
    c = min((1024 + tiles - 1) // max(tiles, 1), tiles, 64)
    if n > 0:
        c = min(c, (1 << 30) // n)
    return max(c, 1)


def corners(n, seed, offset=0.0):
    """n lines: the edges of max(1, n // 3) corners with random frames; line k is an edge of corner k mod m along the frame's axis (k // m) mod 3, so
    the edges of one corner lie m apart: in different waves and, from n = 513 on, in different tiles.  An edge starts up to 0.05 short of its corner
    or overshoots it by up to 0.02, up to 0.005 beside it; every fourth runs towards the corner"""
    rng = np.random.default_rng(seed)
    m = max(1, n // 3)
    c = rng.uniform(-5, 5, (m, 3)) + offset
    frames = np.linalg.qr(rng.normal(size=(m, 3, 3)))[0]
    out = np.zeros((n, 6))
    for k in range(n):
        a = frames[k % m][:, (k // m) % 3]
        P = c[k % m] + a * rng.uniform(-0.02, 0.05) + rng.uniform(-0.005, 0.005, 3)
        Q = P + a * rng.uniform(1, 3)
        out[k] = np.hstack([Q, P]) if k % 4 == 3 else np.hstack([P, Q])
    return out


def fan(count, nx, step, base=(0.25, -0.5, 1.5)):
    """`count` lines that all start at one point, in directions (x, y, 1) over a grid of nx columns with the given step: neighbours lie at least
    step / 1.5 radians apart while the grid stays within 0.71 of the axis, and no two directions are opposite"""
    k = np.arange(count)
    d = np.stack([(k % nx - nx // 2) * step, (k // nx) * step - 0.5 * step * (count // nx), np.ones(count)], axis=1)
    d /= np.linalg.norm(d, axis=1)[:, None]
    P = np.tile(np.asarray(base, F), (count, 1))
    return np.hstack([P, P + d * (1.0 + (k % 7)[:, None] * 0.25)])


SIZES = (1, 2, 64, 65, 256, 257, 300, 513)
for n in SIZES:
    case("size_%d" % n, corners(n, 200 + n), 0.05, 0.1, ("size", n))

# ---- the three kinds
case("box_corner", [[0.01, 0, 0, 2, 0, 0], [0, 0.02, 0, 0, 3, 0], [0, 0, -0.01, 0, 0, 1]], 0.05, 0.1, ("corner", 3))
case("t_end_on_interior", [[0, 0, 0, 4, 0, 0], [2, 0.01, 0, 2, 3, 0]], 0.05, 0.1, ("t", 2))
_x = [[0, 0, 0, 4, 0, 0], [2, -1, 0.01, 2, 1, 0.01]]
case("x_without_crossings", _x, 0.05, 0.1, ("x", 0))
case("x_with_crossings", _x, 0.05, 0.1, ("x", 1), crossings=1)

# ---- the parameter at its thresholds.  The probe (0,0,0)-(4,0,0) has L = 4; the other line starts at (x0, 0, 0) and runs along y, so the probe's
# parameter is x0 exactly and the other's is 0 (END_P).  probe_first: the probe is line i and the parameter is s; otherwise it is line j and t
PROBE = [0, 0, 0, 4, 0, 0]


def at(x0):
    return [x0, 0, 0, x0, 3, 0]


def threshold(name, x0, ext, n_records, where):
    for first in (True, False):
        lines = [PROBE, at(x0)] if first else [at(x0), PROBE]
        case("%s_%s" % ("s" if first else "t", name), lines, 0.05, [ext, 0.5] if first else [0.5, ext],
             ("param", "s" if first else "t", x0, n_records, where))


threshold("at_minus_ext_passes", -0.5, 0.5, 1, jm.END_P)
threshold("below_minus_ext_fails", dn(-0.5), 0.5, 0, None)
threshold("at_ext_is_an_end", 0.5, 0.5, 1, jm.END_P)
threshold("above_ext_is_interior", up(0.5), 0.5, 1, jm.INTERIOR)
threshold("at_half_L_is_on_the_P_side", 2.0, 0.5, 1, jm.INTERIOR)
threshold("above_half_L_is_on_the_Q_side", up(2.0), 0.5, 1, jm.INTERIOR)
threshold("at_L_minus_ext_is_an_end", 3.5, 0.5, 1, jm.END_Q)
threshold("below_L_minus_ext_is_interior", dn(3.5), 0.5, 1, jm.INTERIOR)
threshold("at_L_plus_ext_passes", 4.5, 0.5, 1, jm.END_Q)
threshold("above_L_plus_ext_fails", up(4.5), 0.5, 0, None)
# L <= 2 ext: no interior is left, and L / 2 decides between the ends
threshold("L_below_2_ext_at_half_L_is_END_P", 2.0, 2.5, 1, jm.END_P)
threshold("L_below_2_ext_above_half_L_is_END_Q", up(2.0), 2.5, 1, jm.END_Q)

# ---- the gap at the tolerance: the second line passes h above the probe, so g = sqrt(h h) = h
above = lambda h: [2, 0, h, 2, 3, h]
case("g_equals_tol_passes", [PROBE, above(0.5)], [0.5, 0.5], 0.1, ("gap", 0.5, 1))
case("g_one_ulp_above_tol_fails", [PROBE, above(up(0.5))], [0.5, 0.5], 0.1, ("gap", up(0.5), 0))
case("the_larger_tolerance_decides_i", [PROBE, above(0.5)], [0.5, 0.0], 0.1, ("gap", 0.5, 1))
case("the_larger_tolerance_decides_j", [PROBE, above(0.5)], [0.0, 0.5], 0.1, ("gap", 0.5, 1))
case("both_tolerances_below_g_fails", [PROBE, above(0.5)], [0.25, 0.25], 0.1, ("gap", 0.5, 0))

# ---- the angle: d_j = (4 / 5, 3 / 5, 0), so b = 4 / 5 as rounded
C45 = float(F(4) / F(5))
_b = [[0, 0, 0, 10, 0, 0], [0, 0, 0, 4, 3, 0]]
case("b_equals_cos_max_passes", _b, 0.05, 0.1, ("angle", C45, 1), cos_max=C45)
case("b_one_ulp_above_cos_max_fails", _b, 0.05, 0.1, ("angle", C45, 0), cos_max=dn(C45))
case("negative_b_counts_by_its_size", [[0, 0, 0, 10, 0, 0], [4, 3, 0, 0, 0, 0]], 0.05, 0.5, ("angle", -C45, 1), cos_max=C45)
case("parallel_lines_are_never_a_pair", [[0, 0, 0, 4, 0, 0], [4, 0, 0, 8, 0, 0], [0, 0.01, 0, 4, 0.01, 0]], 1.0, 1.0, ("none",), cos_max=dn(1.0))

# ---- the star rule: five lines whose P ends lie 0.08 apart in a row along x, directions turning by 20 degrees in the y-z plane: the closest points of
# lines i and j are their P ends, 0.08 |i - j| apart.  tol 0.1: a chain 0 - 1 - 2 - 3 - 4 that spans 0.32
_row = lambda lengths: [[0.08 * k, 0, 0, 0.08 * k, L * math.cos(math.radians(20 * k)), L * math.sin(math.radians(20 * k))] for k, L in enumerate(lengths)]
case("row_of_five_representative_at_one_end", _row([3, 1, 1, 1, 1]), 0.1, 0.05, ("row", 0, [0, 2], [4, 6, 8]))
case("row_of_five_representative_in_the_middle", _row([1, 1, 3, 1, 1]), 0.1, 0.05, ("row", 4, [2, 4, 6], [0, 8]))
case("row_of_five_representative_has_the_highest_index", _row([1, 1, 1, 1, 3]), 0.1, 0.05, ("row", 8, [6, 8], [0, 2, 4]))
# equal L: the lowest node is the representative
case("equal_L_the_lowest_node_is_the_representative", [[0, 0, 0, 3, 0, 0], [0, 0, 0, 0, 3, 0], [9, 9, 9, 9, 9, 19]], 0.05, 0.1, ("rep", {0: 0, 2: 0}))
case("equal_L_the_lowest_node_is_a_Q_end", [[3, 0, 0, 0, 0, 0], [0, 0, 0, 0, 3, 0], [0, 0, 0, 0, 0, 3]], 0.05, 0.1, ("rep", {1: 1, 2: 1, 4: 1}))

# ---- attachments
_a2 = [[0, 0, 0, 4, 0, 0], [2, 0, -2, 2, 0, 2]]
case("attach_equal_gaps_the_lower_record_wins", _a2 + [[2, 0.01, 0, 2, 3, 0]], 0.05, 0.1, ("attach", 4, 0, 2))
case("attach_the_smaller_gap_wins", _a2 + [[2, 0.01, 0.001, 2, 3, 0.001]], 0.05, 0.1, ("attach", 4, 1, 2))
# the corner of lines 0 and 1 lies on the inside of line 2: two T records whose end nodes are in a vertex
case("an_end_in_a_vertex_is_not_attached", [[0, 0, 0, 2, 0, 0], [0, 0, 0, 0, 3, 0], [0, 0, -2, 0, 0, 2]], 0.05, 0.1, ("vertex_not_attached", 2))

_t = corners(300, 7)
_t[100, 3:] = _t[100, :3]                                 # L = 0
_t[101, 4] = np.nan
_t[102, 0] = np.inf
_tol = np.full(300, 0.05)
_ext = np.full(300, 0.1)
_tol[103] = np.inf
_ext[104] = np.inf
case("ineligible_lines_in_the_middle_of_a_tile", _t, _tol, _ext, ("ineligible", [100, 101, 102, 103, 104]))

# 300 lines that start at one point: every pair is an L record at (P, P), one vertex of degree 300 -- rows of up to 299 records for the scan
case("300_lines_from_one_point", fan(300, 20, 0.05), 0.05, 0.1, ("dense", 300, 44850), cos_max=math.cos(math.radians(1.0)))
# the same lines prolonged backwards through the point: every pair is an X record
_f = fan(300, 20, 0.05)
_f[:, :3] -= (_f[:, 3:] - _f[:, :3])
case("300_lines_through_one_point_crossing", _f, 0.05, 0.1, ("dense_x", 300, 44850), cos_max=math.cos(math.radians(1.0)), crossings=1)
case("lines_1e6_units_from_the_origin", corners(64, 9, offset=1e6), 0.05, 0.1, ("far", 1e6))

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def model_of(case):
    if "model" not in case:
        case["model"] = jm.junctions(case["lines"], case["tol"], case["ext"], case["cos_max"], case["crossings"])
    return case["model"]


KEYS = (("records", jm.RECORD), ("node_vertex", np.int32), ("vertices", jm.VERTEX), ("node_attach", np.int32), ("counts", np.int32))


def same(got, exp):
    """bit for bit: records, node_vertex, vertices, node_attach, counts"""
    return all(np.asarray(got[k]).dtype == dt and np.asarray(got[k]).shape == np.asarray(exp[k]).shape
               and np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes() for k, dt in KEYS)


def difference(got, exp):
    """which outputs differ (for a failing assertion's message)"""
    return [k for k, dt in KEYS if not (np.asarray(got[k]).dtype == dt and np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes())]


# (name, overrides of a good call, code, a word of the cause)
GOOD = dict(lines=np.array([[0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0]], F), tol=np.array([0.1, 0.1], F), ext=np.array([0.1, 0.1], F), cos_max=0.9, crossings=0)
REFUSALS = [
    ("negative_count", dict(lines=-1, tol=None, ext=None), 1, "negative count"),
    ("null_lines", dict(lines=2), 1, "null array"),
    ("null_tol", dict(tol=None), 1, "null array"),
    ("null_ext", dict(ext=None), 1, "null array"),
    ("cos_max_one", dict(cos_max=1.0), 1, "cos_max"),
    ("cos_max_above_one", dict(cos_max=1.5), 1, "cos_max"),
    ("cos_max_negative", dict(cos_max=-0.1), 1, "cos_max"),
    ("cos_max_nan", dict(cos_max=float("nan")), 1, "cos_max"),
    ("tol_negative", dict(tol=np.array([0.1, -0.1], F)), 1, "tol[1]"),
    ("tol_nan", dict(tol=np.array([float("nan"), 0.1], F)), 1, "tol[0]"),
    ("ext_negative", dict(ext=np.array([-0.1, 0.1], F)), 1, "ext[0]"),
    ("ext_nan", dict(ext=np.array([0.1, float("nan")], F)), 1, "ext[1]"),
    ("more_than_2_30_lines", dict(lines=(1 << 30) + 1, tol=None, ext=None), 5, "2^30"),
]


def refusal_arguments(overrides):
    kw = dict(GOOD)
    kw.update(overrides)
    return kw
