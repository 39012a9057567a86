"""Crafted tables for the grouping of duplicate 3-D lines (include/line3d_amd.h, "MERGING DUPLICATE LINES"), each named for the case it is;
tests/test_merge_cases_cpu.py checks with the model that every table is what its name claims.  The decision points are built from exactly
representable numbers: axis-aligned lines and 3-4-5 directions."""
import math

import numpy as np

import merge_model as mm

F = np.float64
COS5 = math.cos(5.0 * math.pi / 180.0)
up = lambda x: float(np.nextafter(F(x), F(np.inf)))

CASES = []


def case(name, lines, tol, claim, cos_min=COS5, max_gap=0.0):
    lines = np.asarray(lines, F).reshape(-1, 6)
    tol = np.full(len(lines), tol, F) if np.isscalar(tol) else np.asarray(tol, F)
    assert len(tol) == len(lines)
    CASES.append(dict(name=name, lines=lines, tol=tol, cos_min=float(cos_min), max_gap=float(max_gap), claim=claim))


def copies(n, seed, jitter=0.01, offset=0.0):
    """n lines: near-copies (end points moved by up to `jitter`) of n // 4 random base lines of length 1 to 3; line k copies base k mod (n // 4), so
    the copies of one base lie n // 4 apart: in different waves and, from n = 513 on, two tiles apart"""
    rng = np.random.default_rng(seed)
    m = max(1, n // 4)
    P = rng.uniform(-5, 5, (m, 3)) + offset
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    Q = P + d * rng.uniform(1, 3, (m, 1))
    base = np.hstack([P, Q])
    out = base[np.arange(n) % m] + rng.uniform(-jitter, jitter, (n, 6))
    flip = rng.random(n) < 0.3                           # some copies run the other way
    out[flip] = out[flip][:, [3, 4, 5, 0, 1, 2]]
    return out


SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)
for n in SIZES:
    case("size_%d" % n, copies(n, 100 + n), 0.05, ("size", n))

# rows of more than 64 and more than 128 pairs
case("bundle_of_130_identical_lines", np.tile([[0.1, 0.2, 0.3, 1.3, 2.2, 0.8]], (130, 1)), 0.01, ("one_group", 130, 130 * 129 // 2))
# 300 lines along x, 1e-4 apart in y, each a little longer than the one before: all match, and the last is the representative
case("300_mutually_matching_lines", [[0, k * 1e-4, 0, 10 + k * 1e-3, k * 1e-4, 0] for k in range(300)], 0.1, ("one_group", 300, 44850))

A4 = [0, 0, 0, 4, 0, 0]
case("e_equals_tol_passes", [A4, [1, 0.5, 0, 3, 0.5, 0]], [0.5, 0.5], ("terms", 1, dict(e=0.5)))
case("e_one_ulp_above_tol_fails", [A4, [1, up(0.5), 0, 3, 0.5, 0]], [0.5, 0.5], ("terms", 0, dict(e=up(0.5))))
case("the_larger_tolerance_decides_a", [A4, [1, 0.5, 0, 3, 0.5, 0]], [0.5, 0.0], ("terms", 1, dict(e=0.5)))
case("the_larger_tolerance_decides_b", [A4, [1, 0.5, 0, 3, 0.5, 0]], [0.0, 0.5], ("terms", 1, dict(e=0.5)))
case("both_tolerances_below_e_fails", [A4, [1, 0.5, 0, 3, 0.5, 0]], [0.25, 0.25], ("terms", 0, dict(e=0.5)))
A10 = [0, 0, 0, 10, 0, 0]
B345 = [0, 0, 0, 4, 3, 0]                                 # L = 5, d = (4 / 5, 3 / 5, 0)
case("dot_equals_cos_min_passes", [A10, B345], 10.0, ("terms", 1, dict(c=float(F(4) / F(5)))), cos_min=float(F(4) / F(5)))
case("dot_one_ulp_below_cos_min_fails", [A10, B345], 10.0, ("terms", 0, dict(c=float(F(4) / F(5)))), cos_min=up(F(4) / F(5)))
case("antiparallel_passes", [A4, [3, 0, 0, 1, 0, 0]], 0.0, ("terms", 1, dict(c=1.0, e=0.0)))
case("touching_end_to_end_passes", [A4, [4, 0, 0, 6, 0, 0]], 0.0, ("terms", 1, dict(ov=0.0)))
case("gap_of_one_ulp_fails", [A4, [up(4), 0, 0, 6, 0, 0]], 0.0, ("terms", 0, dict(ov=4.0 - up(4))))
case("gap_on_max_gap_times_Lb_passes", [A4, [5, 0, 0, 7, 0, 0]], 0.0, ("terms", 1, dict(ov=-1.0)), max_gap=0.5)
case("gap_inside_max_gap_times_Lb_passes", [A4, [4.5, 0, 0, 6.5, 0, 0]], 0.0, ("terms", 1, dict(ov=-0.5)), max_gap=0.5)
case("gap_outside_max_gap_times_Lb_fails", [A4, [up(5), 0, 0, 7, 0, 0]], 0.0, ("terms", 0, dict(ov=4.0 - up(5))), max_gap=0.5)
# equal L = 5: from line 0's axis the ends of line 1 lie 0 and 3 away, from line 1's axis the ends of line 0 lie 0.6 and 2.4 away; tol 2.5
case("equal_L_the_lower_index_is_a", [[0, 0, 0, 5, 0, 0], [1, 0, 0, 5, 3, 0]], 2.5, ("equal_L", 0), cos_min=0.5)
case("equal_L_the_lower_index_is_the_representative", [[0, 0, 0, 5, 0, 0], [9, 9, 9, 9, 9, 10], [0, 0, 0, 5, 0, 0], [0, 0, 0, 5, 0, 0]], 0.0, ("rep", [0, 1, 0, 0]))
ang = lambda deg, L: [0, 0, 0, L * math.cos(math.radians(deg)), L * math.sin(math.radians(deg)), 0]
# A ~ B (4 degrees), B ~ C (4 degrees), A unlike C (8 degrees): one component, C released
case("chain_whose_end_fails_against_the_representative", [ang(0, 10), ang(4, 5), ang(8, 4)], 10.0, ("release", [0, 0, 2], [1, 1, 1, 1]))
# the same chain with the representative in the middle of the index order, and the released line the lowest index
case("chain_released_line_has_the_lowest_index", [ang(8, 4), ang(4, 5), ang(0, 10)], 10.0, ("release", [0, 1, 1], [1, 1, 1, 1]))
case("representative_is_not_the_lowest_index", [[1, 0, 0, 2, 0, 0], [0, 0, 0, 4, 0, 0], [7, 7, 7, 8, 8, 8]], 0.0, ("rep", [1, 1, 2]))
_t = copies(300, 7)
_t[100] = [1, 2, 3, 1, 2, 3]                              # L = 0
_t[101, 4] = np.nan
_t[102, 0] = np.inf
case("ineligible_lines_in_the_middle_of_a_tile", _t, 0.05, ("ineligible", [100, 101, 102]))
case("tol_zero_coincident_lines", [[0, 0, 0, 2, 0, 0], [0, 0, 0, 2, 0, 0]], 0.0, ("terms", 1, dict(e=0.0)))
case("lines_1e6_units_from_the_origin", copies(64, 9, jitter=1e-3, offset=1e6), 0.05, ("far", 1e6))

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def model_of(case):
    if "model" not in case:
        case["model"] = mm.group_lines(case["lines"], case["tol"], case["cos_min"], case["max_gap"])
    return case["model"]


def same(got, exp):
    """bit for bit: group, pairs, counts"""
    return all(np.asarray(got[k]).dtype == np.int32 and np.asarray(got[k]).shape == np.asarray(exp[k]).shape
               and np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes() for k in ("group", "pairs", "counts"))


# (name, overrides of a good call, code, a word of the cause)
GOOD = dict(lines=np.array([[0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0]], F), tol=np.array([0.1, 0.1], F), cos_min=0.9, max_gap=0.0)
REFUSALS = [
    ("negative_count", dict(lines=-1, tol=None), 1, "negative count"),
    ("null_lines", dict(lines=2), 1, "null array"),
    ("cos_min_above_one", dict(cos_min=1.5), 1, "cos_min"),
    ("cos_min_negative", dict(cos_min=-0.1), 1, "cos_min"),
    ("cos_min_nan", dict(cos_min=float("nan")), 1, "cos_min"),
    ("max_gap_negative", dict(max_gap=-1.0), 1, "max_gap"),
    ("max_gap_infinite", dict(max_gap=float("inf")), 1, "max_gap"),
    ("max_gap_nan", dict(max_gap=float("nan")), 1, "max_gap"),
    ("tol_negative", dict(tol=np.array([0.1, -0.1], F)), 1, "tol[1]"),
    ("tol_nan", dict(tol=np.array([float("nan"), 0.1], F)), 1, "tol[0]"),
]


def refusal_arguments(overrides):
    kw = dict(GOOD)
    kw.update(overrides)
    return kw
