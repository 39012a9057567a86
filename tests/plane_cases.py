"""Crafted tables for the planes of 3-D lines (include/line3d_amd.h, "PLANES OF 3-D LINES"), each named for the case it is;
tests/test_plane_cases_cpu.py checks with the model that every table is what its name claims.  The decision points are built from exactly
representable numbers: a floor of axis-parallel lines in z = 0 whose hypotheses have N = (0, 0, +-1) and c = 0 exactly, lines lifted above it by a
tolerance or one ulp more, and a cube with integer corners."""
import functools
import math

import numpy as np

import plane_model as pm

F = np.float64
COS10 = math.cos(10.0 * math.pi / 180.0)
up = lambda x: float(np.nextafter(F(x), F(np.inf)))
dn = lambda x: float(np.nextafter(F(x), F(-np.inf)))

CASES = []


def case(name, lines, tol, seeds, claim, cos_max=COS10, cos_min=COS10, min_lines=3):
    lines = np.asarray(lines, F).reshape(-1, 6)
    tol = np.full(len(lines), tol, F) if np.isscalar(tol) else np.asarray(tol, F)
    seeds = np.asarray(seeds, np.int32).reshape(-1, 2)
    assert len(tol) == len(lines)
    CASES.append(dict(name=name, lines=lines, tol=tol, seeds=seeds, cos_max=float(cos_max), cos_min=float(cos_min), min_lines=int(min_lines), claim=claim))


def chunks(m):
    """the column chunks of the device's hypothesis search (plane::chunks, the rule of merge::chunks)"""
    tiles = (m + 255) // 256
    if tiles >= 512:
        return 1
    c = min((1024 + tiles - 1) // max(tiles, 1), tiles, 64)
    if m > 0:
        c = min(c, (1 << 30) // m)
    return max(c, 1)


# ---- boxes: 12 edges each, edge 4 a + 2 [s1 > 0] + [s2 > 0] runs along axis a at the signs (s1, s2) of the two other axes (in ascending axis order)
def edge_id(a, signs):
    o = [k for k in range(3) if k != a]
    return 4 * a + 2 * (signs[o[0]] > 0) + (signs[o[1]] > 0)


CORNERS = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
# the 24 corner pairs of a box as (edge, edge, face): the face is (the axis neither edge runs along, the corner's sign on it)
CORNER_PAIRS = []
for _c in CORNERS:
    for _a, _b in ((0, 1), (0, 2), (1, 2)):
        _n = 3 - _a - _b
        CORNER_PAIRS.append((edge_id(_a, _c), edge_id(_b, _c), 2 * _n + (_c[_n] > 0)))


def boxes(nb, seed, offset=0.0, exact=False):
    """(12 nb, 6) lines: the edges of nb boxes.  exact: one axis-parallel cube per box with corners at +-2 around the integer centre (8 b, 8 b, 8 b), so
    that no two faces share a plane; otherwise random frames and half sizes, every edge up to 0.05 short of its corners or 0.02 beyond them and up to
    0.003 beside them, every fourth reversed"""
    rng = np.random.default_rng(seed)
    out = np.zeros((12 * nb, 6))
    for b in range(nb):
        if exact:
            c, R, h = np.array([8.0 * b, 8.0 * b, 8.0 * b]) + offset, np.eye(3), np.array([2.0, 2.0, 2.0])
        else:
            c, R, h = rng.uniform(-5, 5, 3) + offset, np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.uniform(0.5, 1.5, 3)
        for a in range(3):
            o = [k for k in range(3) if k != a]
            for s1 in (-1, 1):
                for s2 in (-1, 1):
                    mid = c + R[:, o[0]] * (s1 * h[o[0]]) + R[:, o[1]] * (s2 * h[o[1]])
                    P, Q = mid - R[:, a] * h[a], mid + R[:, a] * h[a]
                    if not exact:
                        P = P + R[:, a] * rng.uniform(-0.02, 0.05) + rng.uniform(-0.003, 0.003, 3)
                        Q = Q - R[:, a] * rng.uniform(-0.02, 0.05) + rng.uniform(-0.003, 0.003, 3)
                    k = 12 * b + 4 * a + 2 * (s1 > 0) + (s2 > 0)
                    out[k] = np.hstack([Q, P]) if (not exact and k % 4 == 3) else np.hstack([P, Q])
    return out


def box_seeds(nb, n, m):
    """m seeds over the first n lines of nb boxes: the corner pairs whose two lines are in the table, ordered by (corner pair, box) -- the
    hypotheses of one face lie up to 23 nb apart, in different waves and tiles -- and repeated from the start when m is larger than their number"""
    pairs = [(12 * b + i, 12 * b + j) for i, j, _ in CORNER_PAIRS for b in range(nb) if 12 * b + i < n and 12 * b + j < n]
    return np.array([pairs[k % len(pairs)] for k in range(m)], np.int32)


SIZES = ((12, 1), (256, 255), (257, 256), (300, 257), (300, 513), (2052, 4096))
for _n, _m in SIZES:
    _nb = (_n + 11) // 12
    case("size_n%d_m%d" % (_n, _m), boxes(_nb, 300 + _m)[:_n], 0.03, box_seeds(_nb, _n, _m), ("size", _n, _m))
case("size_n1_m1", [[0, 0, 0, 1, 0, 0]], 0.03, [[0, 0]], ("none", 1, 0))

# ---- the floor: four axis-parallel lines in z = 0.  Seeds (0, 1) and (0, 2) have N = (0, 0, 1), seeds (1, 3) and (2, 3) have N = (0, 0, -1); c = 0
FLOOR = [[0, 0, 0, 2, 0, 0], [0, 0, 0, 0, 3, 0], [2, 0, 0, 2, 3, 0], [0, 3, 0, 2, 3, 0]]
FLOOR_SEEDS = [[0, 1], [0, 2], [1, 3], [2, 3]]
case("floor_normals_of_opposite_signs", FLOOR, 0.01, FLOOR_SEEDS, ("floor", 4))
case("duplicated_seed_is_two_hypotheses", FLOOR, 0.01, [[0, 1], [0, 1], [2, 3]], ("duplicate", 3))
# A of (1, 3) is (3 x 2) x 1 = 6 = A of (0, 1): the lower index is the representative
case("equal_weights_the_lower_index_represents", FLOOR, 0.01, [[1, 3], [0, 1]], ("equal", 0))
case("equal_weights_the_lower_index_represents_swapped", FLOOR, 0.01, [[0, 1], [1, 3]], ("equal", 0))
# ineligible seeds: line 4 has no length, line 5 holds a NaN, seed (1, 1) names one line twice
_inel = FLOOR + [[1, 1, 0, 1, 1, 0], [0, 0, float("nan"), 1, 0, 0]]
case("ineligible_seeds", _inel, 0.01, [[0, 4], [0, 1], [5, 1], [1, 1], [2, 3]], ("ineligible", [0, 2, 3], [4, 5]))
# |b| at cos_max: line 1 runs along (0.6, 0.8, 0), b = d_0 . d_1 = 0.6 as rounded; cos_max = b passes, one ulp less does not
_slant = [[0, 0, 0, 2, 0, 0], [0, 0, 0, 3, 4, 0], [2, 0, 0, 2, 3, 0]]
_b = float(pm.hypothesis_terms(pm.prepare(_slant[0], 0.01), pm.prepare(_slant[1], 0.01))["b"])
case("angle_at_cos_max", _slant, 0.01, [[0, 1], [0, 2]], ("cos_max", _b, 2), cos_max=_b)
case("angle_just_above_cos_max", _slant, 0.01, [[0, 1], [0, 2]], ("cos_max", _b, 1), cos_max=dn(_b))


# ---- the fan: line 0 is the x axis, line k runs from the origin at k x 6 degrees about it; seed (0, k) spans the plane through the axis at that
# angle.  Neighbouring hypotheses pass the pair test (6 degrees, the far end 0.105 off), the next but one does not (12 degrees): one component,
# the representative is the longest line's hypothesis, in the middle, and only its two neighbours stay
def fan_lines(count, step_deg=6.0, longest=3):
    out = [[0, 0, 0, 4, 0, 0]]
    for k in range(1, count + 1):
        a = math.radians(step_deg * k)
        ln = 1.04 if k == longest else 1.0
        out.append([0, 0, 0, 0, ln * math.cos(a), ln * math.sin(a)])
    return out


case("fan_the_star_rule_releases_the_outer_hypotheses", fan_lines(5), 0.11, [[0, k] for k in range(1, 6)], ("fan", 2, [1, 2, 3], [0, 4]))

# ---- a cube: every edge in two planes, no edge between the hypotheses of different faces
_cube_seeds = [(i, j) for i, j, _ in CORNER_PAIRS]
case("cube_every_edge_in_two_planes", boxes(1, 0, exact=True), 0.01, _cube_seeds, ("cube", 6))
case("cube_with_tolerance_zero", boxes(1, 0, exact=True), 0.0, _cube_seeds, ("cube", 6))
case("two_cubes_far_from_the_origin", boxes(2, 0, offset=1048576.0, exact=True), 0.01, [(12 * b + i, 12 * b + j) for b in range(2) for i, j, _ in CORNER_PAIRS],
     ("cube", 12))
case("boxes_translated_by_1e6", boxes(8, 77, offset=1e6), 0.03, box_seeds(8, 96, 192), ("far", 1e6))

# ---- min_lines with exactly 2 and 3 members
case("two_members_min_lines_2", FLOOR[:2], 0.01, [[0, 1]], ("members", 2, 1), min_lines=2)
case("two_members_min_lines_3", FLOOR[:2], 0.01, [[0, 1]], ("members", 2, 0), min_lines=3)
case("three_members_min_lines_3", FLOOR[:3], 0.01, [[0, 1]], ("members", 3, 1), min_lines=3)

# ---- a plane distance exactly tol and one ulp above it.  Membership: the single hypothesis (0, 1) gives N = (0, 0, 1), c = 0; line 2 lies at height z
_lift = lambda z: FLOOR[:2] + [[1, 1, z, 3, 1, z]]
case("member_at_exactly_tol", _lift(0.25), [0.01, 0.01, 0.25], [[0, 1]], ("member_distance", 2, 0.25, True), min_lines=2)
case("member_one_ulp_beyond_tol", _lift(up(0.25)), [0.01, 0.01, 0.25], [[0, 1]], ("member_distance", 2, up(0.25), False), min_lines=2)
# the pair test: a second hypothesis in the parallel plane at height z; every line has tol 0.25
_two = lambda z: FLOOR[:2] + [[0, 0, z, 2, 0, z], [0, 0, z, 0, 3, z]]
case("pair_at_exactly_tol", _two(0.25), 0.25, [[0, 1], [2, 3]], ("pair_distance", 0.25, 1), min_lines=2)
case("pair_one_ulp_beyond_tol", _two(up(0.25)), 0.25, [[0, 1], [2, 3]], ("pair_distance", up(0.25), 0), min_lines=2)
# |N_h . N_g| exactly cos_min and one ulp below it: the fan's first two hypotheses, 6 degrees apart
_f2 = fan_lines(2)
_t = [pm.prepare(l, 0.2) for l in _f2]
_nd = float(abs(pm.dot(pm.hypothesis(_t, 0, 1, COS10)["N"], pm.hypothesis(_t, 0, 2, COS10)["N"])))
case("normals_at_exactly_cos_min", _f2, 0.2, [[0, 1], [0, 2]], ("cos_min", _nd, 1), cos_min=_nd, min_lines=2)
case("normals_one_ulp_below_cos_min", _f2, 0.2, [[0, 1], [0, 2]], ("cos_min", _nd, 0), cos_min=up(_nd), min_lines=2)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def model_of_name(name):
    c = BY_NAME[name]
    return pm.planes(c["lines"], c["tol"], c["seeds"], c["cos_max"], c["cos_min"], c["min_lines"])


def model_of(case_):
    """the model's result on a case, computed once and shared (read-only)"""
    return model_of_name(case_["name"])


KEYS = ("planes", "members", "hyp_plane", "counts")


def same(got, exp):
    return all(np.asarray(got[k]).dtype == np.asarray(exp[k]).dtype and np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes() for k in KEYS)


def difference(got, exp):
    out = []
    for k in KEYS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        if g.shape != e.shape:
            out.append("%s: shape %s, expected %s" % (k, g.shape, e.shape))
        elif g.tobytes() != e.tobytes():
            idx = [i for i in range(len(g)) if g[i].tobytes() != e[i].tobytes()][:3]
            out.append("%s differs at %s: %s, expected %s" % (k, idx, [g[i] for i in idx], [e[i] for i in idx]))
    return "; ".join(out)


# ---- the refusals: (name, overrides of GOOD, status, a word of the cause).  lines / seeds given as an int: a NULL array with that count
GOOD = dict(lines=np.asarray(FLOOR, F), tol=np.full(4, 0.01), seeds=np.asarray(FLOOR_SEEDS, np.int32), cos_max=COS10, cos_min=COS10, min_lines=3)
INVALID, UNSUPPORTED = 1, 5
REFUSALS = [
    ("negative_n", dict(lines=-1, tol=None, seeds=0), INVALID, "negative"),
    ("negative_m", dict(seeds=-1), INVALID, "negative"),
    ("null_lines", dict(lines=4), INVALID, "null array"),
    ("null_tol", dict(tol=None), INVALID, "null array"),
    ("null_seeds", dict(seeds=4), INVALID, "null array"),
    ("seed_beyond_the_table", dict(seeds=[[0, 1], [0, 4]]), INVALID, "outside"),
    ("seed_negative", dict(seeds=[[-1, 1]]), INVALID, "outside"),
    ("tol_negative", dict(tol=[0.01, -0.01, 0.01, 0.01]), INVALID, "tol[1]"),
    ("tol_nan", dict(tol=[0.01, 0.01, float("nan"), 0.01]), INVALID, "tol[2]"),
    ("cos_max_negative", dict(cos_max=-0.1), INVALID, "cos_max"),
    ("cos_max_one", dict(cos_max=1.0), INVALID, "cos_max"),
    ("cos_max_nan", dict(cos_max=float("nan")), INVALID, "cos_max"),
    ("cos_min_zero", dict(cos_min=0.0), INVALID, "cos_min"),
    ("cos_min_above_one", dict(cos_min=up(1.0)), INVALID, "cos_min"),
    ("cos_min_nan", dict(cos_min=float("nan")), INVALID, "cos_min"),
    ("min_lines_one", dict(min_lines=1), INVALID, "min_lines"),
    ("more_than_2_30_lines", dict(lines=2 ** 30 + 1, tol=None), UNSUPPORTED, "2^30"),
    ("more_than_2_30_seeds", dict(seeds=2 ** 30 + 1), UNSUPPORTED, "2^30"),
]


def refusal_arguments(overrides):
    kw = dict(GOOD)
    kw.update(overrides)
    return kw
