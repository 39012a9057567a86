"""The seeded case table of the line fit (l3d_fit_clusters / l3d_fit_labelled_clusters), shared by tests/test_linefit_cases_cpu.py (the
conditions on the inputs, the model against the oracle's align(), what the table contains) and tests/test_gpu_linefit_shapes.py.

A case is one l3d_fit_clusters call: a dict of
    name, seed, hyp (HYP_DTYPE, numbered camera by camera), hyp_cam (uint32, ascending), group_start, member_hyp, Rinv, scale_inv, tneg
and, for the twins of the overflow cases, twin_of (the name of the case this one is with its last member taken away).

How a cluster is laid out: its members' end points sit on distinct SLOTS of a grid along a line (cell 1/64, a point somewhere in the first
half of its cell, noise of 2 % of a cell on every coordinate), so two different points are never closer than a third of a cell along the
line -- thousands of float32 ulps of the longest cluster -- and the float32 order of the distances does not depend on whose eigenvectors
found the direction (condition (a) of the CPU test, which measures it for every cluster).  Members come in CHUNKS: 2w consecutive
slots, the first w open a member each, the last w close them in a shuffled order; between two chunks nothing is open, so a chunk
with three cameras gives one 3-D segment.

k_fit_clusters takes one of four paths per cluster (model: linefit_model.path_of): 'lo' (<= 64 members), 'hi' (65-128 members: both
halves of the open mask), 'overflow' (<= 128 members, a 65th distinct camera), 'global' (> 128 members)."""
import numpy as np

from line3d_amd.capi import HYP_DTYPE

import linefit_model as lm

CELL = 1.0 / 64
IDENT = (np.eye(3), 1.0, np.zeros(3))
_TH = 0.4
ROTATED = (np.array([[np.cos(_TH), -np.sin(_TH), 0.0], [np.sin(_TH), np.cos(_TH), 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]]),
           2.5, np.array([0.3, -1.2, 0.7]))                          # (those of test_fit_clusters_against_the_oracle_line_fit)


# ---- clusters: lists of (camera, P1, P2)

def _chunk_slots(rng, sizes, gap=2):
    """-> per member (start slot, end slot): chunks of w members on 2w of the next 4w slots"""
    out, cursor = [], 0
    for w in sizes:
        s = np.sort(rng.choice(4 * w, 2 * w, replace=False)) + cursor
        ends = rng.permutation(s[w:])
        out += [(int(s[i]), int(ends[i])) for i in range(w)]
        cursor += 4 * w + gap
    return out


def _sizes(rng, m, lo=2, hi=9):
    out = []
    while m > 0:
        w = min(m, int(rng.integers(lo, hi)))
        out.append(w)
        m -= w
    return out


def _spread(rng, m, cams):
    """m camera ids, every one of `cams` at least once (m >= len(cams)), in random order"""
    cams = list(cams)
    assert m >= len(cams)
    a = cams + [cams[int(k)] for k in rng.integers(0, len(cams), m - len(cams))]
    return [a[int(k)] for k in rng.permutation(m)]


def _place(rng, slots, cams, swap=0.3, noise=0.02, offset=0.0, scale=1.0, line=None):
    """the members on a random line; swap: the share of members with P2 before P1 along the line"""
    p0, d = (rng.uniform(-3, 3, 3), rng.normal(size=3)) if line is None else line
    d = d / np.linalg.norm(d)
    if d[int(np.argmax(np.abs(d)))] > 0:                       # (the fit's direction has its largest component positive and the sweep starts at
        d = -d                                                 # the far end ALONG it, line3D.cc:1527-1541: this way it runs in slot order)
    n_slots = max(max(s) for s in slots) + 1
    out = []
    for (a, b), cam in zip(slots, cams):
        P = []
        for s in (a, b):
            t = (s + 0.5 * rng.random() - 0.5 * n_slots) * CELL
            P.append(((p0 + t * d + rng.normal(scale=noise * CELL, size=3)) + offset) * scale)
        if rng.random() < swap:
            P.reverse()
        out.append((int(cam), P[0], P[1]))
    return out


def random_cluster(rng, m, n_cams, cam_base=0, **kw):
    return _place(rng, _chunk_slots(rng, _sizes(rng, m)), _spread(rng, m, range(cam_base, cam_base + n_cams)), **kw)


def triples_cluster(rng, m):
    """chunks of three members of three cameras: one segment per chunk"""
    assert m % 3 == 0
    cams = [3 * ((i // 3) % 2) + i % 3 for i in range(m)]
    return _place(rng, _chunk_slots(rng, [3] * (m // 3)), cams)


def oscillating_cluster(rng, n_short):
    """two members of two cameras span everything, short members of two more cameras follow one another: 2, 3, 2, 3, ... cameras open"""
    n = 2 * n_short + 4
    slots = [(0, n - 1), (1, n - 2)] + [(2 + 2 * k, 3 + 2 * k) for k in range(n_short)]
    return _place(rng, slots, [10, 11] + [12 + k % 2 for k in range(n_short)], swap=0.0)


def multi_open_cluster(rng, n_chunks):
    """chunks of six members, three of them of one camera and two of another: a camera's count of open members goes to 3 and back"""
    return _place(rng, _chunk_slots(rng, [6] * n_chunks), [20, 20, 20, 21, 21, 22] * n_chunks)


def overflow_cluster(rng, where):
    """64 cameras in chunks that emit a segment each, then the member of the 65th camera (the largest id: the LAST member in key order).
    where = 'after': it opens first in a closing chunk of three cameras (that chunk's segment exists only with it);
    where = 'last': it lies alone behind everything -- its two points are the last two of the sweep, the 65th camera is met at the last
    step at which a camera can be met at all (a member's second point never brings a new camera)."""
    sizes = [3] * 20 + [4]
    slots = _chunk_slots(rng, sizes)
    cams = list(range(100, 164))
    end = max(max(s) for s in slots) + 3
    if where == "after":
        slots += [(end, end + 5), (end + 1, end + 4), (end + 2, end + 3)]
        cams += [999, 100, 101]
    else:
        slots += [(end, end + 1)]
        cams += [999]
    return _place(rng, slots, cams, swap=0.0)


def sequential_cluster(rng, m, cams):
    """members one after the other, never two open"""
    return _place(rng, [(2 * k, 2 * k + 1) for k in range(m)], [cams[k % len(cams)] for k in range(m)])


def exact_cluster(slots, cams, p0, step):
    """noiseless, every coordinate a small dyadic fraction: point = p0 + slot * step"""
    p0, step = np.asarray(p0, np.float64), np.asarray(step, np.float64)
    return [(int(c), p0 + a * step, p0 + b * step) for (a, b), c in zip(slots, cams)]


def identical_pairs_cluster():
    """pairs of bit-identical members in different cameras: every tie of the sort is between such twins"""
    slots, cams = [], []
    for j in range(4):
        b = 20 * j
        slots += [(b, b + 8), (b, b + 8), (b + 2, b + 6), (b + 2, b + 6), (b + 11, b + 15)]
        cams += [1, 2, 3, 4, 5]
    return exact_cluster(slots, cams, (1.0, 2.0, 3.0), (0.5, 0.125, -0.25))


# ---- cases

def make_case(name, seed, clusters, transform=IDENT, twin_of=None):
    """clusters: lists of (camera, P1, P2).  The hypotheses are numbered by (camera, order of appearance), members ascend per group."""
    flat = [(cam, P1, P2, g) for g, cl in enumerate(clusters) for (cam, P1, P2) in cl]
    order = sorted(range(len(flat)), key=lambda k: (flat[k][0], k))
    hyp = np.zeros(len(flat), HYP_DTYPE)
    hyp_cam = np.zeros(len(flat), np.uint32)
    groups = [[] for _ in clusters]
    for new, old in enumerate(order):
        cam, P1, P2, g = flat[old]
        hyp[new]["P1"], hyp[new]["P2"], hyp_cam[new] = P1, P2, cam
        groups[g].append(new)
    group_start, member_hyp = [0], []
    for members in groups:
        member_hyp += members
        group_start.append(len(member_hyp))
    Rinv, scale_inv, tneg = transform
    return {"name": name, "seed": seed, "hyp": hyp, "hyp_cam": hyp_cam, "group_start": np.array(group_start, np.int32),
            "member_hyp": np.array(member_hyp, np.int32), "Rinv": np.array(Rinv, np.float64), "scale_inv": float(scale_inv),
            "tneg": np.array(tneg, np.float64), "twin_of": twin_of, "identity": transform is IDENT}


MEMBER_LADDER = [(4, 1001), (31, 1002), (32, 1003), (33, 1004), (63, 1005), (64, 1006), (65, 1007), (96, 1008), (127, 1009), (128, 1010),
                 (129, 1011), (130, 1012), (255, 1013), (256, 1014), (257, 1015), (600, 1016)]                       # (members, seed)
CAMERA_LADDER = [(64, 63, 1101), (64, 64, 1102), (64, 64, 1103),                                                     # (members, cameras, seed)
                 (65, 64, 1104), (65, 65, 1105), (65, 65, 1106), (100, 64, 1107), (100, 65, 1108), (100, 100, 1109),
                 (128, 64, 1110), (128, 65, 1111), (128, 128, 1112), (129, 65, 1113), (129, 200, 1114), (300, 65, 1115), (300, 200, 1116)]
GROUP_COUNTS = [(1, 1401), (2, 1402), (3, 1403), (4, 1404), (5, 1405), (9, 1406)]                                    # (n_groups, seed)


def build_cases():
    cases = []

    def add(name, seed, make, **kw):
        cases.append(make_case(name, seed, make(np.random.default_rng(seed)), **kw))

    for m, seed in MEMBER_LADDER:
        add("members_%d" % m, seed, lambda r, m=m: [random_cluster(r, m, min(m, 5 + m % 5))])         # (5-9 cameras; 4 members have 4)
    for m, c, seed in CAMERA_LADDER:
        if c > m:
            # more cameras than members cannot be: 129 and 300 members "with 200 cameras" have as many distinct cameras as fit, min(m, 200)
            c = m
        add("cameras_%dm_%dc_s%d" % (m, c, seed), seed, lambda r, m=m, c=c: [random_cluster(r, m, c)])
    # where the overflow happens, and the same clusters without the member of the 65th camera
    for where, seed in (("after", 1201), ("last", 1202)):
        cl = overflow_cluster(np.random.default_rng(seed), where)
        cases.append(make_case("overflow_%s" % where, seed, [cl]))
        cases.append(make_case("overflow_%s_twin" % where, seed, [[m for m in cl if m[0] != 999]], twin_of="overflow_%s" % where))
    # sweep shapes
    add("triples_126", 1301, lambda r: [triples_cluster(r, 126)])
    add("triples_129", 1302, lambda r: [triples_cluster(r, 129)])
    add("oscillating_2_3", 1303, lambda r: [oscillating_cluster(r, 30)])
    add("camera_count_above_1", 1304, lambda r: [multi_open_cluster(r, 5)])
    add("p2_before_p1", 1305, lambda r: [random_cluster(r, 20, 6, swap=1.0)])
    add("camera_ids_0_and_ffffffff", 1306, lambda r: [_place(r, _chunk_slots(r, _sizes(r, 12)), _spread(r, 12, [0, 0xFFFFFFFF, 5, 7, 0xFFFFFFFE]))])
    # exact ties and degenerate geometry
    add("all_points_identical", 1311, lambda r: [exact_cluster([(0, 0)] * 6, [1, 1, 2, 2, 3, 3], (1.5, -2.25, 3.0), (0.0, 0.0, 0.0))])
    add("identical_member_pairs", 1312, lambda r: [identical_pairs_cluster()])
    # one member ends on the very point at which another starts: the stable order (point index) decides whether the line breaks there
    add("end_and_start_tied", 1314, lambda r: [exact_cluster([(0, 20), (1, 19), a, b], [1, 2, 3, 4], (1.0, 2.0, 3.0), (0.5, 0.125, -0.25))
                                                for a, b in (((2, 8), (8, 14)), ((8, 14), (2, 8)))])
    add("axis_aligned_noiseless", 1313, lambda r: [exact_cluster(_chunk_slots(r, _sizes(r, 24)), _spread(r, 24, range(5)), (0.0, 1.0, 2.0), (0.25, 0.0, 0.0))])
    # scale and transform
    add("offset_1e6", 1321, lambda r: [random_cluster(r, 40, 7, offset=1e6), random_cluster(r, 140, 9, offset=1e6)])
    add("scaled_1e-6", 1322, lambda r: [random_cluster(r, 40, 7, scale=1e-6), random_cluster(r, 140, 9, scale=1e-6)])
    add("transformed", 1323, lambda r: [random_cluster(r, 4, 4), random_cluster(r, 70, 8), random_cluster(r, 129, 9), random_cluster(r, 70, 70),
                                        random_cluster(r, 19, 6)], transform=ROTATED)
    # layout
    for n, seed in GROUP_COUNTS:
        add("groups_%d" % n, seed, lambda r, n=n: [random_cluster(r, int(r.integers(5, 21)), int(r.integers(4, 6)), cam_base=7 * g) for g in range(n)])
    add("mixed_workgroup", 1411, lambda r: [random_cluster(r, 4, 4), random_cluster(r, 128, 9), random_cluster(r, 129, 9), random_cluster(r, 70, 70)])
    add("empty_groups", 1412, lambda r: [[], random_cluster(r, 8, 5), [], random_cluster(r, 9, 5), []])
    add("two_cameras", 1413, lambda r: [random_cluster(r, 10, 2)])
    add("three_cameras_never_overlapping", 1414, lambda r: [sequential_cluster(r, 12, [1, 2, 3])])
    return cases


CASES = build_cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def case_clusters(case):
    """-> per group (pts (2 * members, 3) float64: the inverse-transformed end points in member order, cams (members,))"""
    out = []
    gs, mh = case["group_start"], case["member_hyp"]
    for g in range(len(gs) - 1):
        k = mh[gs[g]:gs[g + 1]]
        P = np.stack([case["hyp"]["P1"][k], case["hyp"]["P2"][k]], axis=1).reshape(-1, 3)
        pts = P.copy() if case["identity"] else lm.inverse_transform(P, case["Rinv"], case["scale_inv"], case["tneg"])
        out.append((pts, case["hyp_cam"][k].astype(np.int64)))
    return out


_MODEL = {}


def model_of(case):
    """-> per group the model's fit (linefit_model.fit_cluster), computed once per case"""
    if case["name"] not in _MODEL:
        _MODEL[case["name"]] = [lm.fit_cluster(pts, cams) for pts, cams in case_clusters(case)]
    return _MODEL[case["name"]]


def merged(cases):
    """several cases with one transform as ONE case: their groups back to back, the hypotheses of all of them renumbered camera by camera
    (a group's members keep their order: they were in camera order already)"""
    clusters = []
    for c in cases:
        gs, mh = c["group_start"], c["member_hyp"]
        for g in range(len(gs) - 1):
            clusters.append([(int(c["hyp_cam"][k]), c["hyp"]["P1"][k].copy(), c["hyp"]["P2"][k].copy()) for k in mh[gs[g]:gs[g + 1]]])
    t = (cases[0]["Rinv"], cases[0]["scale_inv"], cases[0]["tneg"])
    m = make_case("merged", None, clusters, transform=IDENT if cases[0]["identity"] else t)
    m["identity"] = cases[0]["identity"]
    return m
