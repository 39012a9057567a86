"""The line fit's case table (tests/linefit_cases.py) and its float64 model (tests/linefit_model.py), checked without a GPU:

- every cluster of every case keeps the three conditions under which two correct fits must agree on the STRUCTURE (which input points are
  emitted): (a) neighbouring float64 distances that belong to different points differ by more than 4 float32 ulps of the largest distance,
  (b) the largest eigenvalue of the scatter is at least 100 times the second (waived where all points are identical: every distance is 0
  for any direction), (c) the two largest direction components differ by more than 1e-6 in magnitude;
- the model and the oracle's align() (an SVD of the uncentred product: another route to the direction) give the same structure wherever
  the coordinates are below 100 in magnitude;
- the table contains what it claims: how many clusters take each of k_fit_clusters' four paths, where the overflow happens, what the
  sweep shapes produce, how the twins of the overflow cases differ from them."""
from collections import Counter, OrderedDict

import numpy as np
import pytest

import l3d_oracle_pipeline as op
import linefit_cases as lc
import linefit_model as lm

NAMES = [c["name"] for c in lc.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_conditions_on_the_inputs(name):
    case = lc.CASE_BY_NAME[name]
    for g, ((pts, cams), fit) in enumerate(zip(lc.case_clusters(case), lc.model_of(case))):
        if len(pts) == 0:
            continue
        assert np.all(np.isfinite(pts)) and not np.any((pts == 0) & np.signbit(pts))     # (-0.0 would not survive the identity transform bit for bit)
        m = lm.linefit_conditions(pts, fit)
        assert m["gap_ulps"] > 4, (name, g, m)
        assert m["all_identical"] or m["eig_ratio"] >= 100, (name, g, m)
        assert m["all_identical"] or m["dir_gap"] > 1e-6, (name, g, m)


def _align_structure(pts, cams):
    rows = [p.copy() for p in pts]
    index = {id(p): i for i, p in enumerate(rows)}
    t3 = OrderedDict()
    for k in range(len(rows) // 2):
        t3[(int(cams[k]), k)] = (rows[2 * k], rows[2 * k + 1])
    return [(index[id(s)], index[id(e)]) for s, e in op.OracleLine3D(matching_neighbors=4).align(t3)]


@pytest.mark.parametrize("name", NAMES)
def test_model_gives_the_structure_of_the_oracles_align(name):
    case = lc.CASE_BY_NAME[name]
    checked = 0
    for (pts, cams), fit in zip(lc.case_clusters(case), lc.model_of(case)):
        if len(pts) and np.abs(pts).max() < 100:
            assert _align_structure(pts, cams) == fit["structure"], name
            checked += 1
    assert checked or name == "offset_1e6"


def _paths(case):
    return [lm.path_of(len(cams), cams) for _pts, cams in lc.case_clusters(case)]


def test_the_table_reaches_every_path():
    """clusters per path of k_fit_clusters, over the whole table (empty groups count as 'lo': no member, nothing indexed)"""
    n = Counter(p for c in lc.CASES for p in _paths(c))
    assert dict(n) == {"lo": 55, "hi": 11, "overflow": 10, "global": 15}, n
    # ... and cases (calls) in which a path is taken at all
    by_case = Counter(p for c in lc.CASES for p in set(_paths(c)))
    assert dict(by_case) == {"lo": 31, "hi": 11, "overflow": 10, "global": 15}, by_case
    # both sides of every boundary: 64 | 65 and 128 | 129 members, 64 | 65 cameras
    one = {c["name"]: (int(c["group_start"][1]), len(set(c["hyp_cam"].tolist())), _paths(c)[0]) for c in lc.CASES if len(c["group_start"]) == 2}
    assert one["members_64"][::2] == (64, "lo") and one["members_65"][::2] == (65, "hi")
    assert one["members_128"][::2] == (128, "hi") and one["members_129"][::2] == (129, "global")
    assert one["cameras_64m_64c_s1102"] == (64, 64, "lo") and one["cameras_64m_63c_s1101"] == (64, 63, "lo")
    for m in (65, 100, 128):
        assert one["cameras_%dm_64c_s%d" % (m, {65: 1104, 100: 1107, 128: 1110}[m])] == (m, 64, "hi")
        assert one["cameras_%dm_65c_s%d" % (m, {65: 1105, 100: 1108, 128: 1111}[m])] == (m, 65, "overflow")
    assert one["cameras_100m_100c_s1109"] == (100, 100, "overflow") and one["cameras_128m_128c_s1112"] == (128, 128, "overflow")
    assert one["cameras_129m_65c_s1113"] == (129, 65, "global") and one["cameras_129m_129c_s1114"] == (129, 129, "global")
    assert one["cameras_300m_65c_s1115"] == (300, 65, "global") and one["cameras_300m_200c_s1116"] == (300, 200, "global")
    assert _paths(lc.CASE_BY_NAME["mixed_workgroup"]) == ["lo", "hi", "global", "overflow"]
    assert [int(c["group_start"][-1]) for c in lc.CASES[:16]] == [4, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 130, 255, 256, 257, 600]
    assert sorted(len(c["group_start"]) - 1 for c in lc.CASES if c["name"].startswith("groups_")) == [1, 2, 3, 4, 5, 9]
    assert np.diff(lc.CASE_BY_NAME["empty_groups"]["group_start"]).tolist() == [0, 8, 0, 9, 0]


def test_the_register_sweep_uses_both_mask_halves():
    """'hi' clusters do emit segments whose end points belong to members above 63 (the open_hi half) and below"""
    for name in ("members_65", "members_128", "cameras_128m_64c_s1110"):
        idx = np.array(lc.model_of(lc.CASE_BY_NAME[name])[0]["structure"]).ravel() >> 1
        assert (idx >= 64).any() and (idx < 64).any(), name


def test_sweep_shapes_give_what_they_were_built_for():
    n_seg = {name: [len(f["structure"]) for f in lc.model_of(lc.CASE_BY_NAME[name])] for name in NAMES}
    assert n_seg["triples_126"] == [42] and n_seg["triples_129"] == [43]
    assert n_seg["oscillating_2_3"] == [30]
    assert n_seg["two_cameras"] == [0] and n_seg["three_cameras_never_overlapping"] == [0] and n_seg["all_points_identical"] == [0]
    assert n_seg["empty_groups"][0::2] == [0, 0, 0]
    assert n_seg["identical_member_pairs"] == [4] and n_seg["camera_count_above_1"][0] >= 5 and n_seg["p2_before_p1"][0] >= 1
    # every member of p2_before_p1 runs against the direction, about a third of the members elsewhere
    (pts, _), fit = lc.case_clusters(lc.CASE_BY_NAME["p2_before_p1"])[0], lc.model_of(lc.CASE_BY_NAME["p2_before_p1"])[0]
    assert np.all(fit["dist64"][1::2] < fit["dist64"][0::2]) or np.all(fit["dist64"][1::2] > fit["dist64"][0::2])
    d = lc.model_of(lc.CASE_BY_NAME["members_96"])[0]["dist64"]
    assert 10 < (d[1::2] < d[0::2]).sum() < 86
    # a camera with three members open at once
    (pts, cams), fit = lc.case_clusters(lc.CASE_BY_NAME["camera_count_above_1"])[0], lc.model_of(lc.CASE_BY_NAME["camera_count_above_1"])[0]
    open_members, most = set(), 0
    for p in fit["order"]:
        open_members ^= {int(p) >> 1}
        most = max(most, max(Counter(int(cams[m]) for m in open_members).values(), default=0))
    assert most == 3
    # ties: the identical pairs are the only equal distances, and a segment ends on one of a pair
    fit = lc.model_of(lc.CASE_BY_NAME["identical_member_pairs"])[0]
    assert len(np.unique(fit["dist32"])) < len(fit["dist32"])
    # the tie between an end and a start: closed first the line breaks in two, opened first it does not -- both orders are in the table
    assert sorted(n_seg["end_and_start_tied"]) == [1, 2]
    cams = lc.case_clusters(lc.CASE_BY_NAME["camera_ids_0_and_ffffffff"])[0][1]
    assert {0, 0xFFFFFFFF} <= set(cams.tolist())


@pytest.mark.parametrize("where", ["after", "last"])
def test_overflow_cases_and_their_twins(where):
    case, twin = lc.CASE_BY_NAME["overflow_" + where], lc.CASE_BY_NAME["overflow_%s_twin" % where]
    assert twin["twin_of"] == case["name"]
    (pts, cams), fit = lc.case_clusters(case)[0], lc.model_of(case)[0]
    (tpts, tcams), tfit = lc.case_clusters(twin)[0], lc.model_of(twin)[0]
    assert _paths(case) == ["overflow"] and _paths(twin) == [{"after": "hi", "last": "lo"}[where]]     # (66 and 64 members)
    # the twin is the case without its last member, bit for bit
    assert len(tcams) == len(cams) - 1 and tpts.tobytes() == pts[:-2].tobytes() and np.array_equal(tcams, cams[:-1])
    step = lm.overflow_step(cams, fit["order"])
    pos = {int(p): k for k, p in enumerate(fit["order"])}
    emitted_before = sum(1 for _s, e in fit["structure"] if pos[e] < step)
    if where == "after":
        # 21 segments are out when the 65th camera is met; the closing chunk's segment exists only with that camera
        assert emitted_before == 21 and pos[2 * (len(cams) - 1)] == step
        assert len(fit["structure"]) == 22 and fit["structure"][:-1] == tfit["structure"]
    else:
        # met at the last step at which a camera can be met: the last member's first point, second to last of the sweep
        assert step == len(fit["order"]) - 2 and emitted_before == 21
        assert fit["structure"] == tfit["structure"] and len(tfit["structure"]) == 21
