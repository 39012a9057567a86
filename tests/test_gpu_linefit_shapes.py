"""l3d_fit_clusters / l3d_fit_labelled_clusters on the case table of tests/linefit_cases.py: every cluster-size and camera-count path of
k_fit_clusters (<= 64 members; 65-128 members, both halves of the open mask; the re-sweep when a 65th camera turns up; > 128 members in
global scratch), both sides of every boundary between them, and the edges of the k_lab_* grouping -- against the float64 model of
tests/linefit_model.py (numpy's eigh, no code of the product).

What is compared is the STRUCTURE.  The sweep emits input points (emit(start, get(p))), not projected ones, so with the identity as
inverse transform every emitted end point must be BIT-EQUAL to an inverse-transformed input point, and which point it is is a discrete
fact the model states: 2 * member + {0: P1, 1: P2}.  Where the model's point has bit-identical twins (the tie cases) any of them is the
same bytes and is accepted; nothing else is.  The conditions under which the model's structure is the only right one are asserted per
case by tests/test_linefit_cases_cpu.py.

With another inverse transform Q = Rinv (scale_inv P + tneg) the index check stays, and the coordinates must be within
    16 * 2^-53 * M_i,    M_i = sum_j |Rinv_ij| (|scale_inv P_j| + |tneg_j|)
of the float64 transform: coordinate i is three products Rinv_ij * (scale_inv * P_j + tneg_j) and two sums, the inner term a product and a
sum -- each rounded once, in the device's evaluation (which may contract a product and a sum into one rounding) as in numpy's; every
rounding is at most 2^-53 relative to a partial result that M_i bounds, there are at most 3 * 2 + 2 = 8 of them in either computation,
16 in both."""
import ctypes as C

import numpy as np
import pytest

import linefit_cases as lc
import linefit_model as lm

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in lc.CASES]


def _fit(ctx, case, group_start=None, member_hyp=None):
    return ctx.fit_clusters(case["group_start"] if group_start is None else group_start, case["member_hyp"] if member_hyp is None else member_hyp,
                            case["hyp"], case["hyp_cam"], case["Rinv"], case["scale_inv"], case["tneg"])


def _bytes(fits):
    return [b"".join(s.tobytes() + e.tobytes() for s, e in f) for f in fits]


def _check_point(case, raw, pts, got, want, what):
    """got (3,) must be input point `want` of the cluster"""
    if case["identity"]:
        same = [i for i in range(len(pts)) if pts[i].tobytes() == got.tobytes()]
        assert same, "%s: %r is no input point (the model's is %d: %r)" % (what, got, want, pts[want])
        assert want in same, "%s: input point %s, the model's is %d" % (what, same, want)
        assert all(pts[i].tobytes() == pts[want].tobytes() for i in same)
    else:
        M = np.abs(case["Rinv"]) @ (np.abs(case["scale_inv"] * raw[want]) + np.abs(case["tneg"]))
        assert np.all(np.abs(got - pts[want]) <= 16 * 2.0 ** -53 * M), "%s: %r, the model's point %d is %r" % (what, got, want, pts[want])
        near = np.abs(pts - got).max(axis=1)
        assert pts[int(np.argmin(near))].tobytes() == pts[want].tobytes(), "%s: nearest input point %d, the model's is %d" % (what, int(np.argmin(near)), want)


def check_against_model(case, fits):
    """segment counts and structure of every cluster of the case"""
    model = lc.model_of(case)
    gs, mh = case["group_start"], case["member_hyp"]
    assert len(fits) == len(model)
    assert [len(f) for f in fits] == [len(m["structure"]) for m in model], "%s: segments per cluster" % case["name"]
    for g, ((pts, _cams), m, f) in enumerate(zip(lc.case_clusters(case), model, fits)):
        k = mh[gs[g]:gs[g + 1]]
        raw = np.stack([case["hyp"]["P1"][k], case["hyp"]["P2"][k]], axis=1).reshape(-1, 3)
        for n, ((s, e), (ms, me)) in enumerate(zip(f, m["structure"])):
            _check_point(case, raw, pts, s, ms, "%s, cluster %d, segment %d, start" % (case["name"], g, n))
            _check_point(case, raw, pts, e, me, "%s, cluster %d, segment %d, end" % (case["name"], g, n))


@pytest.mark.parametrize("name", NAMES)
def test_fit_clusters_has_the_models_structure(gpu_ctx, name):
    case = lc.CASE_BY_NAME[name]
    check_against_model(case, _fit(gpu_ctx, case))


@pytest.fixture(scope="module")
def tables():
    """the whole table as one call per inverse transform: every identity case, and the transformed one"""
    return [lc.merged([c for c in lc.CASES if c["identity"]]), lc.merged([c for c in lc.CASES if not c["identity"]])]


def test_one_call_and_one_call_per_cluster_give_the_same_bytes_twice(gpu_ctx, tables):
    """the whole table in one call == every cluster in a call of its own (four clusters share a workgroup, no barrier in the kernel, scratch
    sized by the call), and again: the single calls run from the largest cluster to the smallest and then from the smallest to the
    largest, so every call but the first meets scratch a differently sized call left behind"""
    for t in tables:
        whole = _bytes(_fit(gpu_ctx, t))
        gs, mh = t["group_start"], t["member_hyp"]
        n = len(gs) - 1
        assert n >= 5 and sum(len(b) for b in whole) > 0
        by_size = sorted(range(n), key=lambda g: (-(gs[g + 1] - gs[g]), g))
        for order in (by_size, by_size[::-1]):
            for g in order:
                one = _bytes(_fit(gpu_ctx, t, [0, gs[g + 1] - gs[g]], mh[gs[g]:gs[g + 1]]))
                assert one == [whole[g]], "cluster %d of %d members" % (g, gs[g + 1] - gs[g])
        assert _bytes(_fit(gpu_ctx, t)) == whole
    assert len(tables[0]["group_start"]) - 1 == sum(len(c["group_start"]) - 1 for c in lc.CASES if c["identity"])


def _labels_for(rng, case, n_real, roots=None):
    """Nodes in a random order over ALL hypotheses of the case; the first n_real groups are clusters (root: one of their nodes, or the node
    roots[g] asks for), the hypotheses of the other groups stay alone.  -> labels, node_hyp, expected (group_start, member_hyp, kept groups)"""
    n = len(case["hyp"])
    gs, mh = case["group_start"], case["member_hyp"]
    node_hyp = rng.permutation(n).astype(np.int32)
    for g, root in (roots or {}).items():                                  # the node `root` becomes a member of group g
        want = int(mh[gs[g]])
        at = int(np.nonzero(node_hyp == want)[0][0])
        node_hyp[[root, at]] = node_hyp[[at, root]]
    node_of = np.empty(n, np.int64)
    node_of[node_hyp] = np.arange(n)
    labels = np.arange(n, dtype=np.int32)
    kept = {}
    for g in range(n_real):
        k = mh[gs[g]:gs[g + 1]]
        if len(k) == 0:
            continue
        root = (roots or {}).get(g, int(node_of[k[int(rng.integers(0, len(k)))]]))
        labels[node_of[k]] = root
        if len(k) >= 4 and len(set(case["hyp_cam"][k].tolist())) >= 4:
            kept[root] = g
    want_gs, want_mh, groups = [0], [], []
    for root in sorted(kept):
        g = kept[root]
        want_mh += mh[gs[g]:gs[g + 1]].tolist()
        want_gs.append(len(want_mh))
        groups.append(g)
    return labels, node_hyp, want_gs, want_mh, groups


def _check_labelled(ctx, case, labels, node_hyp, want_gs, want_mh):
    got_gs, got_mh, fits = ctx.fit_labelled_clusters(labels, node_hyp, case["hyp"], case["hyp_cam"], case["Rinv"], case["scale_inv"], case["tneg"])
    assert got_gs.tolist() == want_gs and got_mh.tolist() == want_mh
    ref = _fit(ctx, case, want_gs, want_mh) if len(want_gs) > 1 else []
    assert _bytes(fits) == _bytes(ref)
    return _bytes(fits)


def test_fit_labelled_clusters_on_the_table(gpu_ctx, tables):
    """labels built from the table's clusters plus 300 nodes that stay alone: the groups that qualify (>= 4 members from >= 4 cameras,
    line3D.cc:1324-1340) in ascending label order, their fits the bytes l3d_fit_clusters gives for them in the whole-table call"""
    rng = np.random.default_rng(1501)
    for t in tables:
        n_real = len(t["group_start"]) - 1
        clusters = []
        for g in range(n_real):
            k = t["member_hyp"][t["group_start"][g]:t["group_start"][g + 1]]
            clusters.append([(int(t["hyp_cam"][i]), t["hyp"]["P1"][i].copy(), t["hyp"]["P2"][i].copy()) for i in k])
        alone = [[(int(rng.integers(0, 200)), rng.normal(size=3), rng.normal(size=3))] for _ in range(300)]
        case = lc.make_case("labelled", 1501, clusters + alone, transform=lc.IDENT if t["identity"] else (t["Rinv"], t["scale_inv"], t["tneg"]))
        labels, node_hyp, want_gs, want_mh, groups = _labels_for(rng, case, n_real)
        dropped = set(range(n_real)) - set(groups)
        assert len(groups) >= 4 and (not t["identity"] or len(dropped) >= 6)          # (empty groups, two and three cameras, ...)
        got = _check_labelled(gpu_ctx, case, labels, node_hyp, want_gs, want_mh)
        whole = _bytes(_fit(gpu_ctx, t))
        assert got == [whole[g] for g in groups]


# ---- the edges of the grouping (k_lab_*)

def _grouping_case(seed, shapes, n_nodes):
    """shapes: (members, cameras) per cluster; hypotheses that stay alone fill the table up to n_nodes"""
    rng = np.random.default_rng(seed)
    clusters = [lc.random_cluster(rng, m, c, cam_base=10 * g) for g, (m, c) in enumerate(shapes)]
    n_alone = n_nodes - sum(m for m, _ in shapes)
    assert n_alone >= 0
    alone = [[(int(cam), np.zeros(3), np.zeros(3))] for cam in rng.integers(0, 50, n_alone)]
    return rng, lc.make_case("grouping", seed, clusters + alone)


def test_grouping_threshold_of_members_and_cameras(gpu_ctx):
    """exactly 4 members and 4 cameras: kept; 4 members and 3 cameras, 3 members and 3 cameras: dropped; 5 members and 4 cameras: kept"""
    rng, case = _grouping_case(1601, [(4, 4), (4, 3), (3, 3), (5, 4)], 40)
    labels, node_hyp, want_gs, want_mh, groups = _labels_for(rng, case, 4)
    assert sorted(groups) == [0, 3]
    _check_labelled(gpu_ctx, case, labels, node_hyp, want_gs, want_mh)


@pytest.mark.parametrize("n_nodes", [1, 40, 4096, 4097])
def test_grouping_root_labels_at_both_ends(gpu_ctx, n_nodes):
    """a kept cluster whose root label is 0 and one whose root label is n_nodes - 1, the largest label there is; 4096 and 4097 nodes sit
    on either side of a step of the key sort's bit count.  One node alone: no cluster."""
    if n_nodes == 1:
        rng, case = _grouping_case(1610, [], 1)
        labels, node_hyp, want_gs, want_mh, groups = _labels_for(rng, case, 0)
        assert want_gs == [0]
        _check_labelled(gpu_ctx, case, labels, node_hyp, want_gs, want_mh)
        return
    rng, case = _grouping_case(1610 + n_nodes, [(6, 5), (9, 4), (5, 5)], n_nodes)
    labels, node_hyp, want_gs, want_mh, groups = _labels_for(rng, case, 3, roots={0: n_nodes - 1, 2: 0})
    assert groups[0] == 2 and groups[-1] == 0 and len(groups) == 3 and labels.max() == n_nodes - 1 and labels.min() == 0
    got = _check_labelled(gpu_ctx, case, labels, node_hyp, want_gs, want_mh)
    assert all(len(b) > 0 for b in got)


def test_grouping_all_nodes_in_one_cluster(gpu_ctx):
    rng, case = _grouping_case(1621, [(200, 12)], 200)
    labels, node_hyp, want_gs, want_mh, groups = _labels_for(rng, case, 1)
    assert groups == [0] and len(set(labels.tolist())) == 1 and want_gs == [0, 200]
    assert len(_check_labelled(gpu_ctx, case, labels, node_hyp, want_gs, want_mh)[0]) > 0


def test_grouping_without_a_valid_cluster_returns_nothing_and_the_context_lives_on(gpu_ctx):
    """no cluster qualifies: every output pointer NULL, every count 0, L3D_OK -- and the next call on the same context works"""
    rng, case = _grouping_case(1631, [(4, 3), (3, 3), (12, 2)], 60)
    labels, node_hyp, want_gs, want_mh, groups = _labels_for(rng, case, 3)
    assert groups == []
    lab, nh = np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(node_hyp, np.int32)
    R, t = np.ascontiguousarray(case["Rinv"]).reshape(9), np.ascontiguousarray(case["tneg"])
    gs, mh, cnt, segs = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()
    ng, n = C.c_int(-1), C.c_int(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                                          # noqa: E731
    rc = gpu_ctx.lib.l3d_fit_labelled_clusters(gpu_ctx.h, p(lab), p(nh), C.c_int(len(lab)), p(case["hyp"]), p(case["hyp_cam"]), C.c_int(len(case["hyp"])),
                                               p(R), C.c_double(case["scale_inv"]), p(t), C.byref(gs), C.byref(mh), C.byref(ng), C.byref(cnt), C.byref(segs), C.byref(n))
    assert rc == 0 and ng.value == 0 and n.value == 0
    assert not gs and not mh and not cnt and not segs
    _check_labelled(gpu_ctx, case, labels, node_hyp, want_gs, want_mh)
    rng, case = _grouping_case(1632, [(7, 5)], 30)
    labels, node_hyp, want_gs, want_mh, groups = _labels_for(rng, case, 1)
    assert len(_check_labelled(gpu_ctx, case, labels, node_hyp, want_gs, want_mh)) == 1


# ---- the scan on its own

SCAN_SIZES = [0, 1, 7, 8, 2047, 2048, 2049, 4096, 4097, 2048 * 2048 - 1, 2048 * 2048, 2048 * 2048 + 1, 2048 * 2048 + 2049]


@pytest.fixture(scope="module")
def scan_values():
    """the value patterns at the largest size, cut to length per test: ones; random in [0, 3]; negative and positive values (the int32 sum wraps)"""
    rng = np.random.default_rng(1701)
    n = max(SCAN_SIZES)
    return {"ones": np.ones(n, np.int32), "random_0_3": rng.integers(0, 4, n).astype(np.int32),
            "negative": rng.integers(-2000000, 1000, n).astype(np.int32)}


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_sum_on_its_own(gpu_ctx, scan_values, n):
    """exclusive_sum_int (l3d_sort.hip: tiles of 2048, the tile sums scanned one level up -- three levels above 2048^2 entries) against
    numpy's cumsum in int64, wrapped to int32"""
    last = np.zeros(n, np.int32)
    if n:
        last[-1] = 12345
    for name, x in list((k, v[:n]) for k, v in scan_values.items()) + [("zero_but_the_last", last)]:
        want = np.zeros(n, np.int64)
        if n > 1:
            want[1:] = np.cumsum(x[:-1].astype(np.int64))
        got = gpu_ctx.test_exclusive_sum(x)
        assert got.dtype == np.int32 and np.array_equal(got, want.astype(np.int32)), (name, n)
    if n == max(SCAN_SIZES):
        assert np.cumsum(scan_values["negative"].astype(np.int64))[-1] < -2 ** 31          # (the negative pattern does wrap)
