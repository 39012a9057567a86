"""Every edge case of tests/verify_cases.py is the case its name claims (no GPU).  The claims are checked with numpy restatements written here -- the
3-D gate in float64 and in float32 (the reference's operations one rounding at a time), the depth bucket id of the window kernels, the confidence
of one (hypothesis, witness) pair in float64 -- which share no code with the product or the oracle; the oracle (contract build) only supplies the
confidences the claims are about.

Gate-edge cases, pairs (hypothesis, witness of its 102) on which the float32 gate and the float64 gate disagree, of 6528 each:
spatial_k 0.005: 95, 0.02: 114, 0.05: 106 -- the band of +-8 units in the last place holds the whole region in which rounding decides."""
import hashlib
import os

import numpy as np
import pytest

import l3d_oracle_pipeline as op
import verify_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = np.float32, np.float64


# ---- the models -------------------------------------------------------------------------------------------------------------------------------
def seg_slice(case, s):
    a, m = case["match_offsets"][s]
    return slice(int(a), int(a + m))


def rays64(case, s):
    M = case["RtKinv"].astype(F64)
    seg = case["src_segs"][s].astype(F64)
    out = []
    for x, y in ((seg[0], seg[1]), (seg[2], seg[3])):
        r = M @ np.array([x, y, 1.0])
        out.append(r / np.sqrt(r @ r))
    return out


def gate64(case, s, dh, dw):
    """the 3-D gate of hypothesis depths dh = (d1, d2) against witness depths dw [n, 2], everything in float64 from the float32 inputs"""
    C, sk = case["C_src"].astype(F64), F64(case["spatial_k"])
    ok = np.ones(len(dw), bool)
    for e, r in enumerate(rays64(case, s)):
        P = C + F64(dh[e]) * r
        Q = C[None, :] + dw[:, e].astype(F64)[:, None] * r[None, :]
        ok &= np.sqrt(((P[None, :] - Q) ** 2).sum(1)) <= sk * np.sqrt(((C - P) ** 2).sum())
    return ok


def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def rays32(case, s):
    M, seg = case["RtKinv"].astype(F32), case["src_segs"][s].astype(F32)
    out = []
    for x, y in ((seg[0], seg[1]), (seg[2], seg[3])):
        p = np.array([x, y, F32(1.0)], F32)
        r = np.zeros(3, F32)
        for i in range(3):
            acc = F32(0.0)
            for j in range(3):
                acc = F32(acc + F32(M[i, j] * p[j]))
            r[i] = acc
        inv = F32(1.0) / np.sqrt(_dot32(r, r))
        out.append((r * inv).astype(F32))
    return out


def gate32(case, s, dh, dw):
    """the same gate with the reference's float32 operations (unproject: C + depth * ray; lengths: sqrtf of the sum of squares left to right)"""
    C, sk = case["C_src"].astype(F32), F32(case["spatial_k"])
    ok = np.ones(len(dw), bool)
    for e, r in enumerate(rays32(case, s)):
        P = (C + F32(dh[e]) * r).astype(F32)
        Q = (C[None, :] + dw[:, e].astype(F32)[:, None] * r[None, :]).astype(F32)
        cp = (C - P).astype(F32)
        unc = F32(sk * np.sqrt(_dot32(cp, cp)))
        pq = (P[None, :] - Q).astype(F32)
        ok &= ~(np.sqrt(_dot32(pq, pq)) > unc)
    return ok


def conf64(case, s, dh, cams, dw, tq):
    """confidence of the hypothesis (depths dh) under witnesses (camera, depths, 2-D target segment), without the gate, in float64"""
    C = case["C_src"].astype(F64)
    r1, r2 = rays64(case, s)
    P1, P2 = C + F64(dh[0]) * r1, C + F64(dh[1]) * r2
    Pm = case["P"].astype(F64)[cams]
    pr = []
    for X in (P1, P2):
        x = Pm[:, :, :3] @ X + Pm[:, :, 3]
        pr.append(np.stack([x[:, 0] / x[:, 2], x[:, 1] / x[:, 2], np.ones(len(x))], 1))
    q1 = np.stack([tq[:, 0], tq[:, 1], np.ones(len(tq))], 1).astype(F64)
    q2 = np.stack([tq[:, 2], tq[:, 3], np.ones(len(tq))], 1).astype(F64)
    l1, l2 = np.cross(pr[0], pr[1]), np.cross(q1, q2)
    p2l = lambda l, p: np.abs((l * p).sum(1)) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2)
    dist = np.maximum(np.maximum(p2l(l2, pr[0]), p2l(l2, pr[1])), np.maximum(p2l(l1, q1), p2l(l1, q2)))
    Q1 = C[None, :] + dw[:, 0].astype(F64)[:, None] * r1[None, :]
    Q2 = C[None, :] + dw[:, 1].astype(F64)[:, None] * r2[None, :]
    v1 = (P1 - P2) / np.linalg.norm(P1 - P2)
    v2 = (Q1 - Q2) / np.linalg.norm(Q1 - Q2, axis=1)[:, None]
    ang = np.degrees(np.arccos(np.clip(v2 @ v1, -1.0, 1.0)))
    ang = np.where(ang > 90.0, 180.0 - ang, ang)
    sp, sa = F64(case["sigma_p"]), F64(case["sigma_a"])
    cd, ca = np.exp(-dist ** 2 / (2 * sp * sp)), np.exp(-ang ** 2 / (2 * sa * sa))
    return np.minimum(cd, ca), cd, ca


def bucket_ids(d1):
    """bucket of every first depth of ONE segment: (bits >> 15) - the segment's smallest, clamped to [0, 2047]; 0 for a depth that is not positive"""
    raw = (d1.astype(F32).view(np.uint32) >> vc.BUCKET_SHIFT).astype(np.int64)
    base = raw.min()
    return np.where(d1 > 0, np.clip(raw - base, 0, vc.BUCKETS - 1), 0), raw


def targets_of(case, sl):
    md = case["matches_data"][sl]
    cams = md[:, 1].astype(np.int64)
    return cams, case["tgt_segs"][case["camera_offsets"][cams, 0] + md[:, 2].astype(np.int64)]


# ---- the cases and the oracle's confidences, once ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge():
    lib = op.load_lib(libm=False)
    out = {}
    for kw in vc.EDGE_CASES:
        case = vc.make_edge_case(**kw)
        out[kw["name"]] = (case, op.verify_case(lib, case))
    return out


def test_digest_of_cases_is_unchanged():
    g = np.load(os.path.join(HERE, "golden", "verify_ref.npz"))
    for k, kw in enumerate(vc.CASES):
        case = vc.make_case(**kw)
        h = hashlib.sha256()
        for name in sorted(case):
            h.update(np.ascontiguousarray(case[name]).tobytes())
        assert h.digest() == g["c%d_digest" % k].tobytes(), k
    a, b = vc.make_case(seed=1), vc.make_case(seed=1, behind=False)
    neg = a["matches_depths"][:, 0] <= 0
    assert neg.sum() == 28 and (b["matches_depths"][:, :2] > 0).all()
    assert np.array_equal(a["matches_depths"][~neg], b["matches_depths"][~neg]) and np.array_equal(a["matches_data"], b["matches_data"])


def test_every_case_keeps_some_and_not_all(edge):
    for name, (case, conf) in edge.items():
        kept = int((conf > 1.0).sum())
        assert 0 < kept < len(conf), name
        row_start, meta = vc.to_rows(case)
        S, N = len(case["match_offsets"]), len(case["camera_offsets"])
        assert row_start[-1] == len(conf) and np.all(np.diff(row_start) >= 0), name
        rows = np.repeat(np.arange(S * N), np.diff(row_start))
        assert np.array_equal(rows % N, meta[:, 1]) and np.all(meta[:, 0] < case["camera_offsets"][meta[:, 1], 1]), name
        assert (case["matches_depths"][:, :2] > 0).all(), name               # (the product's contract)


def test_sizes_case(edge):
    case, _ = edge["sizes"]
    m = sorted(int(v) for v in case["match_offsets"][:, 1])
    N = len(case["camera_offsets"])
    assert N == 5
    for want in (0, 1, 2, 63, 64, 65, 2048, 2049, 3000):
        assert want in m, want
    for path in (1, 2):
        mm = vc.vw_mmax(max(m), N, path)
        assert 65 < mm < 2048 and mm in m and mm + 1 in m, path
        assert vc.vw_lds_bytes(mm, N) <= vc.VW_LDS_BUDGET
    assert vc.vw_mmax(3000, 5, 1) == 533 and vc.vw_mmax(3000, 5, 2) == 508
    nog, _ = edge["no_gate"]
    assert float(nog["spatial_k"]) == 0.0 and float(case["spatial_k"]) > 0
    for k in case:
        if k != "spatial_k":
            assert np.array_equal(case[k], nog[k]), k


def test_one_camera_case(edge):
    case, conf = edge["one_camera"]
    a, b = seg_slice(case, 0), seg_slice(case, 1)
    assert len(set(case["matches_data"][a, 1])) == 1 and a.stop - a.start >= 100
    assert not conf[a].any()                                                 # own-camera skip: nobody supports anybody
    cams = case["matches_data"][b, 1]
    vals, cnt = np.unique(cams, return_counts=True)
    assert b.stop - b.start == 200 and sorted(cnt) == [1, 199]
    foreign = np.flatnonzero(cams == vals[np.argmin(cnt)])[0]
    assert 0.5 < conf[b][foreign] <= 1.0 and (conf[b] <= 1.0).all() and (conf[b] > 0.5).sum() > 100


def test_dense_cluster_case(edge):
    case, conf = edge["dense_cluster"]
    sl = seg_slice(case, 0)
    d = case["matches_depths"][sl, :2].astype(F64)
    assert len(d) == 600 and len(case["camera_offsets"]) == 8
    assert (np.abs(d / np.median(d, 0) - 1.0) < 1e-3).all()
    cams = case["matches_data"][sl, 1]
    for h in range(0, 600, 7):
        ok = gate64(case, 0, d[h], d) & (cams != cams[h])
        assert ok.sum() > 3 * 128, h                                         # several drains of the 128-entry ring per hypothesis
    assert (conf[sl] > 1.0).all()


@pytest.mark.parametrize("name", ["gate_edge_0.005", "gate_edge_0.02", "gate_edge_0.05"])
def test_gate_edge_case(edge, name):
    case, conf = edge[name]
    ks, ng = np.array(vc.GATE_KS), len(vc.GATE_GROUPS)
    assert len(case["match_offsets"]) == vc.GATE_HYP
    pass64 = np.zeros((vc.GATE_HYP, ng, len(ks)), bool)
    pass32 = np.zeros_like(pass64)
    worst = 0.0
    for s in range(vc.GATE_HYP):
        sl = seg_slice(case, s)
        d = case["matches_depths"][sl, :2]
        cams, tq = targets_of(case, sl)
        assert cams[0] == 0 and np.array_equal(cams[1:], np.repeat(np.arange(1, ng + 1), len(ks)))
        c, cd, ca = conf64(case, s, d[0], cams[1:], d[1:], tq[1:])
        assert (c > 0.5).all() and (cd < ca).all()                           # a witness the gate admits counts, and by its distance term
        g64, g32 = gate64(case, s, d[0], d[1:]), gate32(case, s, d[0], d[1:])
        pass64[s], pass32[s] = g64.reshape(ng, -1), g32.reshape(ng, -1)
        # the hypothesis' confidence under the float32 gate: per camera the best admitted witness; the oracle gives it to 2e-3 (float32 projections),
        # a witness more or less would move it by 6e-3 or more
        cm = np.where(g32, c, 0.0).reshape(ng, -1)
        steps = np.abs(np.diff(np.sort(c.reshape(ng, -1), axis=1), axis=1))
        assert steps.min() > 6e-3
        worst = max(worst, abs(cm.max(1).sum() - float(conf[sl][0])))
        for g, (which, side) in enumerate(vc.GATE_GROUPS):                   # the depths are what the table says
            e = {"first": [0], "second": [1], "both": [0, 1]}[which]
            w = d[1 + g * len(ks):1 + (g + 1) * len(ks)]
            for col in (0, 1):
                if col in e:
                    centre = F32(F64(d[0, col]) * (1.0 + side * F64(case["spatial_k"])))
                    assert np.array_equal(w[:, col].view(np.int32) - centre.view(np.int32), ks)
                else:
                    assert (w[:, col] == d[0, col]).all()
    assert worst < 2e-3, worst
    for k in range(len(ks)):
        assert pass64[:, :, k].any() and not pass64[:, :, k].all(), ks[k]   # witnesses on both sides of the exact gate for every k
    for g in range(ng):
        assert pass64[:, g, :].any() and not pass64[:, g, :].all(), g
    disagree = int((pass64 != pass32).sum())
    print(name, "float32 and float64 gates disagree on", disagree, "of", pass64.size)
    assert disagree > 0


def test_bucket_edge_case(edge):
    case, _ = edge["bucket_edge"]
    found = 0
    for s in range(len(case["match_offsets"])):
        sl = seg_slice(case, s)
        d1 = case["matches_depths"][sl, 0]
        cams = case["matches_data"][sl, 1]
        b, _raw = bucket_ids(d1)
        bits = d1.view(np.int32).astype(np.int64)
        low = bits & 0x7fff
        for pat in (0, 1, 0x7ffe, 0x7fff):
            assert (low == pat).sum() >= 13, (s, pat)
        order = np.argsort(bits, kind="stable")
        for i, j in zip(order[:-1], order[1:]):
            if bits[j] - bits[i] == 1 and b[j] != b[i] and cams[i] != cams[j]:
                assert b[j] == b[i] + 1 and low[i] == 0x7fff and low[j] == 0
                found += 1
        assert 0 < b.max() < vc.BUCKETS - 1                                  # (nothing clamps here)
    assert found >= 20


def test_octaves_case(edge):
    case, conf = edge["octaves"]
    sl = seg_slice(case, 0)
    b, raw = bucket_ids(case["matches_depths"][sl, 0])
    assert raw.max() - raw.min() > vc.BUCKETS and (b == vc.BUCKETS - 1).sum() > 10 and len(np.unique(b)) > 50
    ratio = case["matches_depths"][sl, 0].astype(F64)
    assert np.log2(ratio.max() / ratio.min()) > 12.0
    sl = seg_slice(case, 1)
    d1 = case["matches_depths"][sl, 0]
    b, raw = bucket_ids(d1)
    assert (d1 == F32(1e-30)).sum() == 1 and b[d1 == F32(1e-30)][0] == 0 and (b[d1 != F32(1e-30)] == vc.BUCKETS - 1).all()
    assert (conf[sl] > 1.0).sum() > 20                                       # (and the clamped cluster still supports itself)
    sl = seg_slice(case, 2)
    assert sl.stop - sl.start == 1 and case["matches_depths"][sl, 0][0] == F32(1e-30) and conf[sl][0] == 0.0


def test_far_origin_case(edge):
    case, conf = edge["far_origin"]
    near = vc.make_case(1, spatial_k=0.005, behind=False)
    assert np.allclose(case["C_src"].astype(F64) - near["C_src"], [5000.0, -3000.0, 2000.0], atol=1e-3)
    assert np.array_equal(case["matches_depths"], near["matches_depths"]) and float(case["spatial_k"]) == float(F32(0.005))
    # one unit in the last place of |C| against the gate's width: the exact gate is noisy at the per-cent level here, not at 1e-7
    assert np.spacing(F32(5000.0)) / (0.005 * 2.5) > 0.03


def test_ties_case(edge):
    case, conf = edge["ties"]
    sl = seg_slice(case, 0)
    c, md, dep = conf[sl], case["matches_data"][sl], case["matches_depths"][sl]
    i, j = vc.TIES_AT, vc.TIES_AT + vc.TIES_APART
    assert len(c) == 1500 and np.array_equal(md[i], md[j]) and np.array_equal(dep[i, :2], dep[j, :2])
    assert c[i] == c[j] == c.max() and np.flatnonzero(c == c.max()).tolist() == [i, j]     # the copies, and nobody else, hold the maximum
    assert c[i] > 2.9
    for unit in (256, 512):
        assert i // unit != j // unit                                        # (units of the LIST; the walk's units cut the bucket order, see ties_flat)
    assert np.array_equal(md[600], md[601]) and np.array_equal(dep[600, :2], dep[601, :2]) and c[600] == c[601] and 600 // 256 == 601 // 256


def test_ties_flat_case(edge):
    case, conf = edge["ties_flat"]
    assert float(case["sigma_p"]) == 1e4 and float(case["sigma_a"]) == 1e4
    for s in (0, 1):
        sl = seg_slice(case, s)
        c = conf[sl]
        top = np.flatnonzero(c == c.max())
        assert c.max() == len(case["camera_offsets"]) - 1                    # the count of the other cameras: every one supports with exactly 1.0f
        assert len(top) > 256                                                # on average more than one tied maximum per thread of a workgroup
        d = case["matches_depths"][sl, :2][top]
        assert len(np.unique(d, axis=0)) == len(top)                         # ... all with depths of their own: WHICH one wins shows in the result


@pytest.mark.parametrize("N", [17, 24])
def test_many_cameras_case(edge, N):
    case, _ = edge["many_cameras_%d" % N]
    m = case["match_offsets"][:, 1]
    assert len(case["camera_offsets"]) == N and m.max() == 3000 and len(m) == 31 and (np.sort(m)[:-1] < 60).all()
    assert len(np.unique(case["matches_data"][:, 1])) == N


def test_contract_oracle_agrees_with_libm_oracle(edge):
    """the rule of test_oracle_pins._verify_checks for the contract build: within 5e-6 and the same kept set"""
    libm = op.load_lib(libm=True)
    for name, (case, conf) in edge.items():
        ref = op.verify_case(libm, case)
        assert np.max(np.abs(conf - ref), initial=0) <= 5e-6, name
        assert np.array_equal(conf > 1.0, ref > 1.0), name


def test_reference_vectors_of_the_edge_cases(edge):
    """tests/golden/verify_edges_ref.npz: what the reference's own K_verify_matches text gives for EDGE_CASES (make_golden_verify.py)"""
    g = np.load(os.path.join(HERE, "golden", "verify_edges_ref.npz"))
    libm = op.load_lib(libm=True)
    for name, (case, conf) in edge.items():
        h = hashlib.sha256()
        for k in sorted(case):
            h.update(np.ascontiguousarray(case[k]).tobytes())
        assert h.digest() == g[name + "_digest"].tobytes(), name
        want = g[name + "_conf"]
        assert op.verify_case(libm, case).tobytes() == want.tobytes(), name
        assert np.max(np.abs(conf - want), initial=0) <= 5e-6 and np.array_equal(conf > 1.0, want > 1.0), name


def test_long_runs_case():
    """EXIST_CASES: (segment, camera) runs of 300 and 600, of exactly 256 and 257, of 513 -- and shorter ones -- with distinct, ascending targets, so
    that a shuffled row has one right order; the shuffle moves entries inside the chosen cameras' rows only and really moves them"""
    assert [kw["name"] for kw in vc.EXIST_CASES] == ["long_runs"]
    case = vc.make_edge_case("long_runs")
    row_start, meta = vc.to_rows(case)
    N = 5
    assert np.diff(row_start).reshape(-1, N).tolist() == [list(r) for r in vc.RUN_SIZES]
    runs = np.diff(row_start).reshape(-1, N)[:, [1, 3]].reshape(-1).tolist()
    assert sorted(runs) == [0, 1, 2, 256, 257, 300, 513, 600]
    for row in range(len(row_start) - 1):
        assert np.all(np.diff(meta[row_start[row]:row_start[row + 1], 0].astype(np.int64)) > 0), row
    assert (case["matches_depths"][:, :2] > 0).all()
    conf = op.verify_case(op.load_lib(libm=False), case)
    assert 0 < (conf > 1.0).sum() < len(conf)
    m2, d2, perm = vc.shuffle_rows(row_start, meta, case["matches_depths"], N, (1, 3), 5)
    moved = perm != np.arange(len(perm))
    assert set(meta[moved, 1].tolist()) == {1, 3} and moved.sum() > 1800
    assert np.array_equal(np.sort(perm), np.arange(len(perm))) and np.array_equal(m2[:, 1], meta[:, 1])
    for row in range(len(row_start) - 1):        # a shuffled row holds the same entries
        a, b = row_start[row], row_start[row + 1]
        assert sorted(m2[a:b, 0].tolist()) == meta[a:b, 0].tolist()
