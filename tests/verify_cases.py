"""Seeded candidate lists for the K_verify_matches pin (tests/test_oracle_pins.py, tests/golden/make_golden_verify.py): one source view with S
segments, N neighbour cameras, per source segment a (camera, target)-sorted list of candidates as compute_pairwise_matches packs them
(cudawrapper.cu:958-1003) -- clusters of hypotheses at nearly the same depths (they support each other through the gate), outliers, several
candidates of one camera in a row (the per-camera maximum), candidates of the hypothesis's own camera (skipped), projections behind a camera.

EDGE_CASES / make_edge_case: candidate lists built to break stage 2's depth-window search (tests/test_verify_cases_cpu.py asserts that each is
the case its name claims, tests/test_gpu_verify_variants.py runs every kernel variant on them): segment sizes at every boundary of the
kernels, runs of one camera, a dense cluster, witnesses within ulps of the 3-D gate's edge, first depths at the ends of depth buckets, more
octaves of depth than buckets, a scene far from the origin, tied best confidences, 17 and 24 cameras, no gate.  to_rows converts a case to
the product's layout (row starts per (segment, camera), (target, camera) per candidate)."""
import numpy as np

F32 = np.float32


def make_case(seed, S=40, N=5, m_max=30, spatial_k=0.02, sigma_p=2.5, sigma_a=10.0, behind=True, shift=(0.0, 0.0, 0.0)):
    """behind=False: no hypothesis behind the source camera (the product's contract: positive depths), everything else as with True.
    shift: the whole scene translated (cameras and points; the images stay the same up to float32 rounding of P and C_src)."""
    shift = np.asarray(shift, np.float64)
    rng = np.random.default_rng(seed)
    Ks = np.array([[1500.0, 0, 960.0], [0, 1500.0, 540.0], [0, 0, 1.0]])

    def look_at(C):
        z = -C / np.linalg.norm(C)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        return np.stack([x, y, z])
    C_src = np.array([4.0, 0.2, 0.1])
    R_src = look_at(C_src)
    C_src = C_src + shift
    RtKinv = (R_src.T @ np.linalg.inv(Ks)).astype(F32)
    src = np.empty((S, 4), F32)
    src[:, 0:2] = (rng.random((S, 2)) * [1600, 900] + [150, 90]).astype(F32)
    src[:, 2:4] = src[:, 0:2] + rng.normal(0, 60, (S, 2)).astype(F32)
    P = np.empty((N, 3, 4), F32)
    cams = []
    for c in range(N):
        th = 0.25 * (c + 1) * (1 if c % 2 else -1)
        Cc = np.array([4.0 * np.cos(th), 0.3 * c - 0.5, 4.0 * np.sin(th)])
        Rc = look_at(Cc)
        Cc = Cc + shift
        cams.append((Rc, Cc))
        P[c] = (Ks @ np.concatenate([Rc, (-Rc @ Cc)[:, None]], 1)).astype(F32)

    def ray(p):
        r = RtKinv.astype(np.float64) @ np.array([p[0], p[1], 1.0])
        return r / np.linalg.norm(r)

    data, depths, offsets, tgt_by_cam = [], [], np.zeros((S, 2), np.int32), [[] for _ in range(N)]
    for s in range(S):
        m = int(rng.integers(0, m_max))
        base1, base2 = rng.uniform(2.5, 5.5), rng.uniform(2.5, 5.5)
        rows = []
        for _ in range(m):
            c = int(rng.integers(0, N))
            kind = rng.integers(0, 5)
            f1 = 1.0 + (rng.normal(0, 0.004) if kind <= 2 else rng.normal(0, 0.2))          # cluster vs outlier
            f2 = 1.0 + (rng.normal(0, 0.004) if kind <= 2 else rng.normal(0, 0.2))
            d1, d2 = base1 * f1, base2 * f2
            if kind == 4 and rng.random() < 0.2 and behind:
                d1 = -d1                                                                   # behind the source camera
            X1, X2 = C_src + d1 * ray(src[s, 0:2]), C_src + d2 * ray(src[s, 2:4])
            q = []
            for X in (X1, X2):
                x = P[c].astype(np.float64) @ np.array([X[0], X[1], X[2], 1.0])
                q += [x[0] / x[2] + rng.normal(0, 1.0), x[1] / x[2] + rng.normal(0, 1.0)] if abs(x[2]) > 1e-9 else [0.0, 0.0]
            rows.append((c, q, d1, d2, rng.uniform(2, 6), rng.uniform(2, 6)))
        rows.sort(key=lambda r: r[0])
        offsets[s] = (len(data), len(rows))
        for c, q, d1, d2, d3, d4 in rows:
            tgt_by_cam[c].append(q)
            data.append((s, c, len(tgt_by_cam[c]) - 1, 0.0))
            depths.append((d1, d2, d3, d4))
    cam_off = np.zeros((N, 2), np.int32)
    tgt = []
    for c in range(N):
        cam_off[c] = (len(tgt), len(tgt_by_cam[c]))
        tgt += tgt_by_cam[c]
    return dict(matches_data=np.array(data, F32).reshape(-1, 4), matches_depths=np.array(depths, F32).reshape(-1, 4), match_offsets=offsets,
                camera_offsets=cam_off, src_segs=src, RtKinv=RtKinv, C_src=C_src.astype(F32), tgt_segs=np.array(tgt, F32).reshape(-1, 4), P=P,
                sigma_p=F32(sigma_p), sigma_a=F32(sigma_a), spatial_k=F32(spatial_k))


CASES = [dict(seed=1), dict(seed=2, S=60, N=8, m_max=50), dict(seed=3, spatial_k=0.0), dict(seed=4, S=25, N=3, m_max=80, spatial_k=0.05),
         dict(seed=5, S=80, N=12, m_max=40, sigma_p=1.0, sigma_a=5.0)]


# ---- the product's layout ------------------------------------------------------------------------------------------------------------------
def to_rows(case):
    """(row_start [S*N + 1], cand_meta [R, 2] = (target id within its camera, camera)) of a case: the rows of a segment are sorted by camera, so a
    row is a run of one camera inside the segment's slice and its start is a count."""
    md, mo = case["matches_data"], case["match_offsets"]
    S, N, R = len(mo), len(case["camera_offsets"]), len(md)
    seg, cam = md[:, 0].astype(np.int64), md[:, 1].astype(np.int64)
    assert np.all(np.diff(seg * N + cam) >= 0) and np.array_equal(np.bincount(seg, minlength=S), mo[:, 1])
    row_start = np.zeros(S * N + 1, np.int32)
    row_start[1:] = np.cumsum(np.bincount(seg * N + cam, minlength=S * N))
    return row_start, np.stack([md[:, 2], md[:, 1]], 1).astype(np.uint32).reshape(R, 2)


# the window kernel's LDS image (l3d_verify_window.hip): bytes of an image of `mmax` candidates for N cameras and 256 threads, the default budget,
# and the two call sites' way to the image size from the largest segment -- what decides which segments take the scratch blocks
VW_LDS_BUDGET = 24000


def vw_lds_bytes(mmax, N):
    return (mmax + 8) * 16 + 256 * N * 4 + 4 * 128 * 16 + N * 52 + 16


def vw_fit_mmax(want, N):
    while want > 64 and vw_lds_bytes(want, N) > VW_LDS_BUDGET:
        want = want * 3 // 4
    return want


def vw_mmax(largest, N, path):
    """the image size of the seam call (path 1) and of the chains (path 2) for a list whose largest segment has `largest` candidates"""
    return vw_fit_mmax(largest if path == 1 else largest + largest // 4 + 64, N)


# ---- edge cases ----------------------------------------------------------------------------------------------------------------------------
class _Scene:
    """make_case's geometry without its random draws: the source camera, N cameras on the circle, float32 tables"""

    def __init__(self, N):
        Ks = np.array([[1500.0, 0, 960.0], [0, 1500.0, 540.0], [0, 0, 1.0]])

        def look_at(C):
            z = -C / np.linalg.norm(C)
            x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
            y = np.cross(z, x)
            return np.stack([x, y, z])
        self.C = np.array([4.0, 0.2, 0.1])
        self.RtKinv = (look_at(self.C).T @ np.linalg.inv(Ks)).astype(F32)
        self.P = np.empty((N, 3, 4), F32)
        for c in range(N):
            th = 0.25 * (c + 1) * (1 if c % 2 else -1)
            Cc = np.array([4.0 * np.cos(th), 0.3 * c - 0.5, 4.0 * np.sin(th)])
            Rc = look_at(Cc)
            self.P[c] = (Ks @ np.concatenate([Rc, (-Rc @ Cc)[:, None]], 1)).astype(F32)
        self.N = N

    def rays(self, seg):
        r = self.RtKinv.astype(np.float64) @ np.array([[seg[0], seg[2]], [seg[1], seg[3]], [1.0, 1.0]])
        return r / np.linalg.norm(r, axis=0)                                   # columns: the rays of the two end points

    def targets(self, seg, cams, p1, p2, off):
        """per row the 2-D segment in camera cams[i] of the 3-D points at depths (p1[i], p2[i]) on the source segment's rays, moved by
        off[i] (4 numbers, pixels); a point no camera can image gives (0, 0)"""
        r = self.rays(seg)
        q = np.zeros((len(cams), 4))
        Pc = self.P.astype(np.float64)[cams]
        for e, d in ((0, np.asarray(p1, np.float64)), (1, np.asarray(p2, np.float64))):
            X = self.C[None, :] + d[:, None] * r[:, e][None, :]
            x = np.einsum("nij,nj->ni", Pc[:, :, :3], X) + Pc[:, :, 3]
            ok = np.abs(x[:, 2]) > 1e-9
            z = np.where(ok, x[:, 2], 1.0)
            q[:, 2 * e] = np.where(ok, x[:, 0] / z, 0.0)
            q[:, 2 * e + 1] = np.where(ok, x[:, 1] / z, 0.0)
        return q + np.asarray(off, np.float64) * (np.abs(q).sum(1) > 0)[:, None]


def _pack(scene, src, segs, spatial_k, sigma_p, sigma_a):
    """segs: per source segment a dict of equally long arrays cam, d1, d2, q [m, 4] (and optionally d3, d4) in the order wanted WITHIN a camera;
    rows are put into camera order (stable) and the targets numbered per camera in order of appearance, as make_case does"""
    N = scene.N
    data, depths, tgt_by_cam, counts = [], [], [[] for _ in range(N)], np.zeros(N, np.int64)
    offsets = np.zeros((len(segs), 2), np.int32)
    n = 0
    for s, g in enumerate(segs):
        cam = np.asarray(g["cam"], np.int64)
        m = len(cam)
        order = np.argsort(cam, kind="stable")
        cam = cam[order]
        tid = np.zeros(m, np.int64)
        for c in range(N):
            k = cam == c
            tid[k] = counts[c] + np.arange(int(k.sum()))
            counts[c] += int(k.sum())
            tgt_by_cam[c].append(np.asarray(g["q"], np.float64).reshape(m, 4)[order][k])
        d = np.empty((m, 4))
        d[:, 0], d[:, 1] = np.asarray(g["d1"])[order], np.asarray(g["d2"])[order]
        d[:, 2] = np.asarray(g.get("d3", np.full(m, 3.0)))[order] if m else 0
        d[:, 3] = np.asarray(g.get("d4", np.full(m, 4.0)))[order] if m else 0
        data.append(np.stack([np.full(m, float(s)), cam.astype(np.float64), tid.astype(np.float64), np.zeros(m)], 1))
        depths.append(d)
        offsets[s] = (n, m)
        n += m
    cam_off = np.zeros((N, 2), np.int32)
    tgt, t0 = [], 0
    for c in range(N):
        blk = np.concatenate(tgt_by_cam[c]) if tgt_by_cam[c] else np.zeros((0, 4))
        cam_off[c] = (t0, len(blk))
        t0 += len(blk)
        tgt.append(blk)
    return dict(matches_data=np.concatenate(data).astype(F32).reshape(-1, 4), matches_depths=np.concatenate(depths).astype(F32).reshape(-1, 4),
                match_offsets=offsets, camera_offsets=cam_off, src_segs=np.asarray(src, F32).reshape(-1, 4), RtKinv=scene.RtKinv, C_src=scene.C.astype(F32),
                tgt_segs=np.concatenate(tgt).astype(F32).reshape(-1, 4), P=scene.P, sigma_p=F32(sigma_p), sigma_a=F32(sigma_a), spatial_k=F32(spatial_k))


def _src_segments(rng, S, long=False):
    src = np.empty((S, 4), F32)
    if long:        # segments across most of the image: a change of ONE end point's depth by a few per cent turns the 3-D line by a few degrees only
        src[:, 0:2] = (rng.random((S, 2)) * [200, 700] + [200, 190]).astype(F32)
        src[:, 2:4] = src[:, 0:2] + (rng.random((S, 2)) * [200, 100] + [1100, -50]).astype(F32)
    else:
        src[:, 0:2] = (rng.random((S, 2)) * [1600, 900] + [150, 90]).astype(F32)
        src[:, 2:4] = src[:, 0:2] + rng.normal(0, 60, (S, 2)).astype(F32)
    return src


def _mixed(rng, scene, seg, m, base=None, cluster=0.6, spread=0.004, noise=1.0):
    """m candidates of one segment as make_case mixes them: a cluster around one depth pair, outliers, random cameras, targets consistent with the
    depths up to `noise` pixels"""
    b1, b2 = (rng.uniform(2.5, 5.5), rng.uniform(2.5, 5.5)) if base is None else base
    cam = rng.integers(0, scene.N, m)
    inl = rng.random(m) < cluster
    d1 = b1 * (1.0 + np.where(inl, rng.normal(0, spread, m), rng.normal(0, 0.2, m)))
    d2 = b2 * (1.0 + np.where(inl, rng.normal(0, spread, m), rng.normal(0, 0.2, m)))
    d1, d2 = np.maximum(d1, 0.05).astype(F32), np.maximum(d2, 0.05).astype(F32)
    return dict(cam=cam, d1=d1, d2=d2, q=scene.targets(seg, cam, d1, d2, rng.normal(0, noise, (m, 4))), d3=rng.uniform(2, 6, m), d4=rng.uniform(2, 6, m))


def _join(*parts):
    keys = ("cam", "d1", "d2", "q", "d3", "d4")
    out = {}
    for k in keys:
        out[k] = np.concatenate([np.asarray(p[k] if k in p else np.full(len(p["cam"]), 3.0 if k == "d3" else 4.0)) for p in parts])
    return out


SIZES_M = (0, 1, 2, 63, 64, 65, 2048, 2049, 3000)
GATE_KS = tuple(range(-8, 9))
GATE_GROUPS = (("first", +1), ("first", -1), ("second", +1), ("second", -1), ("both", +1), ("both", -1))     # group g lives in camera g + 1
GATE_HYP = 64
TIES_AT, TIES_APART = 350, 700
BUCKET_SHIFT, BUCKETS = 15, 2048


def bump(x, k):
    """the float32 k units in the last place above x (positive floats)"""
    return (np.asarray(x, F32).view(np.int32) + np.int32(k)).view(F32)


def make_edge_case(name, **kw):
    rng = np.random.default_rng(hash_name("sizes" if name == "no_gate" else name))     # (no_gate: the sizes case's list)
    if name in ("sizes", "no_gate"):
        # every boundary of the kernels in one list: the empty epilogue, a wave, the LDS image of either call site (and one more: scratch block), the
        # 2048 candidates a workgroup keeps in registers (and one more: re-read), several rounds of hypotheses
        N = 5
        ms = sorted(set(SIZES_M) | {vw_mmax(max(SIZES_M), N, 1), vw_mmax(max(SIZES_M), N, 1) + 1, vw_mmax(max(SIZES_M), N, 2), vw_mmax(max(SIZES_M), N, 2) + 1})
        scene = _Scene(N)
        order = rng.permutation(len(ms))
        src = _src_segments(rng, len(ms))
        return _pack(scene, src, [_mixed(rng, scene, src[s], ms[order[s]]) for s in range(len(ms))], 0.0 if name == "no_gate" else 0.02, 2.5, 10.0)
    if name == "one_camera":
        scene = _Scene(5)
        src = _src_segments(rng, 4)
        a = _mixed(rng, scene, src[0], 150, cluster=0.8)
        a["cam"][:] = 2
        a["q"] = scene.targets(src[0], a["cam"], a["d1"], a["d2"], rng.normal(0, 1.0, (150, 4)))
        b = _mixed(rng, scene, src[1], 200, cluster=1.0)
        b["cam"][:] = 1
        b["cam"][77] = 3                                                       # the one foreign candidate
        b["q"] = scene.targets(src[1], b["cam"], b["d1"], b["d2"], rng.normal(0, 0.5, (200, 4)))
        return _pack(scene, src, [a, b, _mixed(rng, scene, src[2], 90), _mixed(rng, scene, src[3], 40)], 0.02, 2.5, 10.0)
    if name == "dense_cluster":
        scene = _Scene(8)
        src = _src_segments(rng, 2)
        a = _mixed(rng, scene, src[0], 600, base=(3.7, 4.1), cluster=1.0)
        a["d1"], a["d2"] = (3.7 * (1.0 + rng.uniform(-8e-4, 8e-4, 600))).astype(F32), (4.1 * (1.0 + rng.uniform(-8e-4, 8e-4, 600))).astype(F32)
        a["q"] = scene.targets(src[0], a["cam"], a["d1"], a["d2"], rng.normal(0, 1.0, (600, 4)))
        return _pack(scene, src, [a, _mixed(rng, scene, src[1], 60)], 0.02, 2.5, 10.0)
    if name.startswith("gate_edge"):
        # one hypothesis per segment (camera 0, candidate 0) and, per group g = (which depth, side), 17 witnesses of camera g + 1 whose depth is
        # d * (1 +- spatial_k) moved by k units in the last place, k = -8 .. 8.  A witness's target is the hypothesis' own projection moved sideways
        # by 1.5 .. 2.5 pixels, the less the nearer to (or the further beyond) the gate's edge: the outermost witness the gate admits holds its camera's
        # maximum, so ONE dropped or added witness changes the hypothesis' confidence by about 0.01.  Long source segments and sigma_a = 20 keep the
        # angle term above the distance term.
        sk = F32(kw["spatial_k"])
        scene = _Scene(8)
        src = _src_segments(rng, GATE_HYP, long=True)
        segs = []
        for s in range(GATE_HYP):
            d1, d2 = F32(rng.uniform(2.5, 5.5)), F32(rng.uniform(2.5, 5.5))
            cam, w1, w2, rank = [0], [d1], [d2], [0.0]
            for g, (which, side) in enumerate(GATE_GROUPS):
                for k in GATE_KS:
                    e1 = bump(F32(np.float64(d1) * (1.0 + side * np.float64(sk))), k) if which in ("first", "both") else d1
                    e2 = bump(F32(np.float64(d2) * (1.0 + side * np.float64(sk))), k) if which in ("second", "both") else d2
                    cam.append(g + 1); w1.append(e1); w2.append(e2)
                    rank.append(float(8 + side * k))                           # 0: deepest inside the gate ... 16: furthest beyond
            m = len(cam)
            cam, w1, w2 = np.array(cam), np.array(w1, F32), np.array(w2, F32)
            q0 = scene.targets(src[s], cam, np.full(m, d1), np.full(m, d2), np.zeros((m, 4)))       # the hypothesis' own projection into every witness's camera
            nrm = np.stack([-(q0[:, 3] - q0[:, 1]), q0[:, 2] - q0[:, 0]], 1)
            nrm /= np.linalg.norm(nrm, axis=1)[:, None]
            side_px = (2.5 - np.array(rank) / 16.0)[:, None] * nrm
            segs.append(dict(cam=cam, d1=w1, d2=w2, q=q0 + np.concatenate([side_px, side_px], 1)))
        return _pack(scene, src, segs, sk, 2.5, 20.0)
    if name == "bucket_edge":
        # first depths at the two ends of the depth buckets around the cluster: (b << 15) + {0, 1, 0x7ffe, 0x7fff}; the last pattern of bucket b and the
        # first of b + 1 are one unit in the last place apart, in different cameras
        N = 5
        scene = _Scene(N)
        src = _src_segments(rng, 2)
        segs = []
        for s, base in enumerate(((3.7, 4.1), (2.0, 5.0))):          # (2.0: an octave boundary -- the buckets double their width there)
            g = _mixed(rng, scene, src[s], 200, base=base)
            b0 = int(np.array(base[0], F32).view(np.int32)) >> BUCKET_SHIFT
            bits = np.array([((b0 + db) << BUCKET_SHIFT) + pat for db in range(-6, 7) for pat in (0, 1, 0x7ffe, 0x7fff)], np.int32)
            d1 = bits.view(F32)
            cam = np.arange(len(bits)) % N
            d2 = (base[1] * (1.0 + rng.normal(0, 0.003, len(bits)))).astype(F32)
            segs.append(_join(g, dict(cam=cam, d1=d1, d2=d2, q=scene.targets(src[s], cam, d1, d2, rng.normal(0, 0.7, (len(bits), 4))))))
        return _pack(scene, src, segs, 0.02, 2.5, 10.0)
    if name == "octaves":
        N = 5
        scene = _Scene(N)
        src = _src_segments(rng, 3)
        a = _mixed(rng, scene, src[0], 420, base=(3.5, 4.0), cluster=0.9)
        far = rng.random(420) < 1.0 / 3.0
        a["d1"] = np.where(far, a["d1"] * 2.0 ** rng.uniform(-7, 7, 420), a["d1"]).astype(F32)
        a["q"] = scene.targets(src[0], a["cam"], a["d1"], a["d2"], rng.normal(0, 1.0, (420, 4)))
        b = _mixed(rng, scene, src[1], 120, cluster=0.9)
        b["d1"][17] = F32(1e-30)                                               # the segment's bucket base drops to about 0: every other depth clamps into the last bucket
        one = dict(cam=np.array([2]), d1=np.array([1e-30], F32), d2=np.array([3.0], F32), q=np.array([[100.0, 100.0, 160.0, 130.0]]))
        return _pack(scene, src, [a, b, one], 0.02, 2.5, 10.0)
    if name == "far_origin":
        return make_case(1, spatial_k=0.005, behind=False, shift=(5000.0, -3000.0, 2000.0))
    if name == "ties":
        # a candidate and its copy TIES_APART places later in the list (same camera, target, depths), with witnesses of the three other cameras made for
        # them: the copies hold the segment's largest confidence.  One more copied pair, next to each other, with an ordinary confidence.
        # (What this case can show: equal confidences for equal candidates wherever they sit, and an epilogue that copes with two equal maxima.  It
        # cannot show WHICH copy won -- their depths are the same --, and the split walk cuts its units out of the bucket order, where copies are
        # neighbours, not out of the list order.  ties_flat below is the case in which the winner shows.)
        N, m = 4, 1500
        scene = _Scene(N)
        src = _src_segments(rng, 2)
        base = (3.9, 4.3)
        cam = np.repeat([0, 1, 2, 3], [200, 900, 200, 200])                    # (the list is in camera order: camera 1's run holds both copies)
        inl = rng.random(m) < 0.7
        d1 = (base[0] * (1.0 + np.where(inl, rng.normal(0, 0.004, m), rng.normal(0, 0.2, m)))).astype(F32)
        d2 = (base[1] * (1.0 + np.where(inl, rng.normal(0, 0.004, m), rng.normal(0, 0.2, m)))).astype(F32)
        off = rng.uniform(0.5, 1.5, (m, 4)) * rng.choice([-1.0, 1.0], (m, 4))  # (no ordinary candidate matches anything to better than half a pixel)
        q = scene.targets(src[0], cam, np.maximum(d1, 0.05), np.maximum(d2, 0.05), off)
        d1, d2 = np.maximum(d1, F32(0.05)), np.maximum(d2, F32(0.05))
        i, j = TIES_AT, TIES_AT + TIES_APART
        d1[i], d2[i] = base[0], base[1]
        q[i] = scene.targets(src[0], [1], [d1[i]], [d2[i]], [[1.0, -1.0, 1.0, -1.0]])[0]
        for k, c in ((40, 0), (1150, 2), (1350, 3)):                           # their witnesses: the same depths, the exact projections
            d1[k], d2[k] = d1[i], d2[i]
            q[k] = scene.targets(src[0], [c], [d1[i]], [d2[i]], [[0.0, 0.0, 0.0, 0.0]])[0]
        d1[j], d2[j], q[j] = d1[i], d2[i], q[i]
        d1[601], d2[601], q[601] = d1[600], d2[600], q[600]
        a = dict(cam=cam, d1=d1, d2=d2, q=q)
        a_tid_same = (i, j, 600, 601)
        case = _pack(scene, src, [a, _mixed(rng, scene, src[1], 80)], 0.02, 2.5, 10.0)
        for x, y in ((a_tid_same[0], a_tid_same[1]), (a_tid_same[2], a_tid_same[3])):     # same target: the copy points at the first one's 2-D segment
            case["matches_data"][y, 2] = case["matches_data"][x, 2]
        return case
    if name == "ties_flat":
        # sigma_p = sigma_a = 10^4: exp(-x) rounds to 1.0f for every witness within pixels and degrees, so a confidence is the NUMBER of supporting
        # cameras and hundreds of candidates with different depths tie at the segment's maximum -- the first of them in list order is the best
        # hypothesis, in every workgroup, unit and lane order
        scene = _Scene(4)
        src = _src_segments(rng, 3)
        return _pack(scene, src, [_mixed(rng, scene, src[0], 1500, cluster=0.8, noise=0.3), _mixed(rng, scene, src[1], 700, cluster=0.8, noise=0.3),
                                  _mixed(rng, scene, src[2], 50, noise=0.3)], 0.02, 1e4, 1e4)
    if name.startswith("many_cameras"):
        scene = _Scene(int(kw["N"]))
        ms = [3000] + [int(v) for v in rng.integers(0, 60, 30)]
        order = rng.permutation(len(ms))
        src = _src_segments(rng, len(ms))
        return _pack(scene, src, [_mixed(rng, scene, src[s], ms[order[s]]) for s in range(len(ms))], 0.02, 2.5, 10.0)
    if name == "long_runs":
        # (segment, camera) runs at and around the 256 entries a wave orders in registers and the 512 of two staged passes -- what the window kernel has
        # to order itself when the rows hold reverse matches (RUN_SIZES: per segment, candidates per camera)
        scene = _Scene(5)
        src = _src_segments(rng, len(RUN_SIZES))
        segs = []
        for s, per_cam in enumerate(RUN_SIZES):
            cam = np.repeat(np.arange(5), per_cam)
            g = _mixed(rng, scene, src[s], len(cam), cluster=0.7)
            g["cam"] = cam
            g["q"] = scene.targets(src[s], cam, g["d1"], g["d2"], rng.normal(0, 1.0, (len(cam), 4)))
            segs.append(g)
        return _pack(scene, src, segs, 0.02, 2.5, 10.0)
    raise KeyError(name)


RUN_SIZES = ((50, 300, 20, 600, 0), (0, 256, 7, 257, 3), (10, 513, 0, 2, 1), (9, 1, 12, 0, 8))
# lists for the ordering of unordered runs (no reference vector of their own: held to the contract oracle and to their ordered twin)
EXIST_CASES = [dict(name="long_runs")]


def shuffle_rows(row_start, meta, depths, N, cams, seed):
    """the entries of every row of the cameras `cams` in a seeded random order (metadata and depths together), everything else in place"""
    rng = np.random.default_rng(seed)
    perm = np.arange(len(meta))
    for row in range(len(row_start) - 1):
        if row % N in cams:
            a, b = int(row_start[row]), int(row_start[row + 1])
            perm[a:b] = a + rng.permutation(b - a)
    return meta[perm].copy(), depths[perm].copy(), perm


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31 - 1)


EDGE_CASES = [dict(name="sizes"), dict(name="one_camera"), dict(name="dense_cluster"),
              dict(name="gate_edge_0.005", spatial_k=0.005), dict(name="gate_edge_0.02", spatial_k=0.02), dict(name="gate_edge_0.05", spatial_k=0.05),
              dict(name="bucket_edge"), dict(name="octaves"), dict(name="far_origin"), dict(name="ties"), dict(name="ties_flat"),
              dict(name="many_cameras_17", N=17), dict(name="many_cameras_24", N=24), dict(name="no_gate")]
