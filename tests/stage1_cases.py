"""Crafted segment sets for stage 1 of the matcher (k_pair_mask, k_row_count, k_scan, k_tgt_rays, k_pair_fill): one source view and its neighbour
cameras, sized and shaped so that every launch path and every shape-dependent branch of those kernels is taken -- tile, wave and word ends, rows
of 64 / 65 / 128 / 129+ bits and candidates, a neighbour with more than 4096 and one with exactly 16384 segments, more than 4096 rows, 96 and 97
cameras, a subset of the cameras, epipoles inside the image, pairs at the decision points of the interval bounds, degenerate segments and tables.
tests/test_stage1_cases_cpu.py asserts that each case is what its name claims; tests/test_gpu_stage1_paths.py runs every launch path on them.

The cameras are tests/verify_cases.py::make_case's (look-at poses on a circle, K with f = 1500); F = K^-T [t]x R K^-1 is formed in double and cast
to float32 as the library's callers do.  Most targets come from adversarial_pairs.craft_targets, which builds them from the sources' epipolar
lines, so many pairs pass the overlap test.  A case is a dict of the arguments of Context.test_pair_candidates plus `seg_range` (None: all).

expected(case): per row (segment * N + camera) the number of pairs that pass the overlap test (`upper`), the candidates (four positive depths) in
ascending target order with their depths -- from the contract oracle's dense buffers (l3d_oracle_pipeline.pairwise_dense).
Test infrastructure; no reference code involved."""
import numpy as np

import adversarial_pairs as ap

F32 = np.float32
W, H = 1920, 1080
K = np.array([[1500.0, 0, 960.0], [0, 1500.0, 540.0], [0, 0, 1.0]])
C_SRC = (4.0, 0.2, 0.1)


def look_at(C, T=(0.0, 0.0, 0.0)):
    z = np.asarray(T, float) - np.asarray(C, float)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def circle_centers(N):
    """make_case's neighbour centres; beyond a dozen the circle is walked again at other heights (no two cameras coincide)"""
    out = []
    for c in range(N):
        k, lap = c % 12, c // 12
        th = 0.25 * (k + 1) * (1 if k % 2 else -1) + 0.021 * lap
        out.append((4.0 * np.cos(th), 0.3 * k - 0.5 + 0.37 * lap, 4.0 * np.sin(th)))
    return out


def rig(centers, targets=None, src=C_SRC, src_target=(0.0, 0.0, 0.0)):
    """float32 tables of a source camera and its neighbours (+ the double fundamental matrices the targets are crafted from)"""
    N = len(centers)
    Ki = np.linalg.inv(K)
    Rs, Cs = look_at(src, src_target), np.asarray(src, float)
    ts = -Rs @ Cs
    F = np.zeros((N, 3, 3)); RtKinv = np.zeros((N, 3, 3), F32); cen = np.zeros((N, 3), F32)
    for c in range(N):
        Cc = np.asarray(centers[c], float)
        same = np.allclose(Cc, Cs)
        Rc = Rs if same else look_at(Cc, (0.0, 0.0, 0.0) if targets is None else targets[c])
        R = Rc @ Rs.T
        t = -Rc @ Cc - R @ ts
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        F[c] = 0.0 if same else Ki.T @ tx @ R @ Ki                           # (no baseline: the fundamental matrix is zero)
        RtKinv[c] = (Rc.T @ Ki).astype(F32)
        cen[c] = Cc.astype(F32)
    return dict(F64=F, F=F.astype(F32), RtKinv=RtKinv, centers=cen, RtKinv_src=(Rs.T @ Ki).astype(F32), C_src=Cs.astype(F32))


def random_segments(rng, n, sigma=60.0):
    s = np.empty((n, 4), F32)
    s[:, 0:2] = (rng.random((n, 2)) * [1600, 900] + [150, 90]).astype(F32)
    s[:, 2:4] = s[:, 0:2] + rng.normal(0, sigma, (n, 2)).astype(F32)
    return s


def crafted(rng, F, src, n, per_source=4):
    """n targets of one camera: craft_targets from sources drawn in turn, filled up with random segments; the kinds' labels beside them"""
    if n == 0:
        return np.zeros((0, 4), F32), []
    want = max(1, (n * 3 // 4) // per_source)
    pick = src[rng.permutation(len(src))[:min(want, len(src))]]
    tg, kinds = ap.craft_targets(F, pick, W, H, rng, per_source)
    tg, kinds = tg[:n], list(kinds[:n])
    if len(tg) < n:
        tg = np.concatenate([tg.reshape(-1, 4), random_segments(rng, n - len(tg))])
        kinds += ["random"] * (n - len(kinds))
    order = rng.permutation(n)                                          # (crafted and random ones mixed: both kinds at the ends of the tiles)
    return np.ascontiguousarray(tg[order], F32), [kinds[i] for i in order]


def assemble(name, r, src, per_cam, tbm=None, seg_range=None, kinds=None, **extra):
    N = len(per_cam)
    offsets = np.zeros((N, 2), np.int32)
    o = 0
    for c, t in enumerate(per_cam):
        offsets[c] = (o, len(t))
        o += len(t)
    tgt = np.concatenate([np.asarray(t, F32).reshape(-1, 4) for t in per_cam]) if o else np.zeros((0, 4), F32)
    case = dict(name=name, src_segs=np.ascontiguousarray(src, F32), tgt_segs=np.ascontiguousarray(tgt, F32), offsets=offsets, F=r["F"], RtKinv=r["RtKinv"],
                centers=r["centers"], RtKinv_src=r["RtKinv_src"], C_src=r["C_src"], tbm=np.arange(N, dtype=np.int32) if tbm is None else np.asarray(tbm, np.int32),
                seg_range=seg_range, kinds=kinds, F64=r["F64"])
    case.update(extra)
    return case


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
# camera -> one of its targets that is some source's candidate: copied to the camera's last place, so that the last word / wave / tile holds one
TILES_LAST = {1: 0, 2: 0, 3: 1, 4: 1, 6: 0, 7: 1, 8: 1, 9: 1}


def case_tiles(last=None):
    """10 cameras with 0, 1, 63, 64, 65, 0, 255, 256, 257 and 513 segments (an empty one in the middle too): tile, wave and word ends, the exit of a
    tile beyond a camera's segments (the grid is sized by the widest camera)"""
    rng = np.random.default_rng(101)
    widths = [0, 1, 63, 64, 65, 0, 255, 256, 257, 513]
    r = rig(circle_centers(len(widths)))
    src = random_segments(rng, 70)
    per_cam = [crafted(rng, r["F64"][c], src, w)[0] for c, w in enumerate(widths)]
    for c, j in (TILES_LAST if last is None else last).items():
        per_cam[c][-1] = per_cam[c][j]
    return assemble("tiles", r, src, per_cam)


# (camera, index into its crafted targets, exact copies): each of these targets pairs with one source only, so its copies lengthen that one row --
# to 64, 65 and 128 set bits, or candidates (found by a search over the oracle's buffers; tests/test_stage1_cases_cpu.py checks the outcome)
DENSE_COPIES = [(0, 28, 60), (0, 48, 60), (0, 58, 125), (0, 64, 51), (1, 9, 52), (1, 40, 124), (1, 51, 109), (1, 53, 122), (2, 0, 61), (2, 3, 59)]


def case_dense_rows(copies=None):
    """3 cameras, 101 sources: copies of crafted targets, jittered by a pixel, make rows of far more than 129 set bits and candidates; exact copies of
    targets that pair with a single source bring rows to exactly 64, 65 and 128"""
    rng = np.random.default_rng(202)
    r = rig(circle_centers(3))
    src = random_segments(rng, 101)
    per_cam = []
    for c in range(3):
        base, _ = crafted(rng, r["F64"][c], src, 500, per_source=8)
        parts = [base]
        for k, n in enumerate((190, 90, 30)):
            parts.append((base[11 * k + c][None, :] + rng.normal(0, 1.0, (n, 4))).astype(F32))
        parts += [np.repeat(base[i][None, :], n, axis=0) for cam, i, n in (DENSE_COPIES if copies is None else copies) if cam == c]
        t = np.concatenate(parts)
        per_cam.append(t[np.random.default_rng(203 + c).permutation(len(t))])
    return assemble("dense_rows", r, src, per_cam)


WIDE_TAIL = {0: [1, 15, 18], 1: [2, 4, 5]}


def case_wide(tail_from=None):
    """9 sources, a camera with 4100 segments (the second 64-word chunk of k_pair_fill's prefix) and one with exactly 16384 (kMaxW64); crafted targets
    at both ends of both arrays"""
    rng = np.random.default_rng(303)
    r = rig(circle_centers(2))
    src = random_segments(rng, 9)
    per_cam = []
    for c, n in enumerate((4100, 16384)):
        t = random_segments(rng, n)
        head, _ = crafted(rng, r["F64"][c], src, 96, per_source=16)
        tail, _ = crafted(rng, r["F64"][c], src, 96, per_source=16)
        mid, _ = crafted(rng, r["F64"][c], src, 64, per_source=16)
        t[:96], t[n - 96:] = head, tail
        t[4064:4128 if n > 4128 else 4064 + 36] = mid[:64 if n > 4128 else 36]
        for i, j in enumerate(WIDE_TAIL.get(c, ()) if tail_from is None else tail_from.get(c, ())):
            t[n - 1 - i] = head[j]                                       # (some source's candidate at the very end: the last word of the second chunk)
        per_cam.append(t)
    return assemble("wide", r, src, per_cam)


def case_many_rows():
    """600 sources x 7 cameras = 4200 rows: two scan tiles, 17 row blocks; segments [37, 411) leave the range's pointers 259 ints off 16-byte alignment
    and end inside a tile.  The sources 200..299 sit in a corner no target's lines reach: row blocks without a candidate."""
    rng = np.random.default_rng(404)
    r = rig(circle_centers(7))
    src = random_segments(rng, 600)
    live = np.r_[0:200, 300:600]
    per_cam = [crafted(rng, r["F64"][c], src[live], 40, per_source=1)[0] for c in range(7)]
    src[200:300, 0:2] = (rng.random((100, 2)) * 3.0 + [40000.0, 40000.0]).astype(F32)      # far outside every image: nothing overlaps
    src[200:300, 2:4] = src[200:300, 0:2] + rng.normal(0, 1.0, (100, 2)).astype(F32)
    return assemble("many_rows", r, src, per_cam, seg_range=(37, 411))


def _case_cams(N, seed):
    rng = np.random.default_rng(seed)
    r = rig(circle_centers(N))
    src = random_segments(rng, 130)
    return assemble("cams_%d" % N, r, src, [crafted(rng, r["F64"][c], src, 3 + c % 3, per_source=1)[0] for c in range(N)], spb=64, seg_range=(1, 130))


def case_cams_96():
    """96 cameras, 3-5 targets each, 130 sources: with 64 sources per workgroup (`spb`: the *_spb64 variants; the launcher's rule gives 16) the rows
    lie 96 apart and span 24 row blocks, 25 over the range [1, 130) -- the LDS table has 26"""
    return _case_cams(96, 505)


def case_cams_97():
    """97 cameras: past the fused row starts (the seam call and the chains' scan launch only)"""
    return _case_cams(97, 506)


def case_subset():
    """6 cameras of which 1, 2 and 4 are matched"""
    rng = np.random.default_rng(607)
    r = rig(circle_centers(6))
    src = random_segments(rng, 90)
    return assemble("subset", r, src, [crafted(rng, r["F64"][c], src, 150 + 20 * c)[0] for c in range(6)], tbm=[1, 2, 4])


FACING_CENTERS = [(0, 0, -4), (0.3, 0.1, 4), (-0.4, 0.2, 4.2), (0.1, 0.05, -3.0), (0.0, -0.1, -5.0), (4, 0.2, 0.3), (0.5, 0.3, -4.1)]


def case_facing():
    """neighbours that face the source camera or lie ahead of it on its axis (the poses of test_pair_pretest_wrapping_epipolar_transfer): the epipole
    falls inside the image, the epipolar transfer of a source segment wraps through infinity and e_d = e1 - e2 crosses target tiles"""
    rng = np.random.default_rng(708)
    r = rig(FACING_CENTERS[1:], src=FACING_CENTERS[0])
    src = random_segments(rng, 150)
    # (segments that pass close to the epipoles -- near the image centre -- make the wrapped pairs)
    src[:70, 0:2] = (rng.normal(0, 120, (70, 2)) + [960, 540]).astype(F32)
    src[:70, 2:4] = src[:70, 0:2] + rng.normal(0, 150, (70, 2)).astype(F32)
    per_cam = []
    for c in range(len(FACING_CENTERS) - 1):
        t, _ = crafted(rng, r["F64"][c], src, 150, per_source=4)
        t[:60, 0:2] = (rng.normal(0, 120, (60, 2)) + [960, 540]).astype(F32)
        t[:60, 2:4] = t[:60, 0:2] + rng.normal(0, 150, (60, 2)).astype(F32)
        per_cam.append(t)
    return assemble("facing", r, src, per_cam)


def case_adversarial():
    """craft_targets with all four families, 16 per source, 120 sources: intersection points at segment ends, overlap ratios at the thresholds, tiny and
    image-spanning targets"""
    rng = np.random.default_rng(809)
    r = rig(circle_centers(2))
    src = random_segments(rng, 120)
    per_cam, kinds, owner = [], [], []
    for c in range(2):
        t, k, o = [], [], []
        for y in range(len(src)):                                       # (source by source: a target's own source is known)
            ty, ky = ap.craft_targets(r["F64"][c], src[y:y + 1], W, H, rng, 16)
            t.append(ty.reshape(-1, 4)); k += ky; o += [y] * len(ky)
        per_cam.append(np.concatenate(t)); kinds.append(k); owner.append(np.array(o))
    return assemble("adversarial", r, src, per_cam, kinds=kinds, owner=owner)


def case_degenerate():
    """ordinary sets plus zero-length and sub-pixel segments on both sides, a tile of targets beyond 32768 pixels (level 2 is off by its extent guard)
    and a neighbour at the source's own centre (F is all zeros): whatever the oracle says is the answer"""
    rng = np.random.default_rng(910)
    cen = circle_centers(3) + [C_SRC]
    r = rig(cen)
    assert not r["F"][3].any()
    src = random_segments(rng, 83)
    src[5, 2:4] = src[5, 0:2]                                            # zero length
    src[6, 2:4] = src[6, 0:2] + F32(0.25)                                # sub-pixel
    src[7] = np.nextafter(src[8], F32(np.inf))                           # an ulp off its neighbour
    src[9, 2:4] = src[9, 0:2] + F32(1e-3)
    per_cam = []
    for c in range(4):
        t, _ = crafted(rng, r["F64"][min(c, 2)], src, 300 if c == 1 else 120)
        wild = np.abs(t).max(axis=1) > 30000.0                           # (image-spanning crafted targets: only the far tile leaves the validated range)
        t[wild] = random_segments(rng, int(wild.sum()))
        t[3, 2:4] = t[3, 0:2]
        t[4, 2:4] = t[4, 0:2] + F32(0.5)
        t[10, 2:4] = t[10, 0:2] + F32(1e-3)
        if c == 1:      # the second tile of 256: far coordinates, among them long segments that still cross the image
            far, _ = crafted(rng, r["F64"][1], src, 44, per_source=4)
            far[:, 0:2] += (far[:, 0:2] - far[:, 2:4]) * F32(300.0)
            far[::2, 2:4] += F32(40000.0)
            t[256:300] = far
        per_cam.append(t)
    return assemble("degenerate", r, src, per_cam, empty_cams=(3,))


CASES = {f.__name__[5:]: f for f in (case_tiles, case_dense_rows, case_wide, case_many_rows, case_cams_96, case_cams_97, case_subset, case_facing,
                                     case_adversarial, case_degenerate)}
_cases, _expected = {}, {}


def get_case(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


# ---- expected values -------------------------------------------------------------------------------------------------------------------------
def dense_buffers(case, lib):
    """camera of to_be_matched -> the oracle's S x width x 4 depth buffer"""
    import l3d_oracle_pipeline as op
    return {int(cam): op.pairwise_dense(lib, case["src_segs"], case["RtKinv_src"], case["C_src"], case["tgt_segs"], int(case["offsets"][cam][0]),
                                        int(case["offsets"][cam][1]), int(cam), case["F"], case["RtKinv"], case["centers"]) for cam in case["tbm"]}


def expected(case, lib=None, seg_range="case"):
    """dict: upper, count (S*N,) int32 | rows: row -> (targets ascending, depths (n, 4)) | passed, kept: camera -> S x width bool.  seg_range: the
    case's own ("case"), None (all) or (begin, end); rows outside it and of unmatched cameras expect nothing.  Made once per (case, range)."""
    import l3d_oracle_pipeline as op
    rng_ = case["seg_range"] if seg_range == "case" else seg_range
    key = (case["name"], rng_)
    if key in _expected:
        return _expected[key]
    dk = (case["name"], "dense")
    if dk not in _expected:
        _expected[dk] = dense_buffers(case, lib or op.load_lib(libm=False))
    S, N = len(case["src_segs"]), len(case["offsets"])
    s0, s1 = (0, S) if rng_ is None else rng_
    upper, count, rows, passed, kept = np.zeros((S, N), np.int32), np.zeros((S, N), np.int32), {}, {}, {}
    for cam, buf in _expected[dk].items():
        p, k = (buf != 0).any(axis=2), (buf > 0).all(axis=2)
        assert not (k & ~p).any()
        passed[cam], kept[cam] = p, k
        upper[s0:s1, cam], count[s0:s1, cam] = p[s0:s1].sum(1), k[s0:s1].sum(1)
        for y in range(s0, s1):
            x = np.flatnonzero(k[y])
            if len(x):
                rows[y * N + cam] = (x.astype(np.uint32), buf[y, x])
    _expected[key] = dict(upper=upper.reshape(-1), count=count.reshape(-1), rows=rows, passed=passed, kept=kept, range=(s0, s1))
    return _expected[key]


# ---- launch_pair_mask's rule for the source segments per workgroup (l3d_kernels.hip: pair_mask_src_per_block) ----------------------------------------
def src_per_block(n_src, max_w, n_tbm, forced=0):
    if forced > 0:
        return min(forced, 64)
    tiles, spb = (max_w + 255) // 256, 64
    while spb > 8 and tiles * ((n_src + spb - 1) // spb) * n_tbm < 768:
        spb //= 2
    return spb


def case_spb(case, forced=0, seg_range="case"):
    rng_ = case["seg_range"] if seg_range == "case" else seg_range
    s0, s1 = (0, len(case["src_segs"])) if rng_ is None else rng_
    return src_per_block(s1 - s0, int(case["offsets"][case["tbm"], 1].max()), len(case["tbm"]), forced)
