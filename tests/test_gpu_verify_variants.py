"""Stage 2 (K_verify_matches) on crafted candidate lists, every kernel variant: the all-pairs kernel, the per-view seam call's launches and the
chains' single launch -- 4 and 8 waves, LDS images and scratch blocks, bucket starts in global memory, the split build + walk in units of 256 and
512, any segment order -- through l3d_test_verify_candidates, which runs the product's own set-up and launchers on a list of the test's.  Lists:
tests/verify_cases.py (CASES and EDGE_CASES; tests/test_verify_cases_cpu.py says what each is).  Reference: the contract oracle's
confidences, bit for bit, on every path; kept counts and best depths follow from them in numpy.  The reference's own kernel text
(tests/golden/verify_ref.npz, verify_edges_ref.npz) within 5e-6 and with the same kept set.  Which kernels ran is asserted from the hook's own
report, so a launcher that quietly takes another variant fails here."""
import os

import numpy as np
import pytest

import l3d_oracle_pipeline as op
import verify_cases as vc
from line3d_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

CASE_NAMES = ["seed_%d" % kw["seed"] for kw in vc.CASES] + [kw["name"] for kw in vc.EDGE_CASES]
_cache = {}


def get_case(name):
    """(case, rows, contract oracle's confidences, reference vector) -- made once per module"""
    if name not in _cache:
        if name.startswith("seed_"):
            k = [kw["seed"] for kw in vc.CASES].index(int(name[5:]))
            case = vc.make_case(**vc.CASES[k])
            ref = np.load(os.path.join(HERE, "golden", "verify_ref.npz"))["c%d_conf" % k]
        elif name in [kw["name"] for kw in vc.EXIST_CASES]:     # (no reference vector of its own)
            case, ref = vc.make_edge_case(name), None
        else:
            case = vc.make_edge_case(**[kw for kw in vc.EDGE_CASES if kw["name"] == name][0])
            ref = np.load(os.path.join(HERE, "golden", "verify_edges_ref.npz"))[name + "_conf"]
        _cache[name] = (case, vc.to_rows(case), op.verify_case(op.load_lib(libm=False), case), ref)
    return _cache[name]


W256, W512, WGB, BUILD, WALK, WALKGB = capi.VK_WINDOW_256, capi.VK_WINDOW_512, capi.VK_WINDOW_GB, capi.VK_BUILD, capi.VK_WALK, capi.VK_WALK_GB
# name -> (arguments of the hook, kernels expected (a function of N), applies to N).  wide_max = -1 stands for the number of segments.
VARIANTS = {
    "all_pairs": (dict(path=0), lambda N: capi.VK_ALL_PAIRS | capi.VK_SEG_POST, None),
    "seam": (dict(path=1), lambda N: W256 | capi.VK_SEG_POST, None),
    "seam_8wave": (dict(path=1, wide_max=-1), lambda N: W512 | capi.VK_SEG_POST, None),
    "seam_mmax64": (dict(path=1, mmax=64), lambda N: W256 | capi.VK_SEG_POST, None),
    "chain_4wave": (dict(path=2), lambda N: W256, None),
    "chain_8wave": (dict(path=2, wide_max=-1), lambda N: W512, None),
    "chain_mmax64": (dict(path=2, mmax=64), lambda N: W256, None),
    "chain_8wave_mmax64": (dict(path=2, mmax=64, wide_max=-1), lambda N: W512, None),
    "chain_gb": (dict(path=2, gb=1), lambda N: WGB, lambda N: N > 16),
    "chain_gb_mmax64": (dict(path=2, gb=1, mmax=64), lambda N: WGB, lambda N: N > 16),
    "chain_split256": (dict(path=2, split_unit=256, gb=-1), lambda N: BUILD | (WALKGB if N > 16 else WALK), None),
    "chain_split512": (dict(path=2, split_unit=512, gb=-1), lambda N: BUILD | (WALKGB if N > 16 else WALK), None),
    "chain_split256_mmax64": (dict(path=2, split_unit=256, gb=-1, mmax=64), lambda N: BUILD | (WALKGB if N > 16 else WALK), None),
    "chain_reversed": (dict(path=2, seg_order="reversed"), lambda N: W256, None),
    "chain_longest_first": (dict(path=2, seg_order="longest"), lambda N: W256, None),
}


def run_variant(ctx, name, variant):
    case, (row_start, meta), conf, ref = get_case(name)
    kw, kernels, _ = VARIANTS[variant]
    kw = dict(kw)
    S, N = len(case["match_offsets"]), len(case["camera_offsets"])
    m = case["match_offsets"][:, 1]
    if kw.get("wide_max") == -1:
        kw["wide_max"] = S
    if kw.get("gb") == -1:
        kw["gb"] = 1 if N > 16 else 0
    if kw.get("seg_order") == "reversed":
        kw["seg_order"] = np.arange(S)[::-1]
    elif kw.get("seg_order") == "longest":
        kw["seg_order"] = np.argsort(-m, kind="stable")
    got = ctx.test_verify_candidates(case["src_segs"], case["tgt_segs"], case["camera_offsets"], case["P"], case["RtKinv"], case["C_src"], row_start, meta,
                                     case["matches_depths"], case["sigma_p"], case["sigma_a"], case["spatial_k"], **kw)
    return case, conf, ref, got, kernels(N), kw


def expected_epilogue(case, conf):
    S = len(case["match_offsets"])
    kept, best = np.zeros(S, np.int32), np.full((S, 2), -1.0, np.float32)
    for s in range(S):
        a, m = (int(v) for v in case["match_offsets"][s])
        c = conf[a:a + m]
        kept[s] = int((c > 1.0).sum())
        if m and c.max() > 0.5:
            best[s] = case["matches_depths"][a + int(np.argmax(c)), :2]          # (argmax: the first of equal maxima)
    return kept, best


def check(case, conf, ref, got, kernels, kw, what):
    g_conf, g_kept, g_best, mmax_used, ran = got
    assert ran == kernels, (what, "kernels launched", ran, "expected", kernels)
    bad = np.flatnonzero(g_conf.view(np.uint32) != conf.view(np.uint32))
    assert len(bad) == 0, (what, "%d of %d confidences differ from the contract oracle, first at %d: %r against %r" % (len(bad), len(conf), bad[0], g_conf[bad[0]], conf[bad[0]]))
    kept, best = expected_epilogue(case, conf)
    assert np.array_equal(g_kept, kept), (what, "kept counts")
    assert g_best.tobytes() == best.tobytes(), (what, "best depths", np.flatnonzero((g_best != best).any(1))[:8])
    if ref is not None:
        assert np.max(np.abs(g_conf - ref), initial=0) <= 5e-6 and np.array_equal(g_conf > 1.0, ref > 1.0), (what, "reference vectors")
    if kw["path"] != 0:
        N, largest = len(case["camera_offsets"]), int(case["match_offsets"][:, 1].max())
        want = vc.vw_fit_mmax(kw["mmax"], N) if kw.get("mmax") else vc.vw_mmax(largest, N, kw["path"])
        assert mmax_used == want, (what, "image size", mmax_used, want)


CASE_N = dict([("seed_%d" % kw["seed"], kw.get("N", 5)) for kw in vc.CASES] + [(kw["name"], kw.get("N", 0)) for kw in vc.EDGE_CASES])     # (0: at most 16)
RUNS = [(name, variant) for name in CASE_NAMES for variant in VARIANTS if VARIANTS[variant][2] is None or VARIANTS[variant][2](CASE_N[name])]


@pytest.mark.parametrize("name,variant", RUNS)
def test_variant_equals_the_oracle(gpu_ctx, name, variant):
    case, conf, ref, got, kernels, kw = run_variant(gpu_ctx, name, variant)
    assert VARIANTS[variant][2] is None or len(case["camera_offsets"]) > 16
    check(case, conf, ref, got, kernels, kw, (name, variant))


def test_every_code_path_is_reached(gpu_ctx):
    """the sizes a variant's code paths hang on, from the image size the hook reports: LDS blocks and scratch blocks, the 2048 candidates kept in
    registers and the re-read beyond, units of the split walk"""
    case = get_case("sizes")[0]
    m = case["match_offsets"][:, 1]
    for variant, path in (("seam", 1), ("chain_4wave", 2), ("chain_8wave", 2), ("chain_split256", 2), ("chain_split512", 2)):
        mmax_used = run_variant(gpu_ctx, "sizes", variant)[3][3]
        assert mmax_used == vc.vw_mmax(3000, 5, path) and mmax_used in m and mmax_used + 1 in m, variant
        assert ((m > 0) & (m < mmax_used)).any() and (m > mmax_used + 1).any() and 2048 in m and 2049 in m and (m > 2049 + 512).any(), variant
    for name in ("gate_edge_0.005", "gate_edge_0.02", "gate_edge_0.05", "bucket_edge", "octaves", "ties", "ties_flat"):
        m = get_case(name)[0]["match_offsets"][:, 1]
        assert (m > 64).sum() >= 2, name                                     # under mmax = 64 the case's own segments take the scratch blocks and the walk
    for name, N in (("many_cameras_17", 17), ("many_cameras_24", 24)):
        case = get_case(name)[0]
        mmax_used = run_variant(gpu_ctx, name, "chain_gb")[3][3]
        m = case["match_offsets"][:, 1]
        assert mmax_used == vc.vw_mmax(3000, N, 2) and (m > mmax_used).any() and ((m > 0) & (m <= mmax_used)).any(), name


def _tables(name="seed_1"):
    case, (row_start, meta), conf, _ = get_case(name)
    return dict(src_segs=case["src_segs"], tgt_segs=case["tgt_segs"], offsets=case["camera_offsets"].copy(), P=case["P"], RtKinv_src=case["RtKinv"],
                C_src=case["C_src"], row_start=row_start.copy(), cand_meta=meta.copy(), cand_depths=case["matches_depths"], sigma_p=case["sigma_p"],
                sigma_a=case["sigma_a"], spatial_k=case["spatial_k"])


def _break(kind, t):
    N = len(t["offsets"])
    full = int(np.flatnonzero(np.diff(t["row_start"]) > 0)[3])               # a row that holds candidates
    if kind == "row_start descends":
        t["row_start"][full + 1] = t["row_start"][full] - 1
    elif kind == "row_start ends short of R":
        t["row_start"][-1] -= 1
    elif kind == "row_start ends past R":
        t["row_start"][-1] += 1
    elif kind == "row_start starts past 0":
        t["row_start"][0] = 1
    elif kind == "camera of another row":
        r = int(t["row_start"][full])
        t["cand_meta"][r, 1] = (t["cand_meta"][r, 1] + 1) % N
    elif kind == "camera past N":
        t["cand_meta"][int(t["row_start"][full]), 1] = N
    elif kind == "target past its camera":
        r = int(t["row_start"][full])
        t["cand_meta"][r, 0] = t["offsets"][t["cand_meta"][r, 1], 1]
    elif kind == "target far past its camera":
        t["cand_meta"][int(t["row_start"][full]), 0] = 0x7fffffff
    elif kind == "offsets past the targets":
        t["offsets"][N - 1, 1] += 1
    elif kind == "negative offset":
        t["offsets"][0, 0] = -1
    return t


BROKEN = ["row_start descends", "row_start ends short of R", "row_start ends past R", "row_start starts past 0", "camera of another row", "camera past N",
          "target past its camera", "target far past its camera", "offsets past the targets", "negative offset"]


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("kind", BROKEN)
def test_broken_tables_are_refused(gpu_ctx, kind, path):
    """a wrong table is a Python exception with the library's message, never a launch; the context then verifies a valid list as before"""
    t = _break(kind, _tables())
    with pytest.raises(capi.L3DError) as e:
        gpu_ctx.test_verify_candidates(path=path, **t)
    assert e.value.code == 1 and "verify_candidates" in str(e.value)
    variant = ("all_pairs", "seam", "chain_4wave")[path]
    check(*run_variant(gpu_ctx, "seed_1", variant)[:6], ("seed_1 after a refusal", variant))


def test_refused_sizes_and_selections(gpu_ctx):
    t = _tables()
    S, N = len(t["src_segs"]), len(t["offsets"])
    for bad in (dict(path=3), dict(path=-1), dict(path=2, split_unit=100), dict(path=2, gb=2), dict(path=2, mmax=-1), dict(path=1, wide_max=-1),
                dict(path=1, seg_order=np.arange(S)), dict(path=2, seg_order=np.zeros(S, np.int32)), dict(path=2, seg_order=np.arange(S) + 1)):
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.test_verify_candidates(**t, **bad)
        assert e.value.code == 1, bad
    # 2^24 candidates: a position inside a segment would no longer fit its 24 bits (the arrays are never read: the count is refused first)
    R = 1 << 24
    big = dict(t, row_start=np.concatenate([np.zeros(S * N, np.int32), [R]]).astype(np.int32), cand_meta=np.zeros((R, 2), np.uint32), cand_depths=np.zeros((R, 4), np.float32))
    with pytest.raises(capi.L3DError) as e:
        gpu_ctx.test_verify_candidates(path=2, **big)
    assert e.value.code == 1 and "2^24" in str(e.value)
    # 60 neighbours: the window kernels' per-lane maxima do not fit; the all-pairs kernel takes them
    N = 60
    wide = dict(src_segs=np.array([[100.0, 100.0, 300.0, 200.0]], np.float32), tgt_segs=np.zeros((0, 4), np.float32), offsets=np.zeros((N, 2), np.int32),
                P=np.zeros((N, 3, 4), np.float32), RtKinv_src=t["RtKinv_src"], C_src=t["C_src"], row_start=np.zeros(N + 1, np.int32),
                cand_meta=np.zeros((0, 2), np.uint32), cand_depths=np.zeros((0, 4), np.float32), sigma_p=2.5, sigma_a=10.0, spatial_k=0.02)
    for path in (1, 2):
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.test_verify_candidates(path=path, **wide)
        assert e.value.code == 1 and "neighbours" in str(e.value)
    conf, kept, best, _, ran = gpu_ctx.test_verify_candidates(path=0, **wide)
    assert len(conf) == 0 and kept.tolist() == [0] and best.tolist() == [[-1.0, -1.0]] and ran == capi.VK_ALL_PAIRS | capi.VK_SEG_POST
    check(*run_variant(gpu_ctx, "seed_1", "chain_4wave")[:6], ("seed_1 after the refusals", "chain_4wave"))


# ---- unordered reverse-match runs: the window kernel orders the rows of the cameras it is told hold reverse matches (k_verify_window, sort_exist_run)
EXIST_CAMS = {"seed_2": (1, 4, 6), "one_camera": (1, 2), "sizes": (0, 3), "many_cameras_17": (2, 9, 16), "long_runs": (1, 3)}
EXIST_VARIANTS = ("chain_4wave", "chain_8wave", "chain_mmax64", "chain_gb", "chain_split256", "chain_longest_first")
EXIST_RUNS = [(n, v) for n in EXIST_CAMS for v in EXIST_VARIANTS if VARIANTS[v][2] is None or VARIANTS[v][2](CASE_N.get(n, 5))]
_sorted_runs = set()


@pytest.mark.parametrize("name,variant", EXIST_RUNS)
def test_unordered_runs_are_ordered_by_the_window_kernel(gpu_ctx, name, variant):
    """The rows of the chosen cameras shuffled (fixed seed) and named as exist_cams: the candidate arrays come back in the unshuffled order, and
    confidences, kept counts and best depths are the unshuffled run's byte for byte -- which is held to the contract oracle."""
    case, (row_start, meta), conf, ref = get_case(name)
    cams = EXIST_CAMS[name]
    N = len(case["camera_offsets"])
    runs = []
    for row in range(len(row_start) - 1):        # (on the CPU: one right order per shuffled row)
        if row % N in cams:
            assert np.all(np.diff(meta[row_start[row]:row_start[row + 1], 0].astype(np.int64)) > 0), (name, row)
            runs.append(int(row_start[row + 1] - row_start[row]))
    assert max(runs) >= 2
    got0 = run_variant(gpu_ctx, name, variant)
    check(*got0[:6], (name, variant, "ordered"))
    kw = got0[5]
    meta_s, depths_s, perm = vc.shuffle_rows(row_start, meta, case["matches_depths"], N, cams, 11)
    assert (perm != np.arange(len(perm))).sum() >= 2
    got = gpu_ctx.test_verify_candidates(case["src_segs"], case["tgt_segs"], case["camera_offsets"], case["P"], case["RtKinv"], case["C_src"], row_start, meta_s,
                                         depths_s, case["sigma_p"], case["sigma_a"], case["spatial_k"], exist_cams=cams, **kw)
    assert got[4] == got0[4], "kernels launched"
    assert np.array_equal(got[5], meta), "the candidates' metadata did not come back in target order"
    assert got[6].tobytes() == case["matches_depths"].tobytes(), "the depths did not follow their candidates"
    for k, what in ((0, "confidences"), (1, "kept counts"), (2, "best depths")):
        assert got[k].tobytes() == got0[3][k].tobytes(), what
    assert got[3] == got0[3][3]
    _sorted_runs.update(runs)


def test_both_orderings_of_a_run_were_reached():
    """runs a wave ranks in registers (2 .. 256 entries) and runs it stages (above 256: two passes; above 512: three)"""
    assert len(_sorted_runs) > 0, "run with the tests above"
    assert any(2 <= r <= 64 for r in _sorted_runs) and any(64 < r <= 256 for r in _sorted_runs) and 256 in _sorted_runs and 257 in _sorted_runs
    assert any(256 < r <= 512 for r in _sorted_runs) and any(r > 512 for r in _sorted_runs)
