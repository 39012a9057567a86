"""Stage 1 of the matcher (k_pair_mask, k_row_count, k_scan, k_tgt_rays, k_pair_fill) on crafted segment sets, every launch sequence: the per-view
seam call, the resident chain with fused row starts and the chains with a scan launch -- every filter level, 8 and 64 source segments per workgroup,
with and without the viewing-ray tables, whole views and segment ranges -- through l3d_test_pair_candidates, which runs the product's own set-up and
launchers.  Sets: tests/stage1_cases.py (tests/test_stage1_cases_cpu.py says what each is).  Reference: the contract oracle's dense buffers -- the row
counts exactly, the candidates in ascending target order with their depths bit for bit, every slot and row no kernel should write still holding the
hook's fill.  The reference's own kernel (tests/golden/pairwise_ref.npz): the same candidate set and depths on every path."""
import os

import numpy as np
import pytest

import l3d_oracle_pipeline as op
import stage1_cases as sc
from line3d_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = np.uint32(0xffffffff)

# name -> arguments of the hook.  Path 1 (fused row starts) takes up to 96 cameras.
VARIANTS = {
    "seam": dict(path=0, pretest=3),
    "seam_exact": dict(path=0, pretest=0),
    "seam_wedge_only": dict(path=0, pretest=1),
    "seam_bounds_only": dict(path=0, pretest=2),
    "seam_spb64": dict(path=0, spb=64),
    "fused": dict(path=1, pretest=3),
    "fused_no_accept": dict(path=1, pretest=7),
    "fused_exact": dict(path=1, pretest=0),
    "fused_spb8": dict(path=1, spb=8),
    "fused_spb64": dict(path=1, spb=64),
    "fused_no_ray_tables": dict(path=1, ray_tables=0),
    "scan": dict(path=2),
    "scan_spb64": dict(path=2, spb=64),
    "scan_no_ray_tables": dict(path=2, ray_tables=0),
}
SLACK = 64          # slots past the result: they must keep the fill


def applies(variant, name):
    return VARIANTS[variant]["path"] != 1 or len(sc.get_case(name)["offsets"]) <= 96


def run(ctx, case, e, variant=None, **over):
    """the hook on a case over the range of the expectation `e`"""
    kw = dict(VARIANTS[variant] if variant else {}, **over)
    path = kw.get("path", 0)
    kw.setdefault("capacity", int((e["count"] if path == 0 else e["upper"]).sum()) + SLACK)
    out = ctx.test_pair_candidates(case["src_segs"], case["tgt_segs"], case["offsets"], case["F"], case["RtKinv"], case["centers"], case["RtKinv_src"],
                                   case["C_src"], case["tbm"], seg_range=e["range"], **kw)
    return out, kw


def expected_starts(case, e, path):
    """(row starts the candidates sit at, the row_start array the path leaves behind with -1 where it writes nothing)"""
    S, N = len(case["src_segs"]), len(case["offsets"])
    s0, s1 = e["range"]
    scanned = e["count"] if path == 0 else e["upper"]
    pref = np.concatenate([[0], np.cumsum(scanned)]).astype(np.int32)
    left = np.full(S * N + 1, -1, np.int32)
    if path == 0 or (path == 2 and (s0, s1) == (0, S)):
        left[:] = pref                                                  # a scan over all rows
    elif path == 2:
        if s1 > s0:
            left[s0 * N:s1 * N + 1] = pref[s0 * N:s1 * N + 1]           # a scan over the range's rows, the total at the end
            left[S * N] = pref[S * N]
    else:
        w = np.flatnonzero(e["upper"] > 0)                              # k_pair_fill writes the start of a row that has bits
        left[w] = pref[w]
    return pref, left


def check(case, e, out, kw, what):
    path = kw.get("path", 0)
    S, N = len(case["src_segs"]), len(case["offsets"])
    s0, s1 = e["range"]
    upper, count = e["upper"], e["count"]
    assert out["spb_used"] == sc.src_per_block(s1 - s0, int(case["offsets"][case["tbm"], 1].max()), len(case["tbm"]), kw.get("spb", 0)), (what, "spb", out["spb_used"])
    bad = np.flatnonzero(out["row_upper"] != (count if path == 0 else upper))
    assert len(bad) == 0, (what, "row_upper: %d rows differ, first (segment %d, camera %d): %d, expected %d"
                           % (len(bad), bad[0] // N, bad[0] % N, out["row_upper"][bad[0]], (count if path == 0 else upper)[bad[0]]))
    bad = np.flatnonzero(out["row_count"] != count)
    assert len(bad) == 0, (what, "row_count: %d rows differ, first (segment %d, camera %d): %d, expected %d" % (len(bad), bad[0] // N, bad[0] % N, out["row_count"][bad[0]], count[bad[0]]))
    pref, left = expected_starts(case, e, path)
    bad = np.flatnonzero(out["row_start"] != left)
    assert len(bad) == 0, (what, "row_start: %d entries differ, first %d: %d, expected %d" % (len(bad), bad[0], out["row_start"][bad[0]], left[bad[0]]))
    scanned = (count if path == 0 else upper).reshape(S, N)
    assert (out["total"], out["largest"]) == ((-1, -1) if path == 1 or (path == 2 and s1 == s0) else (int(scanned.sum()), int(scanned.sum(1).max(initial=0)))), (what, "statistics", out["total"], out["largest"])
    assert out["overflow"] == 0 and out["needed"] == int(scanned.sum()), (what, out["overflow"], out["needed"])
    cap = len(out["cand_meta"])
    meta, depths = np.full((cap, 2), FILL, np.uint32), np.full((cap, 4), FILL, np.uint32)
    for row, (x, d) in e["rows"].items():
        a = int(pref[row])
        meta[a:a + len(x), 0], meta[a:a + len(x), 1] = x, row % N
        depths[a:a + len(x)] = d.view(np.uint32)
    bad = np.flatnonzero((out["cand_meta"] != meta).any(1))
    assert len(bad) == 0, (what, "candidates: %d slots differ, first %d: (target, camera) %r, expected %r" % (len(bad), bad[0], out["cand_meta"][bad[0]].tolist(), meta[bad[0]].tolist()))
    got = out["cand_depths"].view(np.uint32)
    bad = np.flatnonzero((got != depths).any(1))
    assert len(bad) == 0, (what, "depths: %d slots differ from the oracle's bits, first %d (target %d, camera %d): %r, expected %r"
                           % (len(bad), bad[0], meta[bad[0], 0], meta[bad[0], 1], out["cand_depths"][bad[0]].tolist(), depths[bad[0]].view(np.float32).tolist()))


def ranges(name):
    case = sc.get_case(name)
    return [None] + ([case["seg_range"]] if case["seg_range"] else [])


RUNS = [(name, variant, rng) for name in sc.CASES for variant in VARIANTS if applies(variant, name) for rng in ranges(name)]


@pytest.mark.parametrize("name,variant,seg_range", RUNS, ids=["%s-%s-%s" % (n, v, "all" if r is None else "%d_%d" % r) for n, v, r in RUNS])
def test_variant_equals_the_oracle(gpu_ctx, name, variant, seg_range):
    case = sc.get_case(name)
    e = sc.expected(case, seg_range=seg_range)
    out, kw = run(gpu_ctx, case, e, variant)
    check(case, e, out, kw, (name, variant, seg_range))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_variants_of_a_path_agree(gpu_ctx, name):
    """all variants of one launch sequence leave the same bytes: a difference names the filter level or the workgroup shape that caused it"""
    case = sc.get_case(name)
    e = sc.expected(case, seg_range=None)
    first = {}
    for variant in VARIANTS:
        if not applies(variant, name):
            continue
        out, kw = run(gpu_ctx, case, e, variant)
        blob = {k: out[k].tobytes() for k in ("row_upper", "row_count", "row_start", "cand_meta", "cand_depths")}
        ref_variant, ref = first.setdefault(kw["path"], (variant, blob))
        for k in blob:
            assert blob[k] == ref[k], (name, "%s differs between %s and %s" % (k, variant, ref_variant))
    assert set(first) == ({0, 1, 2} if len(case["offsets"]) <= 96 else {0, 2})


@pytest.mark.parametrize("path", [1, 2])
def test_candidate_overflow(gpu_ctx, path):
    """the chains' capacity guard: room for exactly the upper bounds gives the whole result; one slot less reports the overflow, writes no candidate
    and leaves the upper bounds in the row counts -- what the chains' restart sizes the next attempt from"""
    case = sc.get_case("dense_rows")
    e = sc.expected(case, seg_range=None)
    total = int(e["upper"].sum())
    variant = "fused" if path == 1 else "scan"
    out, kw = run(gpu_ctx, case, e, variant, cand_cap=total)
    check(case, e, out, kw, ("dense_rows", variant, "cand_cap = the upper bounds"))
    out, kw = run(gpu_ctx, case, e, variant, cand_cap=total - 1)
    assert out["overflow"] == 1 and out["needed"] == total
    assert np.array_equal(out["row_upper"], e["upper"]) and np.array_equal(out["row_count"], e["upper"])
    assert (out["cand_meta"] == FILL).all() and (out["cand_depths"].view(np.uint32) == FILL).all()
    pref, left = expected_starts(case, e, path)
    assert np.array_equal(out["row_start"], left if path == 2 else np.full_like(left, -1))       # (fused: the rows give up before they write their start)
    out, kw = run(gpu_ctx, case, e, variant)
    check(case, e, out, kw, ("dense_rows", variant, "after an overflow"))


def test_capacity_too_small_is_reported(gpu_ctx):
    case = sc.get_case("subset")
    e = sc.expected(case, seg_range=None)
    for path, need in ((0, int(e["count"].sum())), (1, int(e["upper"].sum())), (2, int(e["upper"].sum()))):
        with pytest.raises(capi.L3DError) as err:
            run(gpu_ctx, case, e, path=path, capacity=need - 1)
        assert err.value.code == 1 and err.value.needed == need and "pair_candidates" in str(err.value) and str(need) in str(err.value)
        out, kw = run(gpu_ctx, case, e, path=path, capacity=need)                          # exactly enough: no slack
        check(case, e, out, kw, ("subset", path, "capacity = needed"))


def _golden_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_pairwise", os.path.join(HERE, "golden", "make_golden_pairwise.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_reference_vectors(gpu_ctx):
    """tests/golden/pairwise_ref.npz: what the reference's own K_pairwise_matches wrote for every view and camera of two scenes (a helix, cameras that
    face each other).  Every path gives the set of (view, camera, source, target) with four positive depths it gave, and its depths bit for bit; the
    chains' upper bounds are its non-zero entries."""
    m = _golden_module()
    g = np.load(os.path.join(HERE, "golden", "pairwise_ref.npz"))
    seen = 0
    for name, scene, nn in m.scenes():
        o = op.run_scene(scene, nn)
        idx, val = g[name + "_idx"], g[name + "_val"]
        pos = (val > 0).all(axis=1)
        for v in sorted(o.trace):
            mv = o.trace[v]["marshal"]
            S, N = len(mv["src_segs"]), len(mv["offsets"])
            mine = idx[:, 0] == v
            want = {tuple(int(t) for t in i[1:]): d.tobytes() for i, d in zip(idx[mine & pos], val[mine & pos])}
            upper = np.bincount(idx[mine, 2] * N + idx[mine, 1], minlength=S * N)
            for path in (0, 1, 2):
                out = gpu_ctx.test_pair_candidates(mv["src_segs"], mv["tgt_segs"], mv["offsets"], mv["F"], mv["RtKinv"], mv["centers"], mv["RtKinv_src"], mv["C_src"],
                                                   np.arange(N), path=path, capacity=int(upper.sum()))
                got = {}
                for row in np.flatnonzero(out["row_count"]):
                    a = int(out["row_start"][row])
                    for r in range(a, a + int(out["row_count"][row])):
                        assert out["cand_meta"][r, 1] == row % N
                        got[(row % N, row // N, int(out["cand_meta"][r, 0]))] = out["cand_depths"][r].tobytes()
                assert got.keys() == want.keys(), (name, v, path, len(got), len(want))
                assert got == want, (name, v, path, "depths")
                if path:
                    assert np.array_equal(out["row_upper"], upper), (name, v, path, "upper bounds")
            seen += len(want)
    assert seen > 4000


def _valid():
    case = sc.get_case("subset")
    return dict(src_segs=case["src_segs"], tgt_segs=case["tgt_segs"], offsets=case["offsets"].copy(), F=case["F"], RtKinv=case["RtKinv"], centers=case["centers"],
                RtKinv_src=case["RtKinv_src"], C_src=case["C_src"], to_be_matched=case["tbm"].copy())


def _offsets(t, row, col, value):
    t["offsets"][row, col] = value
    return {}


# name -> (changes the tables in place, returns further arguments)
BROKEN = {
    "to_be_matched descends": lambda t: t.update(to_be_matched=np.array([2, 1, 4], np.int32)) or {},
    "to_be_matched repeats": lambda t: t.update(to_be_matched=np.array([1, 1, 4], np.int32)) or {},
    "to_be_matched past N": lambda t: t.update(to_be_matched=np.array([1, 2, 6], np.int32)) or {},
    "to_be_matched negative": lambda t: t.update(to_be_matched=np.array([-1, 2, 4], np.int32)) or {},
    "offsets past the targets": lambda t: _offsets(t, 5, 1, t["offsets"][5, 1] + 1),
    "negative offset": lambda t: _offsets(t, 0, 0, -1),
    "negative count": lambda t: _offsets(t, 3, 1, -5),
    "range starts below 0": lambda t: dict(seg_range=(-1, 10)),
    "range ends past S": lambda t: dict(seg_range=(0, len(t["src_segs"]) + 1)),
    "range ends before it starts": lambda t: dict(seg_range=(5, 4)),
    "path 3": lambda t: dict(path=3),
    "path -1": lambda t: dict(path=-1),
    "pretest 8": lambda t: dict(pretest=8),
    "pretest -1": lambda t: dict(pretest=-1),
    "spb 65": lambda t: dict(spb=65),
    "spb -1": lambda t: dict(spb=-1),
    "cand_cap on path 0": lambda t: dict(path=0, cand_cap=100),
    "ray_tables on path 0": lambda t: dict(path=0, ray_tables=1),
    "ray_tables 2": lambda t: dict(path=2, ray_tables=2),
}


@pytest.mark.parametrize("kind", list(BROKEN))
def test_broken_tables_are_refused(gpu_ctx, kind):
    """a wrong table or selection is a Python exception with the library's message, never a launch; the context then gives a valid case's result as before"""
    t = _valid()
    more = BROKEN[kind](t)
    paths = [more.pop("path")] if "path" in more else [0, 1, 2]
    for path in paths:
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.test_pair_candidates(path=path, capacity=4096, **t, **more)
        assert e.value.code == 1 and "pair_candidates" in str(e.value), (kind, path, str(e.value))
    case = sc.get_case("subset")
    ex = sc.expected(case, seg_range=None)
    for variant in ("seam", "fused", "scan"):
        out, kw = run(gpu_ctx, case, ex, variant)
        check(case, ex, out, kw, ("subset after a refusal", variant))


def test_refused_sizes(gpu_ctx):
    """16385 segments in a matched camera: more than the bit rows hold (16384 pass, tests/stage1_cases.py::case_wide); fused row starts past 96 cameras"""
    t = _valid()
    n = 16385
    t["tgt_segs"] = np.zeros((n, 4), np.float32)
    t["offsets"] = np.array([[0, 10], [0, n], [0, 10], [0, 10], [0, 10], [0, 10]], np.int32)
    for path in (0, 1, 2):
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.test_pair_candidates(path=path, capacity=16, **t)
        assert e.value.code == 1 and "16384" in str(e.value) and "pair_candidates" in str(e.value)
    t["to_be_matched"] = np.array([0, 2], np.int32)                      # (the wide camera is not matched: accepted)
    out = gpu_ctx.test_pair_candidates(path=0, capacity=16, **t)
    assert out["needed"] == 0 and not out["row_count"].any()
    case = sc.get_case("cams_97")
    ex = sc.expected(case, seg_range=None)
    with pytest.raises(capi.L3DError) as e:
        run(gpu_ctx, case, ex, path=1)
    assert e.value.code == 1 and "96" in str(e.value) and "pair_candidates" in str(e.value)
    out, kw = run(gpu_ctx, case, ex, "scan")
    check(case, ex, out, kw, ("cams_97 after the refusals", "scan"))
