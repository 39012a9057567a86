"""l3d_plane_lines (k_plane_prepare, k_plane_hyp, the hypothesis search k_plane_count / k_plane_scan / k_plane_write, the components of the
hypotheses, k_plane_rep, k_plane_star, the candidates' numbering and parameters, the membership pass, the extents) on the case tables of
tests/plane_cases.py and on the inputs of tests/golden/planes_small.npz: bit for bit the model of tests/plane_model.py and the host entry point
l3d_test_plane_lines_host (planes, members, hyp_plane, counts); the search is the same three launches at m = 1 and m = 4096 and only plane_* kernels
run; repeated calls on one context, large tables before small ones, give the same bytes; the slots behind the edge list and the member list stay as
they were (the library fills 16 of them with ones before each write pass and refuses its own result if one changed, so every call that returns
L3D_OK has passed that check); the lists hold exactly the counted records; every refusal is answered before anything is launched; empty tables."""
import os

import numpy as np
import pytest

import plane_cases as pc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [c["name"] for c in pc.CASES]
SEARCH = ("plane_count", "plane_scan", "plane_write")


def run(ctx, case):
    return ctx.plane_lines(case["lines"], case["tol"], case["seeds"], cos_max=case["cos_max"], cos_min=case["cos_min"], min_lines=case["min_lines"])


def host(case):
    from line3d_amd import capi
    return capi.plane_lines_host(case["lines"], case["tol"], case["seeds"], cos_max=case["cos_max"], cos_min=case["cos_min"], min_lines=case["min_lines"])


def launches_of(ctx):
    return {k: v[0] for k, v in ctx.profile_all().items() if v[0]}


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every table once on the device"""
    return {c["name"]: run(gpu_ctx, c) for c in pc.CASES}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_model_bit_for_bit(device_results, name):
    got, exp = device_results[name], pc.model_of(pc.BY_NAME[name])
    assert pc.same(got, exp), (name, pc.difference(got, exp))


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_twin_bit_for_bit(device_results, name):
    exp = host(pc.BY_NAME[name])
    assert pc.same(device_results[name], exp), (name, pc.difference(device_results[name], exp))


def test_device_model_and_host_twin_agree_on_the_golden_inputs(gpu_ctx):
    from line3d_amd import capi
    g = np.load(os.path.join(HERE, "golden", "planes_small.npz"))
    got = gpu_ctx.plane_lines(g["lines"], g["tol"], g["seeds"], cos_max=pc.COS10, cos_min=pc.COS10, min_lines=3)
    exp = {k: g[k] for k in pc.KEYS}
    assert pc.same(got, exp), pc.difference(got, exp)
    assert pc.same(got, capi.plane_lines_host(g["lines"], g["tol"], g["seeds"], cos_max=pc.COS10, cos_min=pc.COS10, min_lines=3))


def test_the_launch_count_does_not_depend_on_m(gpu_ctx):
    """the search is three launches at m = 1 and at m = 4096, everything but the components' rounds runs once (the representatives twice), and
    only plane_* kernels run"""
    gpu_ctx.profile_enable(True)
    try:
        seen = {}
        for name in ("size_n12_m1", "size_n300_m513", "size_n2052_m4096"):
            gpu_ctx.profile_reset()
            out = run(gpu_ctx, pc.BY_NAME[name])
            assert len(out["planes"]) > 0
            launches = launches_of(gpu_ctx)
            assert all(k.startswith("plane_") for k in launches), launches
            assert launches["plane_prepare"] == 1 and launches["plane_hyp"] == 1 and launches["plane_count"] == 1 and launches["plane_scan"] == 1
            if out["counts"][2]:
                assert [launches.get(k, 0) for k in SEARCH] == [1, 1, 1], (name, launches)
                assert launches["plane_cc_hook"] >= 3 and launches["plane_cc_hook"] == launches["plane_cc_compress"]
            else:
                assert "plane_write" not in launches and "plane_cc_hook" not in launches
            seen[name] = {k: v for k, v in launches.items() if k not in ("plane_write", "plane_cc_hook", "plane_cc_compress")}
            assert seen[name]["plane_rep"] == 2 and all(v == 1 for k, v in seen[name].items() if k != "plane_rep"), seen[name]
        assert seen["size_n12_m1"] == seen["size_n300_m513"] == seen["size_n2052_m4096"]
        gpu_ctx.profile_reset()                              # no eligible hypothesis: no candidate, nothing to test for membership
        out = run(gpu_ctx, pc.BY_NAME["size_n1_m1"])
        assert len(out["planes"]) == 0 and not any(k.startswith("plane_m") or k in ("plane_keep", "plane_seed", "plane_extent") for k in launches_of(gpu_ctx))
    finally:
        gpu_ctx.profile_enable(False)


def test_repeated_calls_on_one_context_give_the_same_bytes(gpu_ctx, device_results):
    """the context's buffers are reused: the large tables first, then the small ones behind them, twice"""
    order = sorted(NAMES, key=lambda k: -len(pc.BY_NAME[k]["seeds"]))
    for _ in range(2):
        for name in order:
            assert pc.same(run(gpu_ctx, pc.BY_NAME[name]), device_results[name]), name


def test_the_lists_hold_exactly_the_counted_records(device_results):
    """members ascending by (plane, line), no record twice, every record inside the tables, per plane as many as it says: with the library's own
    check of the slots behind the lists, nothing was written beyond the counted records"""
    for name, out in device_results.items():
        case = pc.BY_NAME[name]
        n, m = len(case["lines"]), len(case["seeds"])
        mem, pl, hp, counts = out["members"], out["planes"], out["hyp_plane"], out["counts"]
        assert counts[6] == len(pl) and counts[7] == len(mem) and counts[3] - counts[5] == counts[6], name
        key = mem["plane"].astype(np.int64) * (n + 1) + mem["line"]
        assert np.all(np.diff(key) > 0) and (len(mem) == 0 or (mem["plane"].min() >= 0 and mem["plane"].max() < len(pl) and mem["line"].min() >= 0 and mem["line"].max() < n)), name
        assert np.bincount(mem["plane"], minlength=len(pl)).tolist() == pl["n_lines"].tolist() and np.all(mem["pad"] == 0) and np.all((mem["flags"] & ~1) == 0), name
        assert len(hp) == m and np.bincount(hp[hp >= 0], minlength=len(pl)).tolist() == pl["n_hyp"].tolist(), name
        assert list(pl["first_hyp"]) == sorted(pl["first_hyp"]) and all(hp[h] == k for k, h in enumerate(pl["first_hyp"])), name


@pytest.mark.parametrize("name", [r[0] for r in pc.REFUSALS])
def test_refusals_before_any_launch(gpu_ctx, name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in pc.REFUSALS if r[0] == name)
    kw = pc.refusal_arguments(overrides)
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.plane_lines(kw["lines"], kw["tol"], kw["seeds"], cos_max=kw["cos_max"], cos_min=kw["cos_min"], min_lines=kw["min_lines"])
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert not any(v[0] for v in gpu_ctx.profile_all().values())
    finally:
        gpu_ctx.profile_enable(False)


def test_empty_tables(gpu_ctx):
    for lines, tol, seeds in ((np.zeros((0, 6)), np.zeros(0), np.zeros((0, 2), np.int32)), (pc.GOOD["lines"], pc.GOOD["tol"], np.zeros((0, 2), np.int32))):
        gpu_ctx.profile_enable(True)
        gpu_ctx.profile_reset()
        try:
            out = gpu_ctx.plane_lines(lines, tol, seeds)
            assert not any(v[0] for v in gpu_ctx.profile_all().values())
        finally:
            gpu_ctx.profile_enable(False)
        assert out["planes"].shape == (0,) and out["members"].shape == (0,) and out["hyp_plane"].shape == (0,) and out["counts"].tolist() == [0] * 8
