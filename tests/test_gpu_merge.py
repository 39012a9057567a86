"""l3d_merge_lines (k_merge_prepare, the pair search k_merge_count / k_merge_scan / k_merge_write, the components, k_merge_rep, k_merge_star,
k_merge_group) on the case tables of tests/merge_cases.py: bit for bit the model of tests/merge_model.py and the host entry point
l3d_test_merge_lines_host on every table (group, pairs, counts); the pair search is the same three launches at n = 2 and n = 513; repeated calls on one
context, large tables before small ones, give the same bytes; the slots behind the pair list stay as they were (the library fills 16 of them with
ones before the write pass and refuses its own result if one changed, so every call that returns L3D_OK has passed that check); and every refusal
is answered before anything is launched."""
import numpy as np
import pytest

import merge_cases as mc

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in mc.CASES]
SEARCH = ("merge_count", "merge_scan", "merge_write")


def run(ctx, case):
    return ctx.merge_lines(case["lines"], case["tol"], cos_min=case["cos_min"], max_gap=case["max_gap"])


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every table once on the device"""
    return {c["name"]: run(gpu_ctx, c) for c in mc.CASES}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_model_bit_for_bit(device_results, name):
    assert mc.same(device_results[name], mc.model_of(mc.BY_NAME[name])), name


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_twin_bit_for_bit(device_results, name):
    from line3d_amd import capi
    case = mc.BY_NAME[name]
    assert mc.same(device_results[name], capi.merge_lines_host(case["lines"], case["tol"], cos_min=case["cos_min"], max_gap=case["max_gap"])), name


def test_the_pair_search_is_three_launches_for_any_n(gpu_ctx):
    gpu_ctx.profile_enable(True)
    try:
        seen = {}
        for name in ("size_2", "size_513", "300_mutually_matching_lines"):
            gpu_ctx.profile_reset()
            out = run(gpu_ctx, mc.BY_NAME[name])
            assert len(out["pairs"]) > 0
            launches = {k: v[0] for k, v in gpu_ctx.profile_all().items() if v[0]}
            assert [launches.get(k, 0) for k in SEARCH] == [1, 1, 1], (name, launches)
            assert launches["merge_prepare"] == 1 and launches["merge_rep"] == 2 and launches["merge_star"] == 1 and launches["merge_group"] == 1
            assert all(k.startswith("merge_") for k in launches), launches
            seen[name] = launches
        gpu_ctx.profile_reset()
        out = run(gpu_ctx, mc.BY_NAME["size_1"])            # no pair: nothing to write, no component to hook
        launches = {k: v[0] for k, v in gpu_ctx.profile_all().items() if v[0]}
        assert len(out["pairs"]) == 0 and launches.get("merge_count") == 1 and launches.get("merge_scan") == 1 and "merge_write" not in launches and "merge_cc_hook" not in launches
    finally:
        gpu_ctx.profile_enable(False)


def test_repeated_calls_on_one_context_give_the_same_bytes(gpu_ctx, device_results):
    """the context's buffers are reused: the large tables first, then the small ones behind them, twice"""
    order = sorted(NAMES, key=lambda k: -len(mc.BY_NAME[k]["lines"]))
    for _ in range(2):
        for name in order:
            assert mc.same(run(gpu_ctx, mc.BY_NAME[name]), device_results[name]), name


def test_the_list_holds_exactly_the_counted_pairs(device_results):
    """ascending by (i, j), no pair twice, every pair inside the table: with the library's own check of the slots behind the list, nothing was written
    beyond n_pairs"""
    for name, out in device_results.items():
        p = out["pairs"].astype(np.int64)
        n = len(mc.BY_NAME[name]["lines"])
        key = p[:, 0] * (n + 1) + p[:, 1]
        assert np.all(np.diff(key) > 0) and np.all(p[:, 0] < p[:, 1]) and (len(p) == 0 or (p.min() >= 0 and p.max() < n)), name


@pytest.mark.parametrize("name", [r[0] for r in mc.REFUSALS])
def test_refusals_before_any_launch(gpu_ctx, name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in mc.REFUSALS if r[0] == name)
    kw = mc.refusal_arguments(overrides)
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.merge_lines(kw["lines"], kw["tol"], cos_min=kw["cos_min"], max_gap=kw["max_gap"])
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert not any(v[0] for v in gpu_ctx.profile_all().values())
    finally:
        gpu_ctx.profile_enable(False)


def test_an_empty_table(gpu_ctx):
    out = gpu_ctx.merge_lines(np.zeros((0, 6)), np.zeros(0), cos_min=0.9)
    assert out["group"].shape == (0,) and out["pairs"].shape == (0, 2) and out["counts"].tolist() == [0, 0, 0, 0]


def test_more_than_2_31_pairs_is_refused_as_unsupported(gpu_ctx):
    """65537 identical lines: 65537 x 65536 / 2 = 2^31 + 32768 pairs, 32769 more than the list may hold.  The count pass sums them in 64 bits (the scan's
    int total wraps and is not used), the call is refused with the count in its cause, and the context serves the next call"""
    from line3d_amd import capi
    n = 65537
    assert n * (n - 1) // 2 == 2 ** 31 + 32768
    lines = np.tile(np.array([[0.1, 0.2, 0.3, 1.3, 2.2, 0.8]]), (n, 1))
    with pytest.raises(capi.L3DError) as e:
        gpu_ctx.merge_lines(lines, np.full(n, 0.01))
    assert e.value.code == 5 and str(n * (n - 1) // 2) in str(e.value) and "2^31 - 1" in str(e.value), str(e.value)
    case = mc.BY_NAME["size_257"]
    assert mc.same(run(gpu_ctx, case), mc.model_of(case))
