"""l3d_junction_lines (k_junc_prepare, the search k_junc_count / k_junc_scan / k_junc_write, the components of the line ends, k_junc_rep, k_junc_star,
the vertex numbering and positions, the attachments) on the case tables of tests/junction_cases.py: bit for bit the model of tests/junction_model.py
and the host entry point l3d_test_junction_lines_host on every table (records, node_vertex, vertices, node_attach, counts); the search is the same
three launches at n = 2 and n = 513 and only junc_* kernels run; with no record the write pass and the components are not launched; repeated calls
on one context, large tables before small ones, give the same bytes; the slots behind the record list stay as they were (the library fills 16 of
them with ones before the write pass and refuses its own result if one changed, so every call that returns L3D_OK has passed that check); every
refusal is answered before anything is launched; and a table with more than 2^31 - 1 records is refused from the count pass's 64-bit total."""
import math

import numpy as np
import pytest

import junction_cases as jc

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in jc.CASES]
SEARCH = ("junc_count", "junc_scan", "junc_write")


def run(ctx, case):
    return ctx.junction_lines(case["lines"], case["tol"], case["ext"], cos_max=case["cos_max"], crossings=case["crossings"])


def launches_of(ctx):
    return {k: v[0] for k, v in ctx.profile_all().items() if v[0]}


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every table once on the device"""
    return {c["name"]: run(gpu_ctx, c) for c in jc.CASES}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_model_bit_for_bit(device_results, name):
    got, exp = device_results[name], jc.model_of(jc.BY_NAME[name])
    assert jc.same(got, exp), (name, jc.difference(got, exp))


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_twin_bit_for_bit(device_results, name):
    from line3d_amd import capi
    case = jc.BY_NAME[name]
    exp = capi.junction_lines_host(case["lines"], case["tol"], case["ext"], cos_max=case["cos_max"], crossings=case["crossings"])
    assert jc.same(device_results[name], exp), (name, jc.difference(device_results[name], exp))


def test_the_search_is_three_launches_for_any_n(gpu_ctx):
    gpu_ctx.profile_enable(True)
    try:
        for name in ("size_2", "size_513", "300_lines_from_one_point"):
            gpu_ctx.profile_reset()
            out = run(gpu_ctx, jc.BY_NAME[name])
            assert len(out["records"]) > 0 and len(out["vertices"]) > 0
            launches = launches_of(gpu_ctx)
            assert [launches.get(k, 0) for k in SEARCH] == [1, 1, 1], (name, launches)
            assert launches["junc_prepare"] == 1 and launches["junc_rep"] == 2 and launches["junc_star"] == 1 and launches["junc_vertex"] == 1
            assert launches["junc_attach"] == 2 and launches["junc_finish"] == 1 and launches["junc_cc_hook"] >= 3
            assert all(k.startswith("junc_") for k in launches), launches
        for name in ("size_1", "x_without_crossings"):        # no record: nothing to write, no component to hook, no vertex to place
            gpu_ctx.profile_reset()
            out = run(gpu_ctx, jc.BY_NAME[name])
            assert len(out["records"]) == 0 and launches_of(gpu_ctx) == {"junc_prepare": 1, "junc_count": 1, "junc_scan": 1}
    finally:
        gpu_ctx.profile_enable(False)


def test_repeated_calls_on_one_context_give_the_same_bytes(gpu_ctx, device_results):
    """the context's buffers are reused: the large tables first, then the small ones behind them, twice"""
    order = sorted(NAMES, key=lambda k: -len(jc.BY_NAME[k]["lines"]))
    for _ in range(2):
        for name in order:
            assert jc.same(run(gpu_ctx, jc.BY_NAME[name]), device_results[name]), name


def test_the_list_holds_exactly_the_counted_records(device_results):
    """ascending by (i, j), no pair twice, every pair inside the table: with the library's own check of the slots behind the list, nothing was written
    beyond n_records"""
    for name, out in device_results.items():
        r = out["records"]
        n = len(jc.BY_NAME[name]["lines"])
        i, j = r["i"].astype(np.int64), r["j"].astype(np.int64)
        assert np.all(np.diff(i * (n + 1) + j) > 0) and np.all(i < j) and (len(r) == 0 or (i.min() >= 0 and j.max() < n)), name
        assert out["counts"][1:4].sum() == len(r)


@pytest.mark.parametrize("name", [r[0] for r in jc.REFUSALS])
def test_refusals_before_any_launch(gpu_ctx, name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in jc.REFUSALS if r[0] == name)
    kw = jc.refusal_arguments(overrides)
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.junction_lines(kw["lines"], kw["tol"], kw["ext"], cos_max=kw["cos_max"], crossings=kw["crossings"])
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert not any(v[0] for v in gpu_ctx.profile_all().values())
    finally:
        gpu_ctx.profile_enable(False)


def test_an_empty_table(gpu_ctx):
    out = gpu_ctx.junction_lines(np.zeros((0, 6)), np.zeros(0), np.zeros(0), cos_max=0.9)
    assert out["records"].shape == (0,) and out["vertices"].shape == (0,) and out["node_vertex"].shape == (0,) and out["node_attach"].shape == (0,)
    assert out["counts"].tolist() == [0] * 8


def test_more_than_2_31_records_is_refused_as_unsupported(gpu_ctx):
    """65537 lines that start at one point, in directions at least 0.0026 radians apart (jc.fan: a grid of step 1 / 256) with cos_max = cos(0.05
    degrees): every pair is a record, 65537 x 65536 / 2 = 2^31 + 32768 of them, 32769 more than the list may hold.  The count pass sums them in 64 bits
    (the scan's int total wraps and is not used), the call is refused with the count in its cause, and the context serves the next call"""
    from line3d_amd import capi
    n = 65537
    assert n * (n - 1) // 2 == 2 ** 31 + 32768
    lines = jc.fan(n, 257, 1.0 / 256.0)
    with pytest.raises(capi.L3DError) as e:
        gpu_ctx.junction_lines(lines, np.full(n, 0.01), np.full(n, 0.01), cos_max=math.cos(math.radians(0.05)))
    assert e.value.code == 5 and str(n * (n - 1) // 2) in str(e.value) and "2^31 - 1" in str(e.value), str(e.value)
    case = jc.BY_NAME["size_257"]
    assert jc.same(run(gpu_ctx, case), jc.model_of(case))
