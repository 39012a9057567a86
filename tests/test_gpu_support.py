"""l3d_support_lines (k_sup_prepare, the search k_sup_count / k_sup_scan / k_sup_write: one (camera, 3-D segment) row per lane against column tiles in
LDS, k_sup_best) on the case tables of tests/support_cases.py: bit for bit the model of tests/support_model.py and the host entry point
l3d_test_support_lines_host on every table (records, cam_start, best, counts); the same with the cameras cut into chunks of 1 and 2, three search
launches per chunk at any n; segments in device memory give the same bytes; repeated calls on one context, large tables before small ones, give the
same bytes; the record list holds exactly the counted records (the library fills 16 slots behind it with ones before each write pass and refuses its
own result if one changed, so every call that returns L3D_OK has passed that check); every refusal is answered before anything is launched; and a
camera with more than 2^31 - 1 records is refused from the count pass's 64-bit total."""
import numpy as np
import pytest

import support_cases as sc

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in sc.CASES]
SEARCH = ("sup_count", "sup_scan", "sup_write")
ALL = ("sup_prepare",) + SEARCH + ("sup_best",)


def run(ctx, case, device=False):
    if not device:
        return ctx.support_lines(case["seg3d"], case["cams"], case["segs"], sc.params_of(case["p"]))
    import torch
    from line3d_amd import capi
    cols, start = capi.support_columns(case["segs"])
    d3 = torch.from_numpy(np.ascontiguousarray(case["seg3d"], np.float64)).to("cuda:0")
    d2 = torch.from_numpy(np.ascontiguousarray(cols, np.float32)).to("cuda:0")
    torch.cuda.synchronize()
    return ctx.support_lines(d3, case["cams"], (d2, start), sc.params_of(case["p"]))


def launches_of(ctx):
    return {k: v[0] for k, v in ctx.profile_all().items() if v[0]}


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every table once on the device, host segments, default chunks"""
    gpu_ctx.set_option("L3D_SUP_CHUNK", 0)
    return {c["name"]: run(gpu_ctx, c) for c in sc.CASES}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_model_bit_for_bit(device_results, name):
    assert sc.same(device_results[name], sc.model_of(sc.BY_NAME[name])), name


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_twin_bit_for_bit(device_results, name):
    from line3d_amd import capi
    case = sc.BY_NAME[name]
    assert sc.same(device_results[name], capi.support_lines_host(case["seg3d"], case["cams"], case["segs"], sc.params_of(case["p"]))), name


def test_segments_in_device_memory_give_the_same_bytes(gpu_ctx, device_results):
    for name in ("rows_257", "columns_513", "columns_0", "three_cameras_one_without_segments", "ineligible_columns", "clipped_row"):
        assert sc.same(run(gpu_ctx, sc.BY_NAME[name], device=True), device_results[name]), name


def test_device_segments_at_an_odd_offset(gpu_ctx, device_results):
    """2-D segments that start one float into an allocation: aligned to 4 bytes as the header asks, not to the 16 the column kernel loads, so the library
    copies them first; the same bytes"""
    import torch
    from line3d_amd import capi
    case = sc.BY_NAME["columns_257"]
    cols, start = capi.support_columns(case["segs"])
    flat = torch.zeros(cols.size + 1, dtype=torch.float32, device="cuda:0")
    flat[1:] = torch.from_numpy(cols.reshape(-1)).to("cuda:0")
    d2 = flat[1:].view(-1, 4)
    assert d2.data_ptr() % 16 == 4 and d2.is_contiguous()
    d3 = torch.from_numpy(np.ascontiguousarray(case["seg3d"], np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    assert sc.same(gpu_ctx.support_lines(d3, case["cams"], (d2, start), sc.params_of(case["p"])), device_results["columns_257"])


@pytest.mark.parametrize("chunk", [0, 1, 2])
def test_three_search_launches_per_chunk_of_cameras_at_any_n(gpu_ctx, device_results, chunk):
    gpu_ctx.set_option("L3D_SUP_CHUNK", chunk)
    gpu_ctx.profile_enable(True)
    try:
        for name in ("three_cameras_one_without_segments", "rows_1", "rows_257", "columns_513", "every_row_behind_the_near_plane", "columns_0"):
            case = sc.BY_NAME[name]
            gpu_ctx.profile_reset()
            out = run(gpu_ctx, case)
            assert sc.same(out, device_results[name]), name
            m = len(case["cams"])
            chunks = (m + chunk - 1) // chunk if chunk else 1
            got = launches_of(gpu_ctx)
            assert [got.get(k, 0) for k in SEARCH] == [chunks] * 3, (name, got)
            assert got.get("sup_prepare", 0) == (1 if sum(len(s) for s in case["segs"]) else 0) and got.get("sup_best", 0) == (1 if len(out["records"]) else 0), (name, got)
            assert set(got) <= set(ALL), got
    finally:
        gpu_ctx.profile_enable(False)
        gpu_ctx.set_option("L3D_SUP_CHUNK", 0)


def test_repeated_calls_on_one_context_give_the_same_bytes(gpu_ctx, device_results):
    """the context's buffers are reused: the large tables first, then the small ones behind them, twice"""
    order = sorted(NAMES, key=lambda k: -len(sc.BY_NAME[k]["seg3d"]) * sum(len(s) for s in sc.BY_NAME[k]["segs"]))
    for _ in range(2):
        for name in order:
            assert sc.same(run(gpu_ctx, sc.BY_NAME[name]), device_results[name]), name


def test_the_list_holds_exactly_the_counted_records(device_results):
    """per camera ascending by (k, j), no record twice, every record inside the tables, counts[2] of them: with the library's own check of the slots
    behind the list, nothing was written beyond the count"""
    for name, out in device_results.items():
        case = sc.BY_NAME[name]
        rec, start = out["records"], out["cam_start"]
        assert start[0] == 0 and start[-1] == len(rec) == out["counts"][2], name
        for c in range(len(case["cams"])):
            r = rec[start[c]:start[c + 1]]
            key = r["seg3d"].astype(np.int64) * (len(case["segs"][c]) + 1) + r["seg2d"]
            assert np.all(np.diff(key) > 0), name
            assert len(r) == 0 or (r["seg3d"].min() >= 0 and r["seg3d"].max() < len(case["seg3d"]) and r["seg2d"].min() >= 0 and r["seg2d"].max() < len(case["segs"][c])), name


def test_refusals_before_any_launch(gpu_ctx):
    import torch
    from line3d_amd import capi
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        for _, overrides, code, word in sc.REFUSALS:
            kw = sc.refusal_arguments(overrides)
            with pytest.raises(capi.L3DError) as e:
                gpu_ctx.support_lines(kw["seg3d"], kw["cams"], kw["segs"], sc.params_of(kw["p"]))
            assert e.value.code == code and word in str(e.value), str(e.value)
        for _, change, code, word in sc.RAW_REFUSALS:
            args, keep = sc.raw_arguments(change)
            rc, out = capi._support_call(gpu_ctx.lib.l3d_support_lines, (gpu_ctx.h,), *args)
            assert rc == code and out is None and word in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode(), gpu_ctx.lib.l3d_last_error(gpu_ctx.h)
        # memory kinds: host arrays handed in as device arrays; device arrays whose stated count leaves their allocation; a misaligned array
        (seg, n, cams, m, cols, start, prm), keep = sc.raw_arguments({})
        err = lambda: gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode()
        dev = gpu_ctx.lib.l3d_support_lines_device
        d3 = torch.from_numpy(keep["s"]).to("cuda:0")
        d2 = torch.from_numpy(np.concatenate([keep["cols"], keep["cols"]])).to("cuda:0")
        torch.cuda.synchronize()
        p3, p2 = capi.C.c_void_p(d3.data_ptr()), capi.C.c_void_p(d2.data_ptr())
        assert capi._support_call(dev, (gpu_ctx.h,), seg, n, cams, m, p2, start, prm)[0] == 1 and "3-D segments: device image: not device memory" in err()
        assert capi._support_call(dev, (gpu_ctx.h,), p3, n, cams, m, cols, start, prm)[0] == 1 and "2-D segments: device image: not device memory" in err()
        assert capi._support_call(dev, (gpu_ctx.h,), p3, 1 << 20, cams, m, p2, start, prm)[0] == 1 and "3-D segments" in err() and "allocation" in err()
        assert capi._support_call(dev, (gpu_ctx.h,), p3, n, cams, m, p2, np.array([0, 1 << 20], np.int64), prm)[0] == 1 and "2-D segments" in err() and "allocation" in err()
        assert capi._support_call(dev, (gpu_ctx.h,), capi.C.c_void_p(d3.data_ptr() + 4), n, cams, m, p2, start, prm)[0] == 1 and "aligned to 8" in err()
        assert capi._support_call(dev, (gpu_ctx.h,), p3, n, cams, m, capi.C.c_void_p(d2.data_ptr() + 2), start, prm)[0] == 1 and "aligned to 4" in err()
        assert not launches_of(gpu_ctx), "a refusal launched a kernel"
        rc, out = capi._support_call(dev, (gpu_ctx.h,), p3, n, cams, m, p2, start, prm)
        assert rc == 0 and out["counts"].tolist() == [1, 1, 1, 1] and out["best"].tolist() == [0]
        assert launches_of(gpu_ctx) == {k: 1 for k in ALL}
    finally:
        gpu_ctx.profile_enable(False)


def test_empty_inputs(gpu_ctx):
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        out = gpu_ctx.support_lines(np.zeros((0, 6)), sc.GOOD["cams"], sc.GOOD["segs"])
        assert len(out["records"]) == 0 and out["cam_start"].tolist() == [0, 0] and out["best"].tolist() == [-1] and out["counts"].tolist() == [0, 0, 0, 0]
        out = gpu_ctx.support_lines(sc.GOOD["seg3d"], [], [])
        assert len(out["records"]) == 0 and out["cam_start"].tolist() == [0] and out["best"].shape == (0,) and out["counts"].tolist() == [0, 0, 0, 0]
        assert not launches_of(gpu_ctx)
    finally:
        gpu_ctx.profile_enable(False)


def test_a_camera_with_more_than_2_31_records_is_refused_as_unsupported(gpu_ctx):
    """65536 copies of one 3-D segment against 32768 copies of a 2-D segment on it: 2^31 records in one camera, one more than the list may hold.  The
    count pass sums them in 64 bits, the call is refused with the count in its cause before any record list is allocated (no write pass runs), and
    the context serves the next call"""
    from line3d_amd import capi
    n, k = 65536, 32768
    assert n * k == 2 ** 31
    seg3d = np.tile(np.array(sc.ROW, np.float64), (n, 1))
    cols = np.tile(np.array([[2, 1, 10, 1]], np.float32), (k, 1))
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.support_lines(seg3d, [sc.UNIT], [cols], sc.params_of(sc.P()))
        assert e.value.code == 5 and str(n * k) in str(e.value) and "2^31 - 1" in str(e.value), str(e.value)
        assert launches_of(gpu_ctx) == {"sup_prepare": 1, "sup_count": 1}
    finally:
        gpu_ctx.profile_enable(False)
    case = sc.BY_NAME["rows_257"]
    assert sc.same(run(gpu_ctx, case), sc.model_of(case))
