"""l3d_mask_segments (k_segmask_count, k_segmask_scan, k_segmask_write: one wave per segment) on the case table of tests/segmask_cases.py: bit for bit the
model of tests/segmask_model.py and the host entry point l3d_test_mask_segments_host on every case, in segments and in src_index; a mask in device
memory and segments in device memory give the same bytes as host arrays; the launches are the three named kernels, once per call whatever the number
of segments; and every refusal is answered before anything is launched."""
import numpy as np
import pytest

import segmask_cases as sc

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in sc.CASES]
KERNELS = ("segmask_count", "segmask_scan", "segmask_write")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    return np.array_equal(got[1], want[1]) and got[0].shape == want[0].shape and np.array_equal(_bits(got[0]), _bits(want[0]))


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every case once on the device, host mask and host segments, with every profiled launch counted"""
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    out = {c["name"]: gpu_ctx.mask_segments(c["segments"], sc.capi_mask(c)) for c in sc.CASES}
    launches = {k: v[0] for k, v in gpu_ctx.profile_all().items()}
    gpu_ctx.profile_enable(False)
    return out, launches


def test_the_kernels_launched_are_the_named_ones_once_per_call(device_results):
    out, launches = device_results
    calls = sum(1 for c in sc.CASES if len(c["segments"]) > 0)
    writes = sum(1 for c in sc.CASES if len(sc.model_of(c)[1]) > 0)
    assert launches["segmask_count"] == calls and launches["segmask_scan"] == calls, "one count and one scan launch per call with segments, whatever their number"
    assert launches["segmask_write"] == writes, "one write launch per call that emits a segment"
    assert {k for k, n in launches.items() if n} == set(KERNELS), "another kernel was launched"


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_model_bit_for_bit(device_results, name):
    got = device_results[0][name]
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert _same(got, sc.model_of(sc.BY_NAME[name])), name


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_twin_bit_for_bit(device_results, name):
    from line3d_amd import capi
    case = sc.BY_NAME[name]
    assert _same(device_results[0][name], capi.mask_segments_host(case["segments"], sc.capi_mask(case))), name


def test_device_mask_and_device_segments_give_the_same_bytes(gpu_ctx, device_results):
    """the mask as a torch tensor (the row-stride case as a view into wider rows on the device too), the segments as a torch tensor, and both"""
    import torch
    names = [n for n in NAMES if sc.BY_NAME[n]["claim"][0] in ("stride", "lens", "grows", "samples", "always_dropped", "threshold")] + ["count_5", "count_4097", "count_0"]
    for name in names:
        case, want = sc.BY_NAME[name], device_results[0][name]
        m = case["mask"]
        if m.strides[0] > m.shape[1]:
            wide = torch.full((m.shape[0], m.strides[0]), 255, dtype=torch.uint8, device="cuda:0")
            wide[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m)).to("cuda:0")
            dmask = wide[:, :m.shape[1]]
            assert dmask.stride(0) > dmask.shape[1]
        else:
            dmask = torch.from_numpy(np.ascontiguousarray(m)).to("cuda:0")
        dsegs = torch.from_numpy(np.ascontiguousarray(case["segments"])).to("cuda:0")
        torch.cuda.synchronize()
        assert _same(gpu_ctx.mask_segments(case["segments"], sc.capi_mask(case, dmask)), want), name + ": device mask"
        assert _same(gpu_ctx.mask_segments(dsegs, sc.capi_mask(case)), want), name + ": device segments"
        assert _same(gpu_ctx.mask_segments(dsegs, sc.capi_mask(case, dmask)), want), name + ": device mask and device segments"


def test_results_do_not_depend_on_the_run(gpu_ctx, device_results):
    for name in ("count_4097", "lens_fisheye_split", "split_grows"):
        case = sc.BY_NAME[name]
        assert _same(gpu_ctx.mask_segments(case["segments"], sc.capi_mask(case)), device_results[0][name]), name


def test_refusals_launch_nothing(gpu_ctx, device_results):
    import torch
    from line3d_amd import capi
    segs = np.array([[1.0, 1.0, 9.0, 6.0]], np.float32)
    mask = np.full((12, 16), 255, np.uint8)
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        def refused(s, m, cause):
            with pytest.raises(capi.L3DError, match="error 1") as e:
                gpu_ctx.mask_segments(s, m)
            assert cause in str(e.value), str(e.value)

        refused(segs, None, "mask is null")
        m = capi.segment_mask(mask)
        m.mask_width = 0
        refused(segs, m, "extent")
        m = capi.segment_mask(mask)
        m.mask_row_stride = 15
        refused(segs, m, "row stride")
        refused(segs, capi.segment_mask(mask, mode=3), "mode")
        refused(segs, capi.segment_mask(mask, threshold=256), "threshold")
        refused(segs, capi.segment_mask(mask, keep_permille=1001), "keep_permille")
        refused(segs, capi.segment_mask(mask, max_gap=-1), "max_gap")
        refused(segs, capi.segment_mask(mask, min_length=float("nan")), "min_length")
        cam = (20.0, 20.0, 8.0, 6.0)
        refused(segs, capi.segment_mask(mask, lens=capi.lens(3, [0.1], camera=cam), camera=cam), "unknown model")
        # memory kinds: a host plane that claims to be device memory, a device plane whose stated extent leaves its allocation, host segments
        # handed in as device segments
        m = capi.segment_mask(mask)
        m.mask_on_device = 1
        refused(segs, m, "not device memory")
        dmask = torch.full((12, 16), 255, dtype=torch.uint8, device="cuda:0")
        m = capi.segment_mask(dmask)
        m.mask_height = 1 << 20
        refused(segs, m, "allocation")
        rc, _, _ = capi._mask_segments_call(gpu_ctx.lib.l3d_mask_segments_device, (gpu_ctx.h,), segs.ctypes.data_as(capi.C.c_void_p), 1, capi.segment_mask(mask))
        assert rc == 1
        assert all(gpu_ctx.profile_get(k)[0] == 0 for k in KERNELS), "a refusal launched a kernel"
        out, src = gpu_ctx.mask_segments(segs, capi.segment_mask(dmask))
        assert np.array_equal(_bits(out), _bits(segs)) and src.tolist() == [0]
        assert [gpu_ctx.profile_get(k)[0] for k in KERNELS] == [1, 1, 1]
    finally:
        gpu_ctx.profile_enable(False)
