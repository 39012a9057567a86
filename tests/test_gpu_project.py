"""l3d_project_lines (k_proj_count, k_proj_scan, k_proj_write: one (camera, segment) pair per lane) on the case table of tests/project_cases.py: byte
for byte the model of tests/project_model.py and the host entry point l3d_test_project_lines_host on every case, in every output array; the same with
the cameras cut into chunks of 1 and 2; 3-D segments in device memory give the same bytes; the launches are the three named kernels, once per chunk
whatever the number of segments; and every refusal is answered before anything is launched."""
import numpy as np
import pytest

import project_cases as pc

same = pc.same

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in pc.CASES]
KERNELS = ("proj_count", "proj_scan", "proj_write")


def run(ctx, case, seg3d=None):
    return ctx.project_lines(case["seg3d"] if seg3d is None else seg3d, case["cams"], case["near"], case["margin"])


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every case once on the device, host segments, default chunks, with every profiled launch counted"""
    gpu_ctx.set_option("L3D_PROJ_CHUNK", 0)
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    out = {c["name"]: run(gpu_ctx, c) for c in pc.CASES}
    launches = {k: v[0] for k, v in gpu_ctx.profile_all().items()}
    gpu_ctx.profile_enable(False)
    return out, launches


def test_the_kernels_launched_are_the_named_ones_once_per_call(device_results):
    out, launches = device_results
    calls = sum(1 for c in pc.CASES if len(c["seg3d"]) > 0 and len(c["cams"]) > 0)          # every case fits one chunk of 64 cameras
    assert [launches[k] for k in KERNELS] == [calls] * 3
    assert {k for k, n in launches.items() if n} == set(KERNELS), "another kernel was launched"


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_model_byte_for_byte(device_results, name):
    got = device_results[0][name]
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.uint8 and got[3].dtype == np.int64
    assert same(got, pc.model_of(pc.BY_NAME[name])), name


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_twin_byte_for_byte(device_results, name):
    from line3d_amd import capi
    case = pc.BY_NAME[name]
    assert same(device_results[0][name], capi.project_lines_host(case["seg3d"], case["cams"], case["near"], case["margin"])), name


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunks_of_cameras_give_the_same_bytes_three_launches_each(gpu_ctx, device_results, chunk):
    gpu_ctx.set_option("L3D_PROJ_CHUNK", chunk)
    gpu_ctx.profile_enable(True)
    try:
        for name in NAMES:
            case = pc.BY_NAME[name]
            gpu_ctx.profile_reset()
            assert same(run(gpu_ctx, case), device_results[0][name]), name
            m, n = len(case["cams"]), len(case["seg3d"])
            chunks = (m + chunk - 1) // chunk if n > 0 else 0
            assert [gpu_ctx.profile_get(k)[0] for k in KERNELS] == [chunks] * 3, name
    finally:
        gpu_ctx.profile_enable(False)
        gpu_ctx.set_option("L3D_PROJ_CHUNK", 0)


def test_launches_do_not_depend_on_n(gpu_ctx):
    gpu_ctx.profile_enable(True)
    try:
        counts = []
        for name in ("size_3x63", "size_3x130"):
            gpu_ctx.profile_reset()
            run(gpu_ctx, pc.BY_NAME[name])
            counts.append([gpu_ctx.profile_get(k)[0] for k in KERNELS])
        assert counts == [[1, 1, 1], [1, 1, 1]]
    finally:
        gpu_ctx.profile_enable(False)


def test_device_segments_give_the_same_bytes(gpu_ctx, device_results):
    import torch
    for name in ("size_3x65", "size_3x130", "size_1x1", "input_nan_inf", "size_empty_row"):
        case = pc.BY_NAME[name]
        d = torch.from_numpy(np.ascontiguousarray(case["seg3d"], np.float64)).to("cuda:0")
        torch.cuda.synchronize()
        assert same(run(gpu_ctx, case, d), device_results[0][name]), name


def test_refusals_launch_nothing(gpu_ctx, device_results):
    import torch
    from line3d_amd import capi
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        for _, overrides, code, word in pc.REFUSALS:
            kw = pc.refusal_arguments(overrides)
            with pytest.raises(capi.L3DError, match="error %d" % code) as e:
                gpu_ctx.project_lines(kw["seg3d"], kw["cams"], kw["near"], kw["margin"])
            assert word in str(e.value), str(e.value)
        # memory kinds: host segments handed in as device segments; device segments whose stated count leaves their allocation
        seg = np.array([[0, 0, 2, 0.1, 0.1, 2]], np.float64)
        cams = capi.cameras([pc.cam()])
        rc = capi._project_call(gpu_ctx.lib.l3d_project_lines_device, (gpu_ctx.h,), capi._p(seg), 1, cams, 1, 1e-3, 0.0)[0]
        assert rc == 1 and "not device memory" in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode()
        d = torch.from_numpy(seg).to("cuda:0")
        torch.cuda.synchronize()
        rc = capi._project_call(gpu_ctx.lib.l3d_project_lines_device, (gpu_ctx.h,), capi.C.c_void_p(d.data_ptr()), 1 << 20, cams, 1, 1e-3, 0.0)[0]
        assert rc == 1 and "allocation" in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode()
        assert all(gpu_ctx.profile_get(k)[0] == 0 for k in KERNELS), "a refusal launched a kernel"
        segs, src, flags, start = gpu_ctx.project_lines(d, cams, 1e-3, 0.0)
        assert src.tolist() == [0] and start.tolist() == [0, 1]
        assert [gpu_ctx.profile_get(k)[0] for k in KERNELS] == [1, 1, 1]
    finally:
        gpu_ctx.profile_enable(False)
