"""l3d_refine_lines (k_refine_lines: one wave per cluster) on the case table of tests/refine_cases.py: bit for bit the host entry point
l3d_test_refine_host on every case and every output, within the measured tolerance of the model (tests/golden/refine_tolerance.json), independent of a
group's position and of the run, empty for no groups, and every refusal answered with L3D_ERR_INVALID before anything is launched."""
import numpy as np
import pytest

import refine_cases as rc

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in rc.CASES]
OUTPUTS = ("line", "rms_before", "rms_after", "iterations", "status", "seg_count", "segs")


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every case once on the device, with the launches of k_refine_lines counted"""
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    out = {c["name"]: gpu_ctx.refine_lines(*rc.args_of(c)) for c in rc.CASES}
    launches = gpu_ctx.profile_get("refine_lines")[0]
    gpu_ctx.profile_enable(False)
    return out, launches


@pytest.fixture(scope="module")
def host_results():
    from line3d_amd import capi
    return {c["name"]: capi.refine_lines_host(*rc.args_of(c)) for c in rc.CASES}


def test_the_kernel_was_launched_once_per_case(device_results):
    assert device_results[1] == len(rc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_bit_for_bit(name, device_results, host_results):
    dev, host = device_results[0][name], host_results[name]
    for q in OUTPUTS:
        assert dev[q].dtype == host[q].dtype and dev[q].shape == host[q].shape, "%s: %s" % (name, q)
        assert dev[q].tobytes() == host[q].tobytes(), "%s: %s differs from the host's" % (name, q)


@pytest.mark.parametrize("name", NAMES)
def test_device_agrees_with_the_model(name, device_results):
    rc.check_against_model(rc.BY_NAME[name], device_results[0][name])


def test_position_independence_and_two_identical_runs(gpu_ctx, device_results):
    ref = None
    for k in ("first", "middle", "last"):
        c = rc.BY_NAME["position_" + k]
        g = rc.per_group(device_results[0][c["name"]], c["probe_at"])
        b = b"".join(np.asarray(g[q]).tobytes() for q in ("line", "rms_before", "rms_after", "iterations", "status", "segs"))
        ref = b if ref is None else ref
        assert b == ref, k
    c = rc.BY_NAME["nan_in_points"]
    out, alone = device_results[0][c["name"]], device_results[0][c["clean_name"]]
    for g, ga in ((0, 0), (2, 1)):
        a, b = rc.per_group(out, g), rc.per_group(alone, ga)
        assert all(np.asarray(a[q]).tobytes() == np.asarray(b[q]).tobytes() for q in a), "the groups beside the NaN are untouched"
    for name in ("groups_5", "members_300"):
        again = gpu_ctx.refine_lines(*rc.args_of(rc.BY_NAME[name]))
        assert all(again[q].tobytes() == device_results[0][name][q].tobytes() for q in OUTPUTS), name


def test_no_groups_and_refusals_launch_nothing(gpu_ctx):
    from line3d_amd import capi
    gs, mc, ms, mp, cams, it, hub = rc.args_of(rc.BY_NAME["members_5"])
    bad_cam = cams.copy()
    bad_cam[1, 2, 3] = np.nan
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        out = gpu_ctx.refine_lines(np.zeros(1, np.int32), mc[:0], ms[:0], mp[:0], cams, it, hub)
        assert all(len(out[q]) == 0 for q in OUTPUTS)
        for args in ((np.array([1, 5], np.int32), mc, ms, mp, cams, it, hub), (np.array([0, 5, 3], np.int32), mc, ms, mp, cams, it, hub),
                     (gs, mc + len(cams), ms, mp, cams, it, hub), (gs, mc - 1, ms, mp, cams, it, hub), (gs, mc, ms, mp, cams, -1, hub), (gs, mc, ms, mp, cams, it, -0.5),
                     (gs, mc, ms, mp, bad_cam, it, hub)):
            with pytest.raises(capi.L3DError) as e:
                gpu_ctx.refine_lines(*args)
            assert e.value.code == 1 and "refine" in str(e.value)
        assert gpu_ctx.profile_get("refine_lines")[0] == 0, "a refusal or an empty call launched the kernel"
        gpu_ctx.refine_lines(gs, mc, ms, mp, cams, it, hub)
        assert gpu_ctx.profile_get("refine_lines")[0] == 1
    finally:
        gpu_ctx.profile_enable(False)
