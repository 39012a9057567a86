"""l3d_covisibility (k_covis_keys, the sort, k_covis_runs, k_covis_count, k_covis_scan, k_covis_write) on the case table of tests/covis_cases.py: on
every case num_wps, row_start, col and count equal the model of tests/covis_model.py and the host hook l3d_test_covisibility_host, integer for
integer; path is 0 without repeated ids and 1 with them, where the result is the replay's; the launches are the named covis_* kernels, as many for
three views as for a view of 200 000 observations; and what is refused is refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import covis_cases
import covis_model

pytestmark = pytest.mark.gpu

KERNELS = ("covis_keys", "covis_sort", "covis_runs", "covis_count", "covis_scan", "covis_write")


def _run_profiled(ctx, name):
    case = covis_cases.CASES[name]
    ctx.set_option("L3D_COVIS_TILE", case["tile"])
    ctx.profile_reset()
    out = ctx.covisibility(case["lists"])
    launches = {k: v[0] for k, v in ctx.profile_all().items() if v[0]}
    ctx.set_option("L3D_COVIS_TILE", 0)
    return out, launches


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every case once on the device, with the launches of each call"""
    gpu_ctx.profile_enable(True)
    res = {name: _run_profiled(gpu_ctx, name) for name in covis_cases.NAMES}
    gpu_ctx.profile_enable(False)
    return res


@pytest.mark.parametrize("name", covis_cases.NAMES)
def test_device_equals_the_model(device_results, name):
    got = device_results[name][0]
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int32 and got[2].dtype == np.int32 and got[3].dtype == np.uint32
    want = covis_model.reference(name)
    for what, g, w in zip(("num_wps", "row_start", "col", "count"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs from the model" % (name, what)


@pytest.mark.parametrize("name", covis_cases.NAMES)
def test_device_equals_the_host_hook(device_results, name):
    from line3d_amd import capi
    assert covis_model.same(device_results[name][0], capi.covisibility_host(covis_cases.CASES[name]["lists"])), name


@pytest.mark.parametrize("name", covis_cases.NAMES)
def test_path(device_results, name):
    assert device_results[name][0][4] == (1 if covis_cases.CASES[name]["repeats"] else 0)


@pytest.mark.parametrize("name", covis_cases.NAMES)
def test_the_launches_are_the_named_kernels(device_results, name):
    launches = device_results[name][1]
    if covis_cases.CASES[name]["repeats"]:      # the repeat is seen behind the count and its scan: nothing is written on the device
        assert launches == {k: 1 for k in KERNELS if k != "covis_write"}
    else:
        assert launches == {k: 1 for k in KERNELS}


def test_launch_count_does_not_depend_on_the_observations(device_results):
    """one column tile each: three views and a view of 200 000 observations take the same launches"""
    small, big = device_results["three_views"][1], device_results["one_view_of_200000_observations"][1]
    assert covis_cases.CASES["three_views"]["tile"] == covis_cases.CASES["one_view_of_200000_observations"]["tile"] == 0
    assert small == big and sum(small.values()) == len(KERNELS)
    # and the tiles are a dimension of the grid: five tiles of 64 columns take no more launches
    assert device_results["tiling_300_views_tile_64"][1] == small


def test_counts_above_16_bits(device_results):
    num, row_start, col, count, path = device_results["two_views_share_70000_points"][0]
    assert count[0] == 70000 and col[0] == 1 and num[0] == 70000


def test_refused_before_any_launch(gpu_ctx):
    lib = gpu_ctx.lib
    from line3d_amd.capi import _p
    out = [C.c_void_p() for _ in range(4)]
    path = C.c_int(0)
    ids = np.zeros(4, np.uint32)

    def call(ids_p, start, n_lists, outs=None, path_p=None):
        s = None if start is None else np.ascontiguousarray(start, np.int64)
        outs = [C.byref(o) for o in out] if outs is None else outs
        return lib.l3d_covisibility(gpu_ctx.h, ids_p, None if s is None else _p(s), C.c_int(n_lists), *outs, C.byref(path) if path_p is None else path_p)

    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    assert call(_p(ids), [0, 2 ** 31 - 1], 1) == 5          # L3D_ERR_UNSUPPORTED: 2^31 - 1 observations or more (point_ids is not read)
    assert call(_p(ids), [0, 2 ** 40], 1) == 5
    assert call(None, [0, 3], 1) == 1                       # L3D_ERR_INVALID: observations without ids
    assert call(_p(ids), None, 1) == 1
    assert call(_p(ids), [0, 3], 1, outs=[C.byref(out[0]), None, C.byref(out[2]), C.byref(out[3])]) == 1
    assert call(_p(ids), [0, 3], 1, path_p=C.c_void_p()) == 1
    assert call(_p(ids), [0, 3, 2], 2) == 1                 # offsets descend
    assert call(_p(ids), [1, 3], 1) == 1
    assert call(_p(ids), [0], -1) == 1
    assert lib.l3d_covisibility(None, _p(ids), _p(np.array([0, 3], np.int64)), C.c_int(1), *[C.byref(o) for o in out], C.byref(path)) == 1
    assert all(o.value is None for o in out)
    assert not any(v[0] for v in gpu_ctx.profile_all().values()), "a refusal launched something"
    gpu_ctx.profile_enable(False)
    # no observations at all: an empty result, nothing to launch
    num, row_start, col, count, p = gpu_ctx.covisibility([[], []])
    assert num.tolist() == [0, 0] and row_start.tolist() == [0, 0, 0] and len(col) == 0 and len(count) == 0 and p == 0
