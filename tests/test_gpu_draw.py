"""l3d_draw_segments / l3d_draw_segments_device (k_draw_pieces, k_draw_scan, k_draw_cover, k_draw_resolve) on the case table of tests/draw_cases.py:
host pixels and device images come back byte for byte as the model of tests/draw_model.py and the host entry point l3d_test_draw_segments_host leave
them -- device layouts H x W x C, C x H x W, a cropped view, a flipped view with a negative row stride and a chan map of {2, 1, 0}; the key plane is
back to all zeros after every call (two draws in a row equal two fresh contexts), also when it grows; the launches are the four named kernels
whatever the number of segments; and every refusal is answered before anything is launched."""
import numpy as np
import pytest

import draw_cases as dc
import draw_model as dm

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in dc.CASES]
KERNELS = ("draw_pieces", "draw_scan", "draw_cover", "draw_resolve")


def args(case):
    return case["segments"], case["colors"], case["color_index"], case["width_px"], case["opacity"]


@pytest.fixture(scope="module")
def device_results(gpu_ctx):
    """every case once on the device, one after the other on one context, host pixels, with every profiled launch counted"""
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    out = {c["name"]: gpu_ctx.draw_segments(c["image"], *args(c)) for c in dc.CASES}
    launches = {k: v[0] for k, v in gpu_ctx.profile_all().items()}
    gpu_ctx.profile_enable(False)
    return out, launches


def test_the_kernels_launched_are_the_named_ones(device_results):
    out, launches = device_results
    calls = sum(1 for c in dc.CASES if len(c["segments"]) > 0)
    drawn = sum(1 for c in dc.CASES if len(c["segments"]) > 0 and dm.key_plane(np.asarray(c["image"]).shape[:2], c["segments"], c["width_px"]).any())
    assert launches["draw_pieces"] == calls and launches["draw_scan"] == calls, "one count and one scan launch per call with segments"
    assert drawn <= launches["draw_cover"] == launches["draw_resolve"] <= calls, "one cover and one resolve launch per call whose pieces reach the image"
    assert {k for k, n in launches.items() if n} == set(KERNELS), "another kernel was launched"


@pytest.mark.parametrize("name", NAMES)
def test_host_pixels_equal_model_and_twin(device_results, name):
    from line3d_amd import capi
    case = dc.BY_NAME[name]
    got = device_results[0][name]
    assert got.dtype == np.uint8 and got.shape == np.asarray(case["image"]).shape
    assert np.array_equal(got, dc.model_of(case)), name
    assert np.array_equal(got, capi.draw_segments_host(case["image"], *args(case))), name
    if got.base is not None and got.base.ndim == 2 and got.base.shape[1] > got.shape[1]:      # rows with padding: every padding byte as it was
        assert np.all(got.base[:, got.shape[1]:] == 0xA5)


DEVICE_NAMES = ["width_2_5", "width_64_0", "y_major_reversed", "fan_4097", "alpha_modulo", "opacity_200", "color_index", "crosses_every_border", "four_channels",
                "one_channel_padded", "steps_129", "steps_65_y_major", "no_segments", "wholly_outside"]


@pytest.mark.parametrize("name", DEVICE_NAMES)
def test_device_images_in_every_layout(gpu_ctx, name):
    import torch
    from line3d_amd import capi
    case = dc.BY_NAME[name]
    img = np.ascontiguousarray(case["image"])
    want = dc.model_of(case)
    h, w = img.shape[:2]
    # H x W (x C)
    t = torch.from_numpy(img).to("cuda:0")
    assert gpu_ctx.draw_segments(t, *args(case)) is t
    assert np.array_equal(t.cpu().numpy(), want), "HWC"
    if img.ndim == 3:
        # C x H x W
        t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to("cuda:0")
        gpu_ctx.draw_segments(t, *args(case), layout="CHW")
        assert np.array_equal(t.cpu().numpy().transpose(1, 2, 0), want), "CHW"
        # colour component k into channel chan[k]: the model on the image with its first three channels reversed
        rev = img.copy()
        rev[..., :3] = img[..., 2::-1]
        t = torch.from_numpy(img).to("cuda:0")
        gpu_ctx.draw_segments(t, *args(case), chan=(2, 1, 0))
        want_rev = dm.draw(rev, *args(case))
        got = t.cpu().numpy()
        assert np.array_equal(got[..., 2::-1], want_rev[..., :3]) and np.array_equal(got[..., 3:], img[..., 3:]), "chan"
    # a cropped view: the pixels around it stay
    big = np.full((h + 9, w + 12) + img.shape[2:], 0x5A, np.uint8)
    big[4:4 + h, 7:7 + w] = img
    t = torch.from_numpy(big).to("cuda:0")
    gpu_ctx.draw_segments(t[4:4 + h, 7:7 + w], *args(case))
    got = t.cpu().numpy()
    assert np.array_equal(got[4:4 + h, 7:7 + w], want), "crop"
    got[4:4 + h, 7:7 + w] = 0x5A
    assert np.all(got == 0x5A), "crop: a pixel outside the view changed"
    # a flipped view: the descriptor starts at the last row and its rows go up
    t = torch.from_numpy(np.ascontiguousarray(img[::-1])).to("cuda:0")
    d = capi.device_image(t)
    d.ptr = t.data_ptr() + (h - 1) * d.stride_y
    d.stride_y = -d.stride_y
    gpu_ctx.draw_segments(d, *args(case))
    assert np.array_equal(t.cpu().numpy()[::-1], want), "flipped"


def test_two_draws_in_a_row_equal_two_fresh_contexts(gpu_ctx, device_results):
    from line3d_amd import capi
    a, b = dc.BY_NAME["width_64_0"], dc.BY_NAME["fan_4097"]
    first = gpu_ctx.draw_segments(a["image"], *args(a))
    second = gpu_ctx.draw_segments(b["image"], *args(b))
    for case, got in ((a, first), (b, second)):
        fresh = capi.Context(0)
        try:
            assert np.array_equal(fresh.draw_segments(case["image"], *args(case)), got), case["name"]
        finally:
            fresh.close()
    # the second draw on the first one's result: were a key left in the plane, it would be blended again
    twice = gpu_ctx.draw_segments(first, *args(b))
    assert np.array_equal(twice, dm.draw(first, *args(b)))


def test_the_plane_grows_with_the_image(gpu_ctx):
    rng = np.random.default_rng(9)
    small = dc.BY_NAME["width_9_0"]
    ctx_images = [(small["image"], small["segments"]), (rng.integers(0, 256, (200, 300, 3), dtype=np.uint8), np.array([[-10, -5, 310, 190], [150, 3, 150.5, 197], [2, 100, 298, 101]], np.float32)),
                  (small["image"], small["segments"]), (rng.integers(0, 256, (333, 517), dtype=np.uint8), np.array([[3, 3, 500, 300], [500, 10, 20, 330]], np.float32))]
    from line3d_amd import capi
    ctx = capi.Context(0)
    try:
        for img, segs in ctx_images:
            got = ctx.draw_segments(img, segs, dc.PAL, None, 9.0, 230)
            assert np.array_equal(got, dm.draw(img, segs, dc.PAL, None, 9.0, 230)), img.shape
    finally:
        ctx.close()


def test_launches_do_not_depend_on_n(gpu_ctx):
    gpu_ctx.profile_enable(True)
    try:
        counts = []
        for name in ("horizontal_integer_y", "alpha_modulo", "fan_4097"):
            case = dc.BY_NAME[name]
            gpu_ctx.profile_reset()
            gpu_ctx.draw_segments(case["image"], *args(case))
            counts.append([gpu_ctx.profile_get(k)[0] for k in KERNELS])
        assert counts == [[1, 1, 1, 1]] * 3
    finally:
        gpu_ctx.profile_enable(False)


def test_refusals_launch_nothing(gpu_ctx, device_results):
    import torch
    from line3d_amd import capi
    gpu_ctx.profile_enable(True)
    gpu_ctx.profile_reset()
    try:
        for _, overrides, code, word in dc.REFUSALS:
            kw = dc.refusal_arguments(overrides)
            with pytest.raises(capi.L3DError, match="error %d" % code) as e:
                gpu_ctx.draw_segments(kw["image"], kw["segments"], kw["colors"], kw["color_index"], kw["width_px"], kw["opacity"])
            assert word in str(e.value), str(e.value)
        good = dc.refusal_arguments({})
        tail = (good["segments"], good["colors"], None, 1.0, 255)
        # a device image of another dtype; a descriptor over host memory; a descriptor whose stated height leaves its allocation
        f32 = torch.zeros((48, 64, 3), dtype=torch.float32, device="cuda:0")
        with pytest.raises(capi.L3DError, match="error 5"):
            gpu_ctx.draw_segments(f32, *tail)
        host = np.zeros((48, 64, 3), np.uint8)
        d = capi.device_image(torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda:0"))
        d.ptr = host.ctypes.data
        with pytest.raises(capi.L3DError, match="not device memory"):
            gpu_ctx.draw_segments(d, *tail)
        t = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda:0")
        d = capi.device_image(t)
        d.height = 1 << 15
        with pytest.raises(capi.L3DError, match="allocation"):
            gpu_ctx.draw_segments(d, *tail)
        assert all(gpu_ctx.profile_get(k)[0] == 0 for k in KERNELS), "a refusal launched a kernel"
        gpu_ctx.draw_segments(t, *tail)
        assert np.array_equal(t.cpu().numpy(), dm.draw(np.zeros((48, 64, 3), np.uint8), *tail))
        assert [gpu_ctx.profile_get(k)[0] for k in KERNELS] == [1, 1, 1, 1]
    finally:
        gpu_ctx.profile_enable(False)
