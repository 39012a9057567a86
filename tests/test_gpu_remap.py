"""Undistortion onto another size with a validity plane on the device (k_det_undistort_remap, l3d_undistort.hip) against the contract of
include/line3d_amd.h ("A REMAP") as tests/remap_model.py states it: pixels AND validity byte for byte, no pixel left out.  The margins that make
this exact for the fisheye cases are checked without a device (tests/test_remap_cases_cpu.py).  Then the planner's camera through the call, the
kernels launched, and the refusals."""
import numpy as np
import pytest

import remap_model as rm
from line3d_amd import capi

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _lens(case):
    return capi.lens(case["model"], case["coeffs"], camera=case["src_cam"])


@pytest.fixture(scope="module")
def models():
    """the model's result per case, computed once"""
    return [(c,) + rm.case_image(c) + (rm.case_model(c),) for c in rm.CASES]


def _same(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, "%s: %d bytes differ, first at %s: device %s, model %s" % (what, len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])


@pytest.mark.parametrize("k", range(len(rm.CASES)), ids=lambda k: rm.CASES[k]["name"])
def test_kernel_equals_model(gpu_ctx, models, k):
    import torch
    case, view, img, mask, m = models[k]
    w, h, ch = case["size"][:3]
    K, lens, out_size = _K(*case["out_cam"]), _lens(case), case["out_size"]
    # a larger image of another content first: what it leaves in the buffers must not show
    big = np.random.default_rng(100 + k).integers(0, 256, size=(h + 19, w + 45, 3), dtype=np.uint8)
    gpu_ctx.undistort(big, _K(50.0, 50.0, (w + 45) / 2.0, (h + 19) / 2.0), lens=capi.lens("fisheye", [0.01]), out_size=(w + 50, h + 30),
                      mask=np.zeros((h + 19, w + 45), np.uint8), return_mask=True)
    # host pixels (the padded-row case: a view into padded rows)
    got, valid = gpu_ctx.undistort(view, K, lens=lens, out_size=out_size, mask=mask, return_mask=True)
    _same(got, m["image"], "host, pixels")
    _same(valid, m["valid"], "host, validity")
    _same(gpu_ctx.undistort(view, K, lens=lens, out_size=out_size, mask=mask), m["image"], "host, no plane asked for")
    # device in, device out; the mask from device memory as well
    t = torch.from_numpy(img.copy()).cuda()
    tm = None if mask is None else torch.from_numpy(mask.copy()).cuda()
    out, dvalid = gpu_ctx.undistort(t, K, lens=lens, out_size=out_size, mask=tm, return_mask=True)
    _same(out.cpu().numpy(), m["image"], "device, pixels")
    _same(dvalid.cpu().numpy(), m["valid"], "device, validity")
    assert np.array_equal(t.cpu().numpy(), img)
    if mask is not None:
        # host pixels with the device mask, device pixels with the host mask; a padded mask
        _same(gpu_ctx.undistort(view, K, lens=lens, out_size=out_size, mask=tm, return_mask=True)[1], m["valid"], "host pixels, device mask")
        _same(gpu_ctx.undistort(t, K, lens=lens, out_size=out_size, mask=mask, return_mask=True)[1].cpu().numpy(), m["valid"], "device pixels, host mask")
        wide = torch.zeros((h, w + 13), dtype=torch.uint8, device="cuda")
        wide[:, :w] = tm
        _same(gpu_ctx.undistort(view, K, lens=lens, out_size=out_size, mask=wide[:, :w], return_mask=True)[1], m["valid"], "padded device mask")
        # border_mask off: the caller's mask alone
        only = rm.remap(img, out_size, case["out_cam"], case["model"], case["src_cam"], case["coeffs"], mask=mask, border_mask=False)
        got, valid = gpu_ctx.undistort(view, K, lens=lens, out_size=out_size, mask=mask, border_mask=False, return_mask=True)
        _same(got, m["image"], "border_mask off, pixels")
        _same(valid, only["valid"], "border_mask off, validity")


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_planned_camera_through_the_call(gpu_ctx, alpha):
    """capi.undistort_plan's K and size go into the call; at alpha 0 no pixel is invalid, at alpha 1 some are and the source's corners are seen"""
    rng = np.random.default_rng(3)
    src_cam, co, size = (70.0, 71.0, 60.3, 44.8), [-0.03, 0.008, -0.002, 0.0005], (120, 90)
    img = rng.integers(1, 256, size=(size[1], size[0]), dtype=np.uint8)
    lens = capi.lens("fisheye", co, camera=src_cam)
    for out_size in (None, "keep_focal", (64, 50)):
        K, wh = capi.undistort_plan(lens, size, alpha, out_size, max_dim=200)
        got, valid = gpu_ctx.undistort(img, K, lens=lens, out_size=wh, return_mask=True)
        m = rm.remap(img, wh, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), rm.FISHEYE, src_cam, co)
        if m["tie_margin"].min() >= 1e-7 and m["limit_distance"].min() >= 1e-7:            # (the margin of the table's cases, where this camera has it)
            _same(got, m["image"], "pixels")
            _same(valid, m["valid"], "validity")
        assert got.shape == (wh[1], wh[0])
        assert (valid == 0).sum() == 0 if alpha == 0.0 else (valid == 0).mean() > 0.02
        assert got[valid == 255].min() >= 1                                                  # a valid pixel shows the image (which has no 0)


def test_launches(gpu_ctx):
    img = np.random.default_rng(4).integers(0, 256, size=(40, 56, 3), dtype=np.uint8)
    cam = (40.0, 40.0, 28.0, 20.0)
    K, mask = _K(*cam), rm.case_mask(56, 40)
    names = ("k_det_undistort_remap", "k_det_undistort_lens", "k_det_undistort")
    gpu_ctx.profile_enable(True)
    try:
        def count(call):
            gpu_ctx.profile_reset()
            out = call()
            return out, tuple(gpu_ctx.profile_get(n)[0] for n in names)
        # no lens, a mask: nothing is resampled, the mask is the plane
        (got, valid), n = count(lambda: gpu_ctx.undistort(img, K, mask=mask, return_mask=True))
        assert n == (0, 0, 0) and got.tobytes() == img.tobytes() and np.array_equal(valid, np.where(mask, 255, 0))
        # a pinhole lens, equal cameras and sizes: nothing is launched either
        for lens in (capi.lens("brown", [0.0] * 8, camera=cam), capi.lens(0, [], camera=cam), capi.lens("brown", [1e-13])):
            (got, valid), n = count(lambda: gpu_ctx.undistort(img, K, lens=lens, mask=mask, return_mask=True))
            assert n == (0, 0, 0) and got.tobytes() == img.tobytes() and np.array_equal(valid, np.where(mask, 255, 0))
        # ... another size, or another camera: the pinhole resample, through the new kernel
        (got, valid), n = count(lambda: gpu_ctx.undistort(img, K, lens=capi.lens(0, [], camera=cam), out_size=(70, 40), return_mask=True))
        assert n == (1, 0, 0)
        assert got[:, :56].tobytes() == img.tobytes() and not got[:, 56:].any() and valid[:, :56].min() == 255 and not valid[:, 56:].any()
        _, n = count(lambda: gpu_ctx.undistort(img, _K(40.0, 40.0, 28.5, 20.0), lens=capi.lens(0, [], camera=cam), return_mask=True))
        assert n == (1, 0, 0)
        # a lens alone keeps its kernel, and the k1, k2 call its own
        _, n = count(lambda: gpu_ctx.undistort(img, K, lens=capi.lens("fisheye", [0.01])))
        assert n == (0, 1, 0)
        _, n = count(lambda: gpu_ctx.undistort(img, K, 0.1, 0.0))
        assert n == (0, 0, 1)
        # the same lens with a plane asked for: the new kernel, the same pixels
        want = gpu_ctx.undistort(img, K, lens=capi.lens("brown", [0.3]))               # (pincushion: the rim looks past the source)
        (got, valid), n = count(lambda: gpu_ctx.undistort(img, K, lens=capi.lens("brown", [0.3]), return_mask=True))
        assert n == (1, 0, 0) and got.tobytes() == want.tobytes() and 0 < (valid == 0).sum() < valid.size
    finally:
        gpu_ctx.profile_enable(False)


def _refused(gpu_ctx, call, code):
    names = ("k_det_undistort_remap", "k_det_undistort_lens", "k_det_undistort", "k_det_grey", "k_det_ingest", "k_det_egress", "k_det_valid_from_mask")
    before = {k: gpu_ctx.profile_get(k)[0] for k in names}
    with pytest.raises(capi.L3DError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert {k: gpu_ctx.profile_get(k)[0] for k in before} == before          # nothing was launched
    return str(e.value)


def test_refusals(gpu_ctx):
    import torch
    img = np.random.default_rng(5).integers(0, 256, size=(40, 56), dtype=np.uint8)
    t = torch.from_numpy(img.copy()).cuda()
    cam = (40.0, 40.0, 28.0, 20.0)
    K, good = _K(*cam), capi.lens("fisheye", [0.01], camera=cam)
    gpu_ctx.profile_enable(True)
    try:
        for im in (img, t):
            # an output size without a lens
            assert "needs a lens" in _refused(gpu_ctx, lambda: gpu_ctx.undistort(im, K, out_size=(60, 40), return_mask=True), INVALID)
            # what A LENS refuses
            _refused(gpu_ctx, lambda: gpu_ctx.undistort(im, K, lens=capi.lens(3, [0.1]), out_size=(60, 40)), INVALID)
            _refused(gpu_ctx, lambda: gpu_ctx.undistort(im, K, lens=capi.lens("brown", [float("nan")]), return_mask=True), INVALID)
            _refused(gpu_ctx, lambda: gpu_ctx.undistort(im, _K(0.0, 40.0, 28.0, 20.0), lens=good, return_mask=True), INVALID)
            # output sizes: half given, negative, too large
            for bad in ((60, 0), (0, 40), (-1, -1)):
                _refused(gpu_ctx, lambda: gpu_ctx.undistort(im, K, lens=good, out_size=bad), INVALID)
        _refused(gpu_ctx, lambda: gpu_ctx.undistort(img, K, lens=good, out_size=((1 << 24) + 1, 8)), UNSUPPORTED)
        # the mask: extent and memory kind, the checks of l3d_device_image
        # a dedicated allocation (past everything the caching allocator keeps in one block, after the cache was emptied) and rows so far apart that
        # the 40th lies past its end
        torch.cuda.empty_cache()
        big = torch.ones(48 << 20, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r = capi.remap(good, mask=big[:40 * 56].view(40, 56))
        r.mask_row_stride = (48 << 20) // 20
        out, valid = np.zeros_like(img), np.zeros_like(img)
        import ctypes as C
        pix, w, h, ch, stride = capi.image_arguments(img)

        def raw(rr):
            gpu_ctx._chk(gpu_ctx.lib.l3d_undistort_image_remap(gpu_ctx.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), C.c_double(40.0), C.c_double(40.0),
                                                               C.c_double(28.0), C.c_double(20.0), C.byref(rr), out.ctypes.data_as(C.c_void_p), C.c_size_t(w),
                                                               valid.ctypes.data_as(C.c_void_p), C.c_size_t(w)))
        assert "allocation" in _refused(gpu_ctx, lambda: raw(r), INVALID)
        host = np.ones((40, 56), np.uint8)
        r2 = capi.remap(good, mask=host)
        r2.mask_on_device = 1                                                  # host memory passed off as device memory
        assert "not device memory" in _refused(gpu_ctx, lambda: raw(r2), INVALID)
        r3 = capi.remap(good, mask=host)
        r3.mask_row_stride = 55
        assert "row stride" in _refused(gpu_ctx, lambda: raw(r3), INVALID)
        # a mask of another extent than the source: the library refuses it from the extent the remap states, before it reads a byte -- host pixels
        # (past the binding's own check), device pixels, with and without a lens
        small = np.ones((39, 56), np.uint8)
        assert "the mask is 56 x 39" in _refused(gpu_ctx, lambda: raw(capi.remap(good, mask=small)), INVALID)
        assert "the mask is 56 x 39" in _refused(gpu_ctx, lambda: raw(capi.remap(None, mask=small)), INVALID)
        for m in (small, np.ones((40, 57), np.uint8), torch.ones((41, 56), dtype=torch.uint8, device="cuda")):
            assert "the mask is" in _refused(gpu_ctx, lambda: gpu_ctx.undistort(t, K, lens=good, mask=m, return_mask=True), INVALID)
            assert "the mask is" in _refused(gpu_ctx, lambda: gpu_ctx.undistort(t, K, mask=m, return_mask=True), INVALID)
    finally:
        gpu_ctx.profile_enable(False)
    with pytest.raises(ValueError):
        gpu_ctx.undistort(img, K, lens=good, mask=np.ones((41, 56), np.uint8))          # the binding's shape check
    with pytest.raises(ValueError):
        gpu_ctx.undistort(img, K, 0.1, 0.0, out_size=(60, 40))
