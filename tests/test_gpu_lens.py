"""Undistortion with a lens on the device (k_det_undistort_lens, l3d_undistort.hip) against the contract of include/line3d_amd.h ("A LENS") as
tests/lens_model.py states it: byte for byte, no pixel left out.  The margins that make this exact for the fisheye cases are checked without a
device (tests/test_lens_cases_cpu.py).  Then the wiring into the detector, single and batched, the dispatch between the two undistortion
kernels, and the refusals."""
import os

import numpy as np
import pytest

import lens_model as lm
import undistort_model as um
from line3d_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ref.npz")
INVALID, UNSUPPORTED = 1, 5


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _lens(case):
    return capi.lens(case["model"], case["coeffs"], camera=case["src_cam"])


@pytest.fixture(scope="module")
def models():
    """the model's result per case, computed once"""
    return [(c,) + lm.case_image(c) + (lm.case_model(c),) for c in lm.CASES]


def _same(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = np.argwhere(got != want)
    assert len(diff) == 0, "%s: %d pixels differ, first at %s: device %s, model %s" % (what, len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])


@pytest.mark.parametrize("k", range(len(lm.CASES)), ids=lambda k: lm.CASES[k]["name"])
def test_kernel_equals_model(gpu_ctx, models, k):
    case, view, img, m = models[k]
    w, h, ch = case["size"][:3]
    K, lens = _K(*case["out_cam"]), _lens(case)
    # a larger image of another content first: what it leaves in the buffers must not show
    big = np.random.default_rng(100 + k).integers(0, 256, size=(h + 19, w + 45, 3), dtype=np.uint8)
    gpu_ctx.undistort(big, _K(50.0, 50.0, (w + 45) / 2.0, (h + 19) / 2.0), lens=capi.lens("fisheye", [0.01]))
    _same(gpu_ctx.undistort(view, K, lens=lens), m["image"], "host")                  # (the padded-row case: a view into padded rows)
    if case["claim"] == "identity":
        assert gpu_ctx.undistort(view, K, lens=lens).tobytes() == img.tobytes()
    # in place, on the array with its own row stride; the padding stays
    pad = case["size"][3]
    base = np.full((h, w * ch + pad), 77, np.uint8)
    base[:, :w * ch] = img.reshape(h, w * ch)
    own = np.lib.stride_tricks.as_strided(base, shape=view.shape, strides=(w * ch + pad,) + view.strides[1:])
    back = gpu_ctx.undistort(own, K, lens=lens, in_place=True)
    assert back is own
    _same(own, m["image"], "in place")
    if case["size"][3]:
        assert (base[:, w * ch:] == 77).all()
    # device in, device out (k_det_egress), and in place on the device
    import torch
    t = torch.from_numpy(img.copy()).cuda()
    out = gpu_ctx.undistort(t, K, lens=lens)
    _same(out.cpu().numpy(), m["image"], "device")
    assert np.array_equal(t.cpu().numpy(), img)
    assert gpu_ctx.undistort(t, K, lens=lens, in_place=True) is t
    _same(t.cpu().numpy(), m["image"], "device, in place")


@pytest.mark.parametrize("k", range(len(um.CASES)), ids=lambda k: "%dx%dx%d_k%g_%g" % (um.CASES[k][:3] + um.CASES[k][8:]))
def test_brown_k1_k2_equals_the_existing_call(gpu_ctx, k):
    """every case of undistort_model.CASES as BROWN (k1, k2, 0 ...): the bytes of undistort(img, K, k1, k2) -- with the lens's camera left to the
    output camera and with it given"""
    case = um.CASES[k]
    view, _ = um.case_image(case)
    K = _K(*case[4:8])
    want = gpu_ctx.undistort(view, K, case[8], case[9])
    assert gpu_ctx.undistort(view, K, lens=capi.lens("brown", case[8:10])).tobytes() == want.tobytes()
    assert gpu_ctx.undistort(view, K, lens=capi.lens(capi.LENS_BROWN, list(case[8:10]) + [0.0] * 6, camera=case[4:8])).tobytes() == want.tobytes()


def test_pass_through_launches_nothing(gpu_ctx):
    _, img = um.case_image(um.CASES[3])
    K = _K(70.0, 70.0, 48.0, 40.0)
    gpu_ctx.profile_enable(True)
    try:
        gpu_ctx.profile_reset()
        got = gpu_ctx.undistort(img, K, lens=capi.lens("brown", [1e-13, 0, -1e-12, 0, 0, 1e-12]))
        got2 = gpu_ctx.undistort(img, K, lens=capi.lens("brown", [0.0] * 8, camera=(70.0, 70.0, 48.0, 40.0)))
        assert gpu_ctx.profile_get("k_det_undistort_lens")[0] == 0 and gpu_ctx.profile_get("k_det_undistort")[0] == 0
        assert got.tobytes() == img.tobytes() == got2.tobytes()
        # equal coefficients, another camera: active.  A fisheye without coefficients: active
        a = gpu_ctx.undistort(img, K, lens=capi.lens("brown", [0.0] * 8, camera=(70.0, 70.0, 48.5, 40.0)))
        b = gpu_ctx.undistort(img, K, lens=capi.lens("fisheye", []))
        assert gpu_ctx.profile_get("k_det_undistort_lens")[0] == 2 and gpu_ctx.profile_get("k_det_undistort")[0] == 0
        assert a.tobytes() != img.tobytes() and b.tobytes() != img.tobytes()
    finally:
        gpu_ctx.profile_enable(False)


# ---- wiring into the detector: images of the add tests' scene (320 x 200, decoded from tests/golden/jpeg_ref.npz)
@pytest.fixture(scope="module")
def images(gpu_ctx):
    g = np.load(GOLDEN)
    files = [g["view%d/bytes" % k].tobytes() for k in range(4)]
    return files, [gpu_ctx.decode_jpeg(d) for d in files]


OUT = (250.0, 250.0, 160.0, 100.0)
BROWN8 = ("brown", [-0.2, 0.03, 0.004, -0.003, 0.01, 0.02, -0.01, 0.005], None)
FISH = ("fisheye", [-0.03, 0.01, -0.002, 0.0004], (300.0, 300.0, 158.0, 101.5))
DIST = (-0.2, 0.03)


def test_detect_with_lens_equals_undistort_then_detect(gpu_ctx, images):
    files, imgs = images
    K = _K(*OUT)
    plain = gpu_ctx.detect_segments(imgs[0])
    for model, coeffs, cam in (BROWN8, FISH):
        lens = capi.lens(model, coeffs, camera=cam)
        und = gpu_ctx.undistort(imgs[0], K, lens=lens)
        want = gpu_ctx.detect_segments(und)
        got = gpu_ctx.detect_segments(imgs[0], camera=OUT, lens=lens)
        assert len(want) > 0 and got.tobytes() == want.tobytes() and got.tobytes() != plain.tobytes()
        # rescaled: the undistortion runs at the full size, before the rescale.  From the file, and from device memory
        assert gpu_ctx.detect_segments(imgs[0], new_size=(240, 150), camera=OUT, lens=lens).tobytes() == gpu_ctx.detect_segments(und, new_size=(240, 150)).tobytes()
        assert gpu_ctx.detect_segments_jpeg(files[0], camera=OUT, lens=lens).tobytes() == want.tobytes()
        import torch
        assert gpu_ctx.detect_segments(torch.from_numpy(imgs[0].copy()).cuda(), camera=OUT, lens=lens).tobytes() == want.tobytes()
    # a lens that carries its camera needs none beside it: the image is undistorted onto the lens's own camera
    lens = capi.lens(*FISH[:2], camera=FISH[2])
    assert gpu_ctx.detect_segments(imgs[0], lens=lens).tobytes() == gpu_ctx.detect_segments(gpu_ctx.undistort(imgs[0], _K(*FISH[2]), lens=lens)).tobytes()
    with pytest.raises(ValueError):
        gpu_ctx.detect_segments(imgs[0], lens=capi.lens(*BROWN8[:2]))


def test_batch_mixes_models_in_one_chunk(gpu_ctx, images):
    """a BROWN image, a FISHEYE image, a k1-k2 camera and a plain image in one chunk: the four single calls; the chunk launches the new kernel once"""
    files, imgs = images
    lenses = [capi.lens(*BROWN8[:2], camera=BROWN8[2]), capi.lens(*FISH[:2], camera=FISH[2]), None, None]
    cameras = [OUT, OUT, OUT + DIST, None]
    single = [gpu_ctx.detect_segments(imgs[0], camera=OUT, lens=lenses[0]), gpu_ctx.detect_segments(imgs[1], camera=OUT, lens=lenses[1]),
              gpu_ctx.detect_segments(imgs[2], camera=OUT + DIST), gpu_ctx.detect_segments(imgs[3])]
    assert len({s.tobytes() for s in single}) == 4 and min(len(s) for s in single) > 0
    gpu_ctx.profile_enable(True)
    try:
        for batch in (imgs, [imgs[0], files[1], imgs[2], files[3]]):
            gpu_ctx.profile_reset()
            got = gpu_ctx.detect_segments_batch(batch, cameras=cameras, lenses=lenses)
            assert (gpu_ctx.profile_get("k_det_undistort_lens")[0], gpu_ctx.profile_get("k_det_undistort")[0], gpu_ctx.profile_get("k_det_region")[0]) == (1, 0, 3)
            assert [g.tobytes() for g in got] == [s.tobytes() for s in single]
        import torch
        gpu_ctx.profile_reset()
        got = gpu_ctx.detect_segments_batch([torch.from_numpy(im.copy()).cuda() for im in imgs], cameras=cameras, lenses=lenses)
        assert (gpu_ctx.profile_get("k_det_undistort_lens")[0], gpu_ctx.profile_get("k_det_undistort")[0], gpu_ctx.profile_get("k_det_ingest")[0]) == (1, 0, 1)
        assert [g.tobytes() for g in got] == [s.tobytes() for s in single]
        # a chunk of k1-k2 cameras only (and a plain image): the existing kernel, and it alone -- also through the ..._lens entry point
        gpu_ctx.profile_reset()
        got = gpu_ctx.detect_segments_batch([imgs[2], imgs[2], imgs[3]], cameras=[OUT + DIST, OUT + DIST, None])
        assert (gpu_ctx.profile_get("k_det_undistort_lens")[0], gpu_ctx.profile_get("k_det_undistort")[0]) == (0, 1)
        assert [g.tobytes() for g in got] == [single[2].tobytes(), single[2].tobytes(), single[3].tobytes()]
        gpu_ctx.profile_reset()
        zero = capi.lens("brown", [0.0] * 8)             # a lens that passes the pixels through: the chunk still has no lens
        got = gpu_ctx.detect_segments_batch([imgs[2], imgs[3]], cameras=[OUT + DIST, OUT], lenses=[None, zero])
        assert (gpu_ctx.profile_get("k_det_undistort_lens")[0], gpu_ctx.profile_get("k_det_undistort")[0]) == (0, 1)
        assert [g.tobytes() for g in got] == [single[2].tobytes(), single[3].tobytes()]
    finally:
        gpu_ctx.profile_enable(False)


def _refused(gpu_ctx, call, code):
    before = {k: gpu_ctx.profile_get(k)[0] for k in ("k_det_undistort_lens", "k_det_undistort", "k_det_grey", "k_det_ingest", "k_det_egress")}
    with pytest.raises(capi.L3DError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert {k: gpu_ctx.profile_get(k)[0] for k in before} == before          # nothing was launched
    return str(e.value)


def test_refusals(gpu_ctx, images):
    _, imgs = images
    img = imgs[0]
    K = _K(*OUT)
    nan, inf = float("nan"), float("inf")
    bad = [capi.lens(0, [0.1]), capi.lens(3, [0.1]), capi.Lens(),                                            # unknown model; a zeroed struct
           capi.lens("brown", [0.1, nan]), capi.lens("fisheye", [inf]), capi.lens("brown", [0.1], camera=(nan, 250.0, 160.0, 100.0)),
           capi.lens("brown", [0.1], camera=(250.0, 250.0, 160.0, inf)),                                     # a field that is not finite
           capi.lens("brown", [0.1], camera=(250.0, 0.0, 160.0, 100.0)), capi.lens("fisheye", [], camera=(0.0, 250.0, 160.0, 100.0)),   # exactly one of fx, fy zero
           capi.lens("fisheye", [0.1, 0, 0, 0, 1e-3]), capi.lens("fisheye", [0.1, 0, 0, 0, 0, 0, 0, -1e-300])]   # k[4..7] on a fisheye
    import torch
    t = torch.from_numpy(img.copy()).cuda()
    gpu_ctx.profile_enable(True)
    try:
        for lens in bad:
            _refused(gpu_ctx, lambda: gpu_ctx.undistort(img, K, lens=lens), INVALID)
            _refused(gpu_ctx, lambda: gpu_ctx.undistort(t, K, lens=lens), INVALID)
            _refused(gpu_ctx, lambda: gpu_ctx.detect_segments(img, camera=OUT, lens=lens), INVALID)
            _refused(gpu_ctx, lambda: gpu_ctx.detect_segments(t, camera=OUT, lens=lens), INVALID)
        good = capi.lens(*FISH[:2], camera=FISH[2])
        # the output camera: fx', fy' finite and not zero
        for Kb in (_K(0.0, 250.0, 160.0, 100.0), _K(250.0, nan, 160.0, 100.0)):
            _refused(gpu_ctx, lambda: gpu_ctx.undistort(img, Kb, lens=good), INVALID)
            _refused(gpu_ctx, lambda: gpu_ctx.detect_segments(img, camera=(Kb[0, 0], Kb[1, 1], 160.0, 100.0), lens=good), INVALID)
        # coefficients beside a lens
        assert "both" in _refused(gpu_ctx, lambda: gpu_ctx.detect_segments(img, camera=OUT + DIST, lens=good), INVALID)
        # in a batch a refused entry fails alone
        got, status = gpu_ctx.detect_segments_batch([img, img, img], cameras=[OUT, OUT + DIST, OUT], lenses=[bad[0], good, good], return_status=True)
        assert status == [INVALID, INVALID, 0] and len(got[0]) == 0 and len(got[1]) == 0
        assert got[2].tobytes() == gpu_ctx.detect_segments(img, camera=OUT, lens=good).tobytes()
    finally:
        gpu_ctx.profile_enable(False)
    with pytest.raises(ValueError):
        gpu_ctx.undistort(img, K, 0.1, 0.0, lens=good)
    # a skewed K with an active lens, where a K is taken: the object-level calls (tests/test_gpu_add_lens.py)
