"""The one check behind every undistortion (warp_check, line3d_amd/csrc/l3d_undistort.hip) through l3d_test_undistort_route: no context, no device.
Which kernel an image needs (0 none, 1 k_det_undistort, 2 k_det_undistort_lens, 3 k_det_undistort_remap), whether it carries a validity plane and
the size the detector sees, for a table of entries.  The expected values are written here from the TEXT of include/line3d_amd.h ("Undistortion on
the device", "A LENS", "A REMAP"; the sentence is quoted beside each row), not from the code.  Then every refusal those sections list, with the
codes -- and, where they assert one, the message fragments -- of tests/test_gpu_lens.py::test_refusals, tests/test_gpu_remap.py::test_refusals and
tests/test_gpu_remap_detect.py::test_refusals_in_a_batch, built the way those tests build them."""
import numpy as np
import pytest

from line3d_amd import capi

INVALID, UNSUPPORTED = 1, 5
NONE, RADIAL, LENS, RESAMPLE = 0, 1, 2, 3
W, H = 56, 40
CAM = (40.0, 40.0, 28.0, 20.0)          # the output camera: the entry's camera with k1 = k2 = 0
OTHER = (41.0, 40.0, 28.0, 20.0)        # a source camera that differs from it
MASK = np.ones((H, W), np.uint8)
FISH = ("fisheye", [0.01])


def _route(camera, lens=None, remap=None, size=(W, H)):
    return capi.undistort_route(camera, lens, remap, size)


# name, camera, lens, remap (keywords of capi.remap, or None), expected route, plane, output size
TABLE = [
    # "Undistortion on the device": both |k1| and |k2| <= 1e-12: nothing is launched, the pixels pass through untouched
    ("no camera", None, None, None, NONE, 0, (W, H)),
    ("k1 = k2 = 0", CAM + (0.0, 0.0), None, None, NONE, 0, (W, H)),
    ("|k| = 1e-12", CAM + (1e-12, -1e-12), None, None, NONE, 0, (W, H)),
    ("k1 just above 1e-12", CAM + (1.0000001e-12, 0.0), None, None, RADIAL, 0, (W, H)),
    ("k2 just above 1e-12", CAM + (0.0, -1.0000001e-12), None, None, RADIAL, 0, (W, H)),
    # "A LENS", pass-through: a BROWN lens whose eight coefficients all lie within 1e-12, with equal cameras, launches nothing.  fx == 0 && fy == 0
    # in the lens says "the output camera".  A FISHEYE lens is always active
    ("BROWN all zero, the output camera", CAM + (0.0, 0.0), capi.lens("brown", [0.0] * 8), None, NONE, 0, (W, H)),
    ("BROWN all zero, an equal camera", CAM + (0.0, 0.0), capi.lens("brown", [0.0] * 8, camera=CAM), None, NONE, 0, (W, H)),
    ("BROWN 1e-12 eight times", CAM + (0.0, 0.0), capi.lens("brown", [1e-12, -1e-12] * 4), None, NONE, 0, (W, H)),
    ("BROWN p2 just above 1e-12", CAM + (0.0, 0.0), capi.lens("brown", [0.0, 0.0, 0.0, 1.0000001e-12]), None, LENS, 0, (W, H)),
    ("BROWN all zero, another source camera", CAM + (0.0, 0.0), capi.lens("brown", [0.0] * 8, camera=OTHER), None, LENS, 0, (W, H)),
    ("FISHEYE all zero", CAM + (0.0, 0.0), capi.lens("fisheye", [0.0] * 4), None, LENS, 0, (W, H)),
    # "A REMAP", l3d_remap.lens NULL: nothing is resampled, the mask is the validity plane (out size: 0 or the source's)
    ("remap: no lens, a mask", CAM + (0.0, 0.0), None, dict(mask=MASK), NONE, 1, (W, H)),
    ("remap: no lens, no camera, a mask", None, None, dict(mask=MASK), NONE, 1, (W, H)),
    ("remap: no lens, a mask, the source size spelled out", CAM + (0.0, 0.0), None, dict(mask=MASK, out_size=(W, H)), NONE, 1, (W, H)),
    ("remap: nothing at all", CAM + (0.0, 0.0), None, dict(), NONE, 0, (W, H)),
    # model 0, or BROWN with every coefficient within 1e-12: a pinhole camera -- with the cameras and the sizes equal nothing is launched, otherwise
    # the image is resampled through the same kernel.  THE RESAMPLING: beside the pixel the kernel writes one byte of validity
    ("remap: model 0 at the source size", CAM + (0.0, 0.0), capi.lens(0, [], camera=CAM), dict(), NONE, 0, (W, H)),
    ("remap: model 0 at the source size, a mask", CAM + (0.0, 0.0), capi.lens(0, [], camera=CAM), dict(mask=MASK), NONE, 1, (W, H)),
    ("remap: BROWN 1e-13 at the source size", CAM + (0.0, 0.0), capi.lens("brown", [1e-13]), dict(), NONE, 0, (W, H)),
    ("remap: model 0 at another size", CAM + (0.0, 0.0), capi.lens(0, [], camera=CAM), dict(out_size=(70, 40)), RESAMPLE, 1, (70, 40)),
    ("remap: model 0 at another size, border_mask 0", CAM + (0.0, 0.0), capi.lens(0, [], camera=CAM), dict(out_size=(70, 40), border_mask=False), RESAMPLE, 1, (70, 40)),
    ("remap: model 0, another camera", (40.0, 40.0, 28.5, 20.0, 0.0, 0.0), capi.lens(0, [], camera=CAM), dict(), RESAMPLE, 1, (W, H)),
    # a remap that asks for nothing (a lens alone, border_mask 0, no mask, the source's size) is the ..._lens call
    ("remap: a lens alone, border_mask 0", CAM + (0.0, 0.0), capi.lens(*FISH), dict(border_mask=False), LENS, 0, (W, H)),
    ("remap: a lens alone, border_mask 0, (0, 0)", CAM + (0.0, 0.0), capi.lens(*FISH), dict(border_mask=False, out_size=(0, 0)), LENS, 0, (W, H)),
    ("remap: a lens alone, border_mask 1", CAM + (0.0, 0.0), capi.lens(*FISH), dict(border_mask=True), RESAMPLE, 1, (W, H)),
    ("remap: a lens and a mask, border_mask 0", CAM + (0.0, 0.0), capi.lens(*FISH), dict(mask=MASK, border_mask=False), RESAMPLE, 1, (W, H)),
    ("remap: a lens, border_mask 0, another size", CAM + (0.0, 0.0), capi.lens(*FISH), dict(border_mask=False, out_size=(64, 50)), RESAMPLE, 1, (64, 50)),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r[0])
def test_route(row):
    _, camera, lens, remap, route, plane, out = row
    if remap is None:
        got = _route(camera, lens)
    else:                                           # the lens of a remap travels inside it, as in the ..._batch_remap calls
        got = _route(camera, None, capi.remap(lens, **remap))
    assert got == (0, "", route, plane, out), got


def _refused(code, fragment, camera, lens=None, remap=None, size=(W, H)):
    rc, msg, route, plane, out = _route(camera, lens, remap, size)
    assert rc == code and msg and fragment in msg, (rc, msg)
    assert route == NONE and plane == 0             # a refused entry asks for no kernel


def test_refusals_of_a_lens():
    """tests/test_gpu_lens.py::test_refusals, its list of lenses and output cameras"""
    nan, inf = float("nan"), float("inf")
    out = CAM + (0.0, 0.0)
    bad = [capi.lens(0, [0.1]), capi.lens(3, [0.1]), capi.Lens(),                                            # unknown model; a zeroed struct
           capi.lens("brown", [0.1, nan]), capi.lens("fisheye", [inf]), capi.lens("brown", [0.1], camera=(nan, 250.0, 160.0, 100.0)),
           capi.lens("brown", [0.1], camera=(250.0, 250.0, 160.0, inf)),                                     # a field that is not finite
           capi.lens("brown", [0.1], camera=(250.0, 0.0, 160.0, 100.0)), capi.lens("fisheye", [], camera=(0.0, 250.0, 160.0, 100.0)),   # exactly one of fx, fy zero
           capi.lens("fisheye", [0.1, 0, 0, 0, 1e-3]), capi.lens("fisheye", [0.1, 0, 0, 0, 0, 0, 0, -1e-300])]   # k[4..7] on a fisheye
    for lens in bad:
        _refused(INVALID, "lens:", out, lens)
    good = capi.lens(*FISH, camera=CAM)
    # the output camera: fx', fy' finite and not zero; a lens without a camera has none
    for cam in ((0.0, 40.0, 28.0, 20.0, 0.0, 0.0), (40.0, nan, 28.0, 20.0, 0.0, 0.0), None):
        _refused(INVALID, "fx and fy", cam, good)
    # the k1, k2 camera's own
    _refused(INVALID, "fx and fy", (0.0, 40.0, 28.0, 20.0, 0.1, 0.0))
    # coefficients beside a lens
    _refused(INVALID, "both", CAM + (-0.1, 0.01), good)
    _refused(INVALID, "both", CAM + (0.0, 1e-300), good)


def test_refusals_of_a_remap():
    """tests/test_gpu_remap.py::test_refusals and tests/test_gpu_remap_detect.py::test_refusals_in_a_batch"""
    out = CAM + (0.0, 0.0)
    good = capi.lens(*FISH, camera=CAM)
    # an output size without a lens
    _refused(INVALID, "needs a lens", out, None, capi.remap(None, out_size=(60, 40)))
    _refused(INVALID, "needs a lens", None, None, capi.remap(None, out_size=(300, 200)))
    # what A LENS refuses
    _refused(INVALID, "lens:", out, None, capi.remap(capi.lens(3, [0.1]), out_size=(60, 40)))
    _refused(INVALID, "lens:", out, None, capi.remap(capi.lens("brown", [float("nan")])))
    _refused(INVALID, "fx and fy", (0.0, 40.0, 28.0, 20.0, 0.0, 0.0), None, capi.remap(good))
    _refused(INVALID, "fx and fy", None, None, capi.remap(good))
    # output sizes: half given, negative, too large
    for bad in ((60, 0), (0, 40), (-1, -1)):
        _refused(INVALID, "output size", out, None, capi.remap(good, out_size=bad))
    _refused(UNSUPPORTED, "too large", out, None, capi.remap(good, out_size=((1 << 24) + 1, 8)))
    # the mask: its row stride, and an extent other than the source's -- with and without a lens
    r3 = capi.remap(good, mask=MASK)
    r3.mask_row_stride = W - 1
    _refused(INVALID, "row stride", out, None, r3)
    small = np.ones((H - 1, W), np.uint8)
    _refused(INVALID, "the mask is %d x %d" % (W, H - 1), out, None, capi.remap(good, mask=small))
    _refused(INVALID, "the mask is %d x %d" % (W, H - 1), out, None, capi.remap(None, mask=small))
    _refused(INVALID, "the mask is", out, None, capi.remap(good, mask=np.ones((H, W + 1), np.uint8)))
    # coefficients, or a lens of its own, beside a remap: refused before anything else of the remap is looked at
    _refused(INVALID, "beside", CAM + (0.1, 0.0), None, capi.remap(good, out_size=(60, 40)))
    _refused(INVALID, "beside", out, good, capi.remap(good))
    _refused(INVALID, "beside", CAM + (0.1, 0.0), None, capi.remap(None, out_size=(60, 0)))

