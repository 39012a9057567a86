"""The validity plane through the detector (k_det_valid_*, l3d_detect.hip; "A REMAP" in include/line3d_amd.h): the defined / undefined plane at the
working resolution against tests/remap_model.py byte for byte; the invariant that what invalid pixels hold cannot reach the segments; and the reason
for the feature -- the rim of an undistorted fisheye image yields segments without the plane and none with it.  The scene is the test's own: bright
polygons with straight edges in the IDEAL view on a texture too faint for the gradient threshold, seen through an equidistant fisheye."""
import numpy as np
import pytest

import remap_model as rm
from line3d_amd import capi

pytestmark = pytest.mark.gpu

SIZE = (320, 240)
SRC_CAM = (196.0, 197.5, 160.3, 119.8)          # an equidistant fisheye (no coefficients: theta_d = theta, the inverse is closed-form)
POLYGONS = [                                      # convex, in ideal normalised coordinates, well inside the view
    ([(-0.70, -0.45), (-0.15, -0.55), (-0.10, -0.10), (-0.60, 0.00)], 215),
    ([(0.10, -0.50), (0.65, -0.35), (0.50, 0.05), (0.15, -0.05)], 180),
    ([(-0.55, 0.15), (-0.05, 0.10), (0.05, 0.50), (-0.45, 0.55)], 235),
    ([(0.20, 0.15), (0.70, 0.20), (0.60, 0.55), (0.25, 0.50)], 200),
]


def _scene(seed=11, noise=2):
    """the distorted image: per source pixel the ideal direction (xd, yd) tan(theta) / theta, painted with the polygon it falls into"""
    w, h = SIZE
    fx, fy, cx, cy = SRC_CAM
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xd, yd = (j - cx) / fx, (i - cy) / fy
    th = np.sqrt(xd * xd + yd * yd)
    s = np.where(th > 1e-8, np.tan(np.minimum(th, 1.5)) / np.where(th > 1e-8, th, 1.0), 1.0)
    x, y = xd * s, yd * s
    img = 100.0 + np.random.default_rng(seed).integers(-noise, noise + 1, size=(h, w))
    for pts, level in POLYGONS:
        inside = np.ones((h, w), bool)
        for (ax, ay), (bx, by) in zip(pts, pts[1:] + pts[:1]):
            inside &= (bx - ax) * (y - ay) - (by - ay) * (x - ax) >= 0.0
        img = np.where(inside & (th < 1.2), float(level), img)
    return img.astype(np.uint8)


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _near(invalid, radius):
    """pixels within `radius` (Euclidean, pixel centres) of an invalid pixel"""
    h, w = invalid.shape
    r = int(np.ceil(radius))
    pad = np.zeros((h + 2 * r, w + 2 * r), bool)
    pad[r:r + h, r:r + w] = invalid
    out = np.zeros((h, w), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy <= radius * radius:
                out |= pad[r + dy:r + dy + h, r + dx:r + dx + w]
    return out


def _hugs(segs, near):
    """per segment: every sample along it (half-pixel steps) lies at a pixel of `near`, or off the image"""
    h, w = near.shape
    res = []
    for x1, y1, x2, y2 in np.asarray(segs, np.float64):
        n = max(2, int(2.0 * np.hypot(x2 - x1, y2 - y1)) + 1)
        t = np.linspace(0.0, 1.0, n)
        px, py = np.rint(x1 + t * (x2 - x1)).astype(int), np.rint(y1 + t * (y2 - y1)).astype(int)
        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        res.append(bool(np.all(near[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)] | ~ok)))
    return np.array(res, bool)


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    """the image, the lens, the planner's camera at alpha 1, the model's undistorted image and plane -- and the checks that the scene is what the
    tests below need, made once"""
    img = _scene()
    lens = capi.lens("fisheye", [], camera=SRC_CAM)
    K, wh = capi.undistort_plan(lens, SIZE, 1.0)
    assert wh == SIZE
    cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    m = rm.remap(img, wh, cam, rm.FISHEYE, SRC_CAM, ())
    assert m["tie_margin"].min() >= 1e-7 and m["limit_distance"].min() >= 1e-7          # the margins of the table's cases: the device's plane is the model's
    share = float((m["valid"] == 0).mean())
    assert 0.05 <= share <= 0.60, share
    return dict(img=img, lens=lens, K=K, cam=cam, und=m["image"], valid=m["valid"])


def _plane(gpu_ctx):
    d = gpu_ctx.test_detect_defined_plane()
    assert d is not None
    return d


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, "%s: %d bytes differ, first at %s: device %s, model %s" % (what, len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])


@pytest.mark.parametrize("new_size", [None, (200, 150), (161, 120)], ids=["full", "rescaled", "rescaled_odd"])
def test_defined_plane_equals_model(gpu_ctx, scene, new_size):
    w, h = SIZE
    img = scene["img"]
    # a blank rim: the fisheye at alpha 1, through the resampling kernel
    gpu_ctx.detect_segments(img, new_size=new_size, camera=scene["cam"], lens=scene["lens"], out_size=SIZE)
    want = rm.defined_plane(scene["valid"], new_size)
    assert 0 < (want == 0).sum() < want.size
    _same(_plane(gpu_ctx), want, "rim")
    # the caller's masks, no lens: a one-pixel hole; a hole touching each edge (the samplers' symmetric boundary); an all-invalid image
    masks = {"one_pixel": np.ones((h, w), np.uint8), "left": np.ones((h, w), np.uint8), "right": np.ones((h, w), np.uint8), "top": np.ones((h, w), np.uint8),
             "bottom": np.ones((h, w), np.uint8), "corner_pixel": np.ones((h, w), np.uint8), "nothing": np.zeros((h, w), np.uint8)}
    masks["one_pixel"][97, 143] = 0
    masks["left"][50:53, 0:2] = 0
    masks["right"][120:122, w - 1] = 0
    masks["top"][0, 200:203] = 0
    masks["bottom"][h - 2:h, 31] = 0
    masks["corner_pixel"][h - 1, w - 1] = 0
    for name, mask in masks.items():
        segs = gpu_ctx.detect_segments(img, new_size=new_size, mask=mask)
        want = rm.defined_plane(mask, new_size)
        _same(_plane(gpu_ctx), want, name)
        if name == "nothing":
            assert want.max() == 0 and len(segs) == 0                                  # an all-invalid image: no segments, and no error
        else:
            assert 0 < (want == 0).sum() < 400, (name, int((want == 0).sum()))         # a hole is a few footprints, not the image
    # no plane: the hook says so
    gpu_ctx.detect_segments(img, new_size=new_size)
    assert gpu_ctx.test_detect_defined_plane() is None


def test_an_all_valid_plane_changes_nothing(gpu_ctx, scene):
    img = scene["img"]
    want = gpu_ctx.detect_segments(img)
    assert len(want) >= 10
    assert gpu_ctx.detect_segments(img, mask=np.ones(img.shape, np.uint8)).tobytes() == want.tobytes()
    assert gpu_ctx.detect_segments(img, new_size=(200, 150), mask=np.full(img.shape, 7, np.uint8)).tobytes() == gpu_ctx.detect_segments(img, new_size=(200, 150)).tobytes()
    # a lens with border_mask off and no mask is the lens alone
    a = gpu_ctx.detect_segments(img, camera=scene["cam"], lens=scene["lens"], border_mask=False)
    assert a.tobytes() == gpu_ctx.detect_segments(img, camera=scene["cam"], lens=scene["lens"]).tobytes()


def _fills(base, invalid, seed=3):
    noise = np.random.default_rng(seed).integers(0, 256, size=base.shape, dtype=np.uint8)
    return [np.where(invalid, fill, base).astype(np.uint8) for fill in (0, 255, noise)]


@pytest.mark.parametrize("new_size", [None, (200, 150)], ids=["full", "rescaled"])
def test_what_invalid_pixels_hold_cannot_reach_the_segments(gpu_ctx, scene, new_size):
    """THE INVARIANT: with a validity plane the segments are byte-identical whether the invalid pixels hold 0, 255 or noise"""
    und, valid = scene["und"], scene["valid"]
    # the fisheye rim: the undistorted image with its plane as the caller's mask, the blank pixels refilled
    direct = gpu_ctx.detect_segments(scene["img"], new_size=new_size, camera=scene["cam"], lens=scene["lens"], out_size=SIZE)
    rim = [gpu_ctx.detect_segments(f, new_size=new_size, mask=valid) for f in _fills(und, valid == 0)]
    assert len(direct) >= 10 and all(r.tobytes() == direct.tobytes() for r in rim)
    # without the plane the fill decides the result
    assert len({gpu_ctx.detect_segments(f, new_size=new_size).tobytes() for f in _fills(und, valid == 0)}) == 3
    # a mask of the caller's through a polygon's middle (ideal view): a band across the first polygon
    band = np.ones(und.shape, np.uint8)
    ys, xs = np.nonzero(und == POLYGONS[0][1])
    band[(ys.min() + ys.max()) // 2 - 3:(ys.min() + ys.max()) // 2 + 4, xs.min() - 5:xs.max() + 6] = 0
    through = [gpu_ctx.detect_segments(f, new_size=new_size, mask=band) for f in _fills(und, band == 0)]
    assert len(through[0]) >= 10 and all(t.tobytes() == through[0].tobytes() for t in through)
    assert through[0].tobytes() != gpu_ctx.detect_segments(und, new_size=new_size).tobytes()
    # inside a batch chunk: the three fills of the rim and of the band together, beside an image without a plane
    imgs = _fills(und, valid == 0) + _fills(und, band == 0) + [und]
    masks = [valid] * 3 + [band] * 3 + [None]
    gpu_ctx.profile_enable(True)
    try:
        gpu_ctx.profile_reset()
        got = gpu_ctx.detect_segments_batch(imgs, new_sizes=[new_size] * 7, masks=masks)
        # one chunk; the masks alone launch no resampling
        assert gpu_ctx.profile_get("k_det_grad")[0] == 1 and gpu_ctx.profile_get("k_det_valid_apply")[0] == 1
        assert gpu_ctx.profile_get("k_det_undistort_remap")[0] == 0 and gpu_ctx.profile_get("k_det_valid_grey")[0] == (0 if new_size is None else 1)
    finally:
        gpu_ctx.profile_enable(False)
    assert all(g.tobytes() == direct.tobytes() for g in got[:3]) and all(g.tobytes() == through[0].tobytes() for g in got[3:6])
    assert got[6].tobytes() == gpu_ctx.detect_segments(und, new_size=new_size).tobytes()


def test_the_rim_yields_segments_without_the_plane_and_none_with_it(gpu_ctx, scene):
    """THE REASON FOR THE FEATURE, on the zero-filled fisheye image.  'At the rim': every sample of the segment lies within the footprint distance
    (remap_model.footprint_distance, an upper bound on how far from an invalid pixel a gradient pixel can be undefined) of a blank pixel."""
    und, valid = scene["und"], scene["valid"]
    near = _near(valid == 0, rm.footprint_distance(SIZE))
    without = gpu_ctx.detect_segments(und)
    with_plane = gpu_ctx.detect_segments(scene["img"], camera=scene["cam"], lens=scene["lens"], out_size=SIZE)
    assert _hugs(without, near).sum() >= 1, "the scene's rim yields no segment"
    assert _hugs(with_plane, near).sum() == 0
    assert len(with_plane) >= 10
    assert len(with_plane) < len(without)
    # the same through a smaller planned view (the output size differs from the source's)
    K, wh = capi.undistort_plan(scene["lens"], SIZE, 1.0, (240, 180))
    cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    und2, valid2 = gpu_ctx.undistort(scene["img"], K, lens=scene["lens"], out_size=wh, return_mask=True)
    near2 = _near(valid2 == 0, rm.footprint_distance(wh))
    a = gpu_ctx.detect_segments(und2)
    b = gpu_ctx.detect_segments(scene["img"], camera=cam, lens=scene["lens"], out_size=wh)
    assert _hugs(a, near2).sum() >= 1 and _hugs(b, near2).sum() == 0 and len(b) >= 10
    assert b.tobytes() == gpu_ctx.detect_segments(und2, mask=valid2).tobytes()         # undistorting first and passing the plane on is the same thing
    assert b[:, [0, 2]].max() < wh[0] and b[:, [1, 3]].max() < wh[1]                   # segments in pixels of the output


def test_a_chunk_mixes_a_remap_a_lens_a_camera_and_a_plain_image(gpu_ctx, scene):
    """the four single calls' bytes; the chunk goes through the resampling kernel once and through no other"""
    img = scene["img"]
    cam, lens = scene["cam"], scene["lens"]
    dist = tuple(cam) + (-0.2, 0.03)
    single = [gpu_ctx.detect_segments(img, camera=cam, lens=lens, out_size=SIZE), gpu_ctx.detect_segments(img, camera=cam, lens=lens),
              gpu_ctx.detect_segments(img, camera=dist), gpu_ctx.detect_segments(img)]
    assert len({s.tobytes() for s in single}) == 4 and min(len(s) for s in single) > 0
    names = ("k_det_undistort_remap", "k_det_undistort_lens", "k_det_undistort", "k_det_valid_apply", "k_det_region")
    gpu_ctx.profile_enable(True)
    try:
        import torch
        for batch in ([img] * 4, [torch.from_numpy(img.copy()).cuda() for _ in range(4)]):
            gpu_ctx.profile_reset()
            got = gpu_ctx.detect_segments_batch(batch, cameras=[cam, cam, dist, None], lenses=[lens, lens, None, None], out_sizes=[SIZE, None, None, None])
            assert tuple(gpu_ctx.profile_get(n)[0] for n in names) == (1, 0, 0, 1, 3)
            assert [g.tobytes() for g in got] == [s.tobytes() for s in single]
        # a chunk without a remap launches none of the new kernels
        gpu_ctx.profile_reset()
        got = gpu_ctx.detect_segments_batch([img] * 3, cameras=[cam, dist, None], lenses=[lens, None, None])
        assert [g.tobytes() for g in got] == [s.tobytes() for s in single[1:]]
        new = ("k_det_undistort_remap", "k_det_valid_from_mask", "k_det_valid_grey", "k_det_valid_x", "k_det_valid_y", "k_det_valid_apply")
        assert all(gpu_ctx.profile_get(n)[0] == 0 for n in new) and gpu_ctx.profile_get("k_det_undistort_lens")[0] == 1
        # another output size: a chunk of its own
        gpu_ctx.profile_reset()
        K, wh = capi.undistort_plan(lens, SIZE, 0.5, (240, 180))
        cam2 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        got = gpu_ctx.detect_segments_batch([img] * 3, cameras=[cam, cam2, None], lenses=[lens, lens, None], out_sizes=[SIZE, wh, None])
        # (the plain image has the first remap's sizes and shares its chunk; the smaller output runs alone)
        assert gpu_ctx.profile_get("k_det_grad")[0] == 2 and gpu_ctx.profile_get("k_det_undistort_remap")[0] == 2
        assert got[0].tobytes() == single[0].tobytes() and got[2].tobytes() == single[3].tobytes()
        assert got[1].tobytes() == gpu_ctx.detect_segments(img, camera=cam2, lens=lens, out_size=wh).tobytes() and len(got[1]) > 0
    finally:
        gpu_ctx.profile_enable(False)


def test_refusals_in_a_batch(gpu_ctx, scene):
    img, cam, lens = scene["img"], scene["cam"], scene["lens"]
    good = gpu_ctx.detect_segments(img, camera=cam, lens=lens, out_size=SIZE)
    # an output size without a lens; coefficients beside a remap; an output below 8 x 8: each fails alone
    got, status = gpu_ctx.detect_segments_batch([img] * 4, cameras=[None, tuple(cam) + (0.1, 0.0), cam, cam], lenses=[None, lens, lens, lens],
                                                out_sizes=[(300, 200), SIZE, (7, 100), SIZE], return_status=True)
    assert status == [1, 1, 1, 0] and got[3].tobytes() == good.tobytes() and all(len(g) == 0 for g in got[:3])
    with pytest.raises(ValueError):
        gpu_ctx.detect_segments(img, mask=np.ones((10, 10), np.uint8))
