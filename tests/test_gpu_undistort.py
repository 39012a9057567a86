"""Undistortion on the device (k_det_undistort, l3d_undistort.hip) against the contract of include/line3d_amd.h as tests/undistort_model.py states
it: byte for byte.  The margins that make this exact are checked without a device (tests/test_undistort_cpu.py).  Then the wiring into the
detector and into addImage (exact), and one agreement test of the geometry through the detector, held to the bar of tests/test_gpu_detect.py.

Measured on an MI355X (the agreement test prints them): see DESIGN.md 4f."""
import os

import numpy as np
import pytest

import detect_metric as dm
import undistort_model as um
from line3d_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_ref.npz")


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


# ---- exact: kernel against model
@pytest.fixture(scope="module")
def models():
    """the model's result per case, computed once"""
    out = []
    for case in um.CASES:
        view, img = um.case_image(case)
        out.append((case, view, um.undistort(img, *case[4:])))
    return out


def test_table_covers_its_categories(models):
    outside = sum(int((~m["inside"]).sum()) for _, _, m in models)
    partial = sum(int(m["partial"].sum()) for _, _, m in models)
    x0neg = sum(int(m["x0_negative"].sum()) for _, _, m in models)
    all_inside = sum(1 for c, _, m in models if m["inside"].all() and not m["partial"].any() and (c[8] or c[9]))
    padded = sum(1 for c, _, _ in models if c[3])
    print("outside %d, partial %d, x0 < 0: %d, cases all inside %d, padded %d" % (outside, partial, x0neg, all_inside, padded))
    assert outside > 0 and partial > 0 and x0neg > 0 and all_inside > 0 and padded > 0
    assert any(-(-c[0] // 32) > 1 for c, _, _ in models) and any(-(-c[1] // 8) > 1 for c, _, _ in models)      # more than one block each way
    assert {c[2] for c, _, _ in models} == {1, 3}


@pytest.mark.parametrize("k", range(len(um.CASES)), ids=lambda k: "%dx%dx%d_k%g_%g" % (um.CASES[k][:3] + um.CASES[k][8:]))
def test_kernel_equals_model(gpu_ctx, models, k):
    case, view, m = models[k]
    w, h, ch = case[:3]
    # a larger image of another content first: what it leaves in the buffers must not show
    big = np.random.default_rng(100 + k).integers(0, 256, size=(h + 19, w + 45, 3), dtype=np.uint8)
    gpu_ctx.undistort(big, _K(50.0, 50.0, (w + 45) / 2.0, (h + 19) / 2.0), 0.2, 0.0)
    got = gpu_ctx.undistort(view, _K(*case[4:8]), case[8], case[9])
    assert got.shape == m["image"].shape and got.dtype == np.uint8
    diff = np.argwhere(got != m["image"])
    assert len(diff) == 0, "%d pixels differ, first at %s: device %s, model %s" % (len(diff), diff[0], got[tuple(diff[0])], m["image"][tuple(diff[0])])
    if not (case[8] or case[9]):
        assert got.tobytes() == np.ascontiguousarray(view).tobytes()


def test_extreme_coefficients(gpu_ctx):
    _, img = um.case_image(um.CASES[3])
    K = _K(70.0, 70.0, 48.0, 40.0)
    got = gpu_ctx.undistort(img, K, 1e6, 0.0)            # coordinates up to 1e8 px: the range test comes before the integer conversion
    assert np.array_equal(got, um.undistort(img, 70.0, 70.0, 48.0, 40.0, 1e6, 0.0)["image"])
    assert np.argwhere(got.any(axis=-1)).tolist() == [[40, 48]]
    for k1, k2 in ((float("nan"), 0.0), (0.1, float("nan")), (float("inf"), 0.0)):
        got = gpu_ctx.undistort(img, K, k1, k2)
        assert np.array_equal(got, um.undistort(img, 70.0, 70.0, 48.0, 40.0, k1, k2)["image"])
        assert not got.any()


def test_argument_errors(gpu_ctx):
    img = np.zeros((16, 16), np.uint8)
    for K in (_K(0.0, 10.0, 8.0, 8.0), _K(10.0, float("nan"), 8.0, 8.0), _K(float("inf"), 10.0, 8.0, 8.0)):
        with pytest.raises(capi.L3DError):
            gpu_ctx.undistort(img, K, 0.1, 0.0)
        with pytest.raises(capi.L3DError):
            gpu_ctx.detect_segments(img, camera=(K[0, 0], K[1, 1], 8.0, 8.0, 0.1, 0.0))
    with pytest.raises(capi.L3DError):
        gpu_ctx.undistort(np.zeros((16, 16, 2), np.uint8), _K(10.0, 10.0, 8.0, 8.0), 0.1, 0.0)
    one = np.array([[200]], np.uint8)                    # 1 x 1 is enough here
    assert gpu_ctx.undistort(one, _K(1.0, 1.0, 0.0, 0.0), 0.5, 0.0)[0, 0] == 200


# ---- exact: wiring
def _draw(width, height, segs):
    """3-px dark strokes on a light ground, anti-aliased by the distance to the segment (as in tests/test_gpu_detect.py)"""
    img = np.full((height, width), 210.0)
    for x1, y1, x2, y2 in np.asarray(segs, np.float64):
        x0, xe = int(max(0, min(x1, x2) - 4)), int(min(width, max(x1, x2) + 5))
        y0, ye = int(max(0, min(y1, y2) - 4)), int(min(height, max(y1, y2) + 5))
        yy, xx = np.mgrid[y0:ye, x0:xe].astype(np.float64)
        d = np.array([x2 - x1, y2 - y1])
        L = np.hypot(*d)
        d /= L
        a = np.clip((xx - x1) * d[0] + (yy - y1) * d[1], 0, L)
        dist = np.hypot(xx - (x1 + a * d[0]), yy - (y1 + a * d[1]))
        img[y0:ye, x0:xe] = np.minimum(img[y0:ye, x0:xe], 210.0 - 170.0 * np.clip(2.0 - dist, 0, 1))
    return np.rint(img).astype(np.uint8)


def _model_bytes(l3d, scene, n_segs):
    parts = []
    for v in scene.views:
        parts.append(np.array([l3d.getSegment2D(v["id"], s) for s in range(n_segs[v["id"]])], np.float32).tobytes())
        parts.append(l3d.view_matches(v["id"])[0].tobytes())
    lines = l3d.getResult()
    for seg2, seg3 in lines:
        parts.append(np.array(sorted((int(c), int(s)) for c, s in seg2), np.int64).tobytes())
        parts.append(np.array([np.concatenate(p) for p in seg3], np.float64).tobytes())
    return b"".join(parts), len(lines)


DIST = (-0.2, 0.03)


@pytest.fixture(scope="module")
def wiring(gpu_ctx):
    """6 views of 320 x 200; every image is taken as a distorted one: (scene, images, undistorted images, their segments)"""
    from line3d_amd.synth import make_scene
    scene = make_scene(6, 30, 6, seed=11, noise_px=0.0, width=320, height=200, f=250.0, seg_len=(0.3, 0.8))
    images = {v["id"]: _draw(320, 200, v["segments"]) for v in scene.views}
    undist = {v["id"]: gpu_ctx.undistort(images[v["id"]], v["K"], *DIST) for v in scene.views}
    detected = {i: gpu_ctx.detect_segments(img) for i, img in undist.items()}
    assert min(len(s) for s in detected.values()) > 0
    return scene, images, undist, detected


def test_detect_with_camera_equals_undistort_then_detect(gpu_ctx, wiring):
    scene, images, undist, detected = wiring
    for v in scene.views[:3]:
        K = v["K"]
        assert not np.array_equal(undist[v["id"]], images[v["id"]])
        cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) + DIST
        got = gpu_ctx.detect_segments(images[v["id"]], camera=cam)
        assert got.tobytes() == detected[v["id"]].tobytes()
        assert got.tobytes() != gpu_ctx.detect_segments(images[v["id"]]).tobytes()
    # rescaled, and three channels: the undistortion runs at the full size, before the rescale
    v = scene.views[0]
    K = v["K"]
    cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) + DIST
    rgb = np.stack([images[v["id"]], 255 - images[v["id"]], images[v["id"]] // 2], axis=-1)
    a = gpu_ctx.detect_segments(rgb, new_size=(240, 150), camera=cam)
    b = gpu_ctx.detect_segments(gpu_ctx.undistort(rgb, K, *DIST), new_size=(240, 150))
    assert len(a) > 0 and a.tobytes() == b.tobytes()
    # coefficients within 1e-12: the plain call
    assert gpu_ctx.detect_segments(images[v["id"]], camera=cam[:4] + (0.0, 1e-13)).tobytes() == gpu_ctx.detect_segments(images[v["id"]]).tobytes()


def test_add_image_pixels_with_dist_equals_undistort_then_add(gpu_ctx, wiring, tmp_path):
    from line3d_amd.pipeline import Line3D
    scene, images, undist, detected = wiring
    n_segs = {i: len(s) for i, s in detected.items()}

    def run(add, directory=tmp_path, **kw):
        l3d = Line3D(str(directory) + os.sep, matchingNeighbors=6, **kw)
        try:
            if not kw:
                l3d.keep_view_matches(True)
            for v in scene.views:
                assert add(l3d, v)
            assert l3d.numCameras() == len(scene.views)
            if kw:          # a node object: the views themselves
                return b"".join(np.array([l3d.getSegment2D(v["id"], s) for s in range(n_segs[v["id"]])], np.float32).tobytes() for v in scene.views), 0
            l3d.compute3Dmodel(False)
            return _model_bytes(l3d, scene, n_segs)
        finally:
            l3d.close()

    caches = lambda: sorted(f for f in os.listdir(tmp_path) if f.startswith("segments_"))
    ref, n_lines = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], undist[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False))
    print("wiring scene: %d views, %d..%d segments per view, %d bytes of segments and matches, %d 3-D lines"
          % (len(scene.views), min(n_segs.values()), max(n_segs.values()), len(ref), n_lines))
    got, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False, dist=DIST))
    assert got == ref
    assert caches() == []
    plain, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False))
    assert plain != ref                                   # (the coefficients matter)
    zero, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False, dist=(0.0, 0.0)))
    assert zero == plain
    # cache rules: written once, then a present cache stands in for the pixels
    got, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=True, dist=DIST))
    assert got == ref
    written = caches()
    assert len(written) == len(scene.views)
    stamps = [os.stat(os.path.join(tmp_path, f)).st_mtime_ns for f in written]
    blank = {i: np.full_like(img, 128) for i, img in images.items()}
    got, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], blank[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=True, dist=DIST))
    assert got == ref
    assert caches() == written and [os.stat(os.path.join(tmp_path, f)).st_mtime_ns for f in written] == stamps
    # world-point links take the same path
    l3d = Line3D(str(tmp_path / "wp") + os.sep, matchingNeighbors=4)
    try:
        v = scene.views[0]
        assert l3d.add_image_pixels(v["id"], images[v["id"]], v["K"], v["R"], v["t"], [1, 2, 3], loadAndStoreSegments=False, dist=DIST)
        assert np.array([l3d.getSegment2D(v["id"], s) for s in range(n_segs[v["id"]])], np.float32).tobytes() == detected[v["id"]].tobytes()
        # a skewed K with coefficients is refused, and the object goes on
        Ks = v["K"].copy()
        Ks[0, 1] = 0.5
        w = scene.views[1]
        assert not l3d.add_image_pixels(w["id"], images[w["id"]], Ks, w["R"], w["t"], [1, 2, 3], loadAndStoreSegments=False, dist=DIST)
        assert "skew" in l3d.lib.l3d_line3d_last_error(l3d.h).decode() and l3d.numCameras() == 1
        assert l3d.add_image_pixels(w["id"], images[w["id"]], w["K"], w["R"], w["t"], [1, 2, 3], loadAndStoreSegments=False, dist=DIST)
        assert l3d.numCameras() == 2
    finally:
        l3d.close()
    # a node object (two ranks on one device) adds the same views
    one, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False, dist=DIST), device=0)
    node, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False, dist=DIST), devices=[0, 0])
    assert node == one == b"".join(detected[v["id"]].tobytes() for v in scene.views)


def test_reconstruct_from_images_accepts_distorted_cameras(gpu_ctx, wiring, tmp_path):
    """the drivers' flow over a scene whose cameras have distortion; reconstruct() still refuses them and names the way"""
    from line3d_amd import sfm
    scene, images, undist, detected = wiring
    cams = [dict(name="img%d.jpg" % v["id"], focal=250.0, dist=np.array([-DIST[0], 0.0]), cv_dist=np.array(DIST), R=v["R"], t=v["t"],
                 worldpoints=np.arange(10, dtype=np.uint32)) for v in scene.views]
    s = sfm.SfmScene(cams, 10)
    assert np.array_equal(sfm.intrinsics(250.0, 320, 200), scene.views[0]["K"])
    ids = [v["id"] for v in scene.views]
    seen = []

    def load(i, name):
        seen.append((i, name))
        return images[ids[i]]
    with pytest.raises(RuntimeError, match="reconstruct_from_images"):
        sfm.reconstruct(s, [detected[i] for i in ids], [(320, 200)] * len(ids))
    l3d = sfm.reconstruct_from_images(s, load, str(tmp_path) + os.sep, out_dir=str(tmp_path / "out"), neighbors=4, load_and_store_segments=False)
    try:
        assert seen == [(k, "img%d.jpg" % i) for k, i in enumerate(ids)] and l3d.numCameras() == len(ids)
        for k, i in enumerate(ids):
            assert np.array([l3d.getSegment2D(k, n) for n in range(len(detected[i]))], np.float32).tobytes() == detected[i].tobytes()
        assert sorted(f[-4:] for f in os.listdir(tmp_path / "out")) == [".stl", ".txt"]
    finally:
        l3d.close()


# ---- agreement: geometry through the detector
AGREE = dict(width=320, height=200, f=250.0, k1=-0.25, k2=0.0, n_strokes=12, margin=14.0, seed=3)


def _strokes(p):
    """long strokes inside the image, `margin` px off its border, no two nearly on top of each other"""
    rng = np.random.default_rng(p["seed"])
    out = []
    while len(out) < p["n_strokes"]:
        a = rng.uniform([p["margin"], p["margin"]], [p["width"] - p["margin"], p["height"] - p["margin"]])
        b = rng.uniform([p["margin"], p["margin"]], [p["width"] - p["margin"], p["height"] - p["margin"]])
        if np.hypot(*(b - a)) < 90.0:
            continue
        mid = 0.5 * (a + b)
        if any(np.hypot(*(mid - 0.5 * (s[:2] + s[2:]))) < 14.0 for s in out):
            continue
        out.append(np.concatenate([a, b]))
    return np.array(out)


def _scene_at(X, Y, strokes):
    """the analytic scene at coordinates (X, Y) of the ideal image: the stroke profile of _draw"""
    val = np.full(X.shape, 210.0)
    for x1, y1, x2, y2 in strokes:
        d = np.array([x2 - x1, y2 - y1])
        L = np.hypot(*d)
        d /= L
        a = np.clip((X - x1) * d[0] + (Y - y1) * d[1], 0, L)
        dist = np.hypot(X - (x1 + a * d[0]), Y - (y1 + a * d[1]))
        val = np.minimum(val, 210.0 - 170.0 * np.clip(2.0 - dist, 0, 1))
    return np.rint(val).astype(np.uint8)


def _newton_inverse(u, v, fx, fy, cx, cy, k1, k2):
    xd, yd = (u - cx) / fx, (v - cy) / fy
    rd = np.hypot(xd, yd)
    r = rd.copy()
    for _ in range(60):
        r = r - (r * (1.0 + (k2 * r * r + k1) * r * r) - rd) / (1.0 + 3.0 * k1 * r * r + 5.0 * k2 * r ** 4)
    s = np.where(rd > 0, r / np.where(rd > 0, rd, 1.0), 1.0)
    return fx * (xd * s) + cx, fy * (yd * s) + cy


def test_undistorted_image_gives_the_ideal_image_s_segments(gpu_ctx):
    """An ideal image of long strokes, and the image a camera with barrel distortion takes of the same scene (the scene sampled at the
    Newton-inverted coordinates).  Detecting with the camera must give the ideal image's segments, to the reference detector's own
    repeatability (`floor`, tests/golden/detect_ref.npz); detecting without it must not -- the control that shows this test can fail."""
    p = AGREE
    floor = float(np.load(GOLDEN)["floor"])
    w, h = p["width"], p["height"]
    cam = (p["f"], p["f"], w / 2.0, h / 2.0, p["k1"], p["k2"])
    strokes = _strokes(p)
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    ideal = _scene_at(uu, vv, strokes)
    jj, ii = _newton_inverse(uu, vv, *cam)
    back = um.source_coordinates(w, h, *cam)              # the inverse is one: distort(inverse(u, v)) = (u, v) at the pixels it will be read at
    distorted = _scene_at(jj, ii, strokes)
    ju, iv = _newton_inverse(back[0], back[1], *cam)
    assert np.abs(ju - uu).max() < 1e-9 and np.abs(iv - vv).max() < 1e-9
    a = gpu_ctx.detect_segments(ideal, min_length=0.0, max_segments=1 << 20)
    b = gpu_ctx.detect_segments(distorted, min_length=0.0, max_segments=1 << 20, camera=cam)
    c = gpu_ctx.detect_segments(distorted, min_length=0.0, max_segments=1 << 20)
    with_cam = (dm.cover(a, b), dm.cover(b, a))
    without = (dm.cover(a, c), dm.cover(c, a))
    print("agreement scene %s: %d / %d / %d segments (ideal / with camera / without)" % (p, len(a), len(b), len(c)))
    print("cover with camera: ideal by undistorted %.4f, undistorted by ideal %.4f; without camera: %.4f, %.4f; floor %.4f" % (with_cam + without + (floor,)))
    assert len(a) >= p["n_strokes"]
    assert min(with_cam) >= floor, (with_cam, floor)
    assert max(without) < floor, (without, floor)
