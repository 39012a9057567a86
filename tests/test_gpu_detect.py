"""The device line segment detector (l3d_detect.hip) against the reference's own detector as committed data
(tests/golden/detect_ref.npz, made by tests/golden/make_golden_detect.py).

The bar is AGREEMENT, not identity (the reference's region growing is a sequential greedy loop): recall = cover(ref, ours) and
precision = cover(ours, ref) (tests/detect_metric.py), pooled over a set of images, must each reach `floor` -- the worst
single-image agreement of the reference with itself when only the noise of the image is redrawn.  Everything else -- determinism,
selection, argument errors, the wiring into addImage -- is exact."""
import os

import numpy as np
import pytest

import detect_metric as dm
from line3d_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _rgb(g):
    grey = g["img_noisy11"].astype(np.int16)
    return np.stack([np.clip(grey + g["rgb_d0"], 0, 255), grey, np.clip(grey + g["rgb_d2"], 0, 255)], axis=-1).astype(np.uint8)


def _report(name, pairs):
    rec = dm.pooled([(ref, ours) for ref, ours in pairs])
    pre = dm.pooled([(ours, ref) for ref, ours in pairs])
    for k, (ref, ours) in enumerate(pairs):
        print("%s[%d]: reference %d segments, detector %d, recall %.4f precision %.4f" % (name, k, len(ref), len(ours), dm.cover(ref, ours), dm.cover(ours, ref)))
    print("%s pooled: recall %.4f precision %.4f" % (name, rec, pre))
    return rec, pre


def test_noisy_set_agrees_with_the_reference(gpu_ctx, golden):
    floor = float(golden["floor"])
    pairs = []
    for i in range(int(golden["n_noisy"])):
        ours = gpu_ctx.detect_segments(golden["img_noisy%02d" % i], min_length=0.0, max_segments=1 << 20)
        ref = golden["ref_noisy%02d" % i]
        assert len(ref) == 0 or len(ours) > 0, "image %d: the reference finds %d segments, the detector none" % (i, len(ref))
        pairs.append((ref, ours))
    rec, pre = _report("noisy", pairs)
    print("floor %.4f" % floor)
    assert len(gpu_ctx.detect_segments(golden["img_flat"], min_length=0.0)) == 0 and len(golden["ref_flat"]) == 0
    assert rec >= floor and pre >= floor, (rec, pre, floor)


def test_special_images_agree_with_the_reference(gpu_ctx, golden):
    floor = float(golden["floor"])
    pairs = []
    for k in ("edge0", "edge90", "edge45", "edge7", "diag", "tiny"):
        ours = gpu_ctx.detect_segments(golden["img_" + k], min_length=0.0, max_segments=1 << 20)
        assert len(golden["ref_" + k]) == 0 or len(ours) > 0, k
        pairs.append((golden["ref_" + k], ours))
    rgb = _rgb(golden)
    pairs.append((golden["ref_rgb"], gpu_ctx.detect_segments(rgb, min_length=0.0, max_segments=1 << 20)))
    # rescaled: the detector works at 320x240, its coordinates come back in pixels of the 640x480 image
    up = float(dm.upscale_factor(640, 480, 320, 240))
    assert up == 2.0
    ours = gpu_ctx.detect_segments(rgb, new_size=(320, 240), min_length=0.0, max_segments=1 << 20)
    ref = golden["ref_rescaled"][:, :4] * up
    assert ours[:, [0, 2]].max() > 330 and ours[:, [1, 3]].max() > 250, "coordinates are not in original-image pixels"
    pairs.append((ref, ours))
    rec, pre = _report("special", pairs)
    assert rec >= floor and pre >= floor, (rec, pre, floor)


def test_deterministic_and_stride_independent(gpu_ctx, golden):
    img = golden["img_noisy10"]
    a = gpu_ctx.detect_segments(img)
    b = gpu_ctx.detect_segments(img)
    assert len(a) > 0 and a.tobytes() == b.tobytes()
    other = capi.Context(0)
    try:
        assert other.detect_segments(img).tobytes() == a.tobytes()
    finally:
        other.close()
    padded = np.full((img.shape[0], img.shape[1] + 37), 77, np.uint8)
    padded[:, :img.shape[1]] = img
    view = padded[:, :img.shape[1]]
    assert view.strides[0] == img.shape[1] + 37
    assert gpu_ctx.detect_segments(view).tobytes() == a.tobytes()
    rgb = _rgb(golden)
    pad3 = np.zeros((480, 700, 3), np.uint8)
    pad3[:, :640] = rgb
    assert gpu_ctx.detect_segments(pad3[:, :640]).tobytes() == gpu_ctx.detect_segments(rgb).tobytes()


def test_selection(gpu_ctx, golden):
    img = golden["img_noisy11"]
    full = gpu_ctx.detect_segments(img, min_length=0.0, max_segments=1 << 20)
    assert len(full) > 10
    dx, dy = full[:, 0] - full[:, 2], full[:, 1] - full[:, 3]
    length = np.sqrt(dx * dx + dy * dy)                 # float32, the selection's own formula
    assert length.dtype == np.float32 and np.all(np.diff(length) <= 0)
    assert gpu_ctx.detect_segments(img, min_length=0.0, max_segments=5).tobytes() == full[:5].tobytes()
    med = float(np.float32(np.median(length)))
    longer = gpu_ctx.detect_segments(img, min_length=med, max_segments=1 << 20)
    assert longer.tobytes() == full[length > np.float32(med)].tobytes() and 0 < len(longer) < len(full)
    assert len(gpu_ctx.detect_segments(img)) == int(np.sum(length > np.float32(0.005) * np.sqrt(np.float32(480 * 480 + 640 * 640))))


def test_argument_errors(gpu_ctx, golden):
    import ctypes as C
    lib = gpu_ctx.lib
    out, n = C.POINTER(C.c_float)(), C.c_int(0)

    def call(img, w, h, ch, stride):
        return lib.l3d_detect_segments(gpu_ctx.h, img.ctypes.data_as(C.c_void_p), C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), C.c_int(w), C.c_int(h),
                                       C.c_float(0.0), C.c_int(3000), C.byref(out), C.byref(n))
    INVALID = 1         # L3D_ERR_INVALID
    buf = np.zeros((64, 64 * 3), np.uint8)
    assert call(buf, 7, 7, 1, 7) == INVALID
    assert call(buf, 32, 32, 2, 64) == INVALID
    assert call(buf, 32, 32, 3, 95) == INVALID
    with pytest.raises(capi.L3DError):
        gpu_ctx.detect_segments(np.zeros((7, 7), np.uint8))
    a = gpu_ctx.detect_segments(golden["img_edge7"], min_length=0.0)
    assert len(a) >= 1                   # the context is usable afterwards


# ---- wiring: pixels -> addImage -> compute3Dmodel
def _draw(width, height, segs):
    """3-px dark strokes on a light ground, anti-aliased by the distance to the segment"""
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


def test_add_image_pixels_equals_detect_then_add_image(gpu_ctx, tmp_path):
    from line3d_amd.pipeline import Line3D
    from line3d_amd.synth import make_scene
    scene = make_scene(10, 40, 6, seed=11, noise_px=0.0, width=640, height=360, f=500.0, seg_len=(0.3, 0.8))
    images = {v["id"]: _draw(640, 360, v["segments"]) for v in scene.views}
    detected = {i: gpu_ctx.detect_segments(img) for i, img in images.items()}
    n_segs = {i: len(s) for i, s in detected.items()}
    assert min(n_segs.values()) > 0

    def run(add):
        l3d = Line3D(str(tmp_path), matchingNeighbors=6)
        try:
            l3d.keep_view_matches(True)
            for v in scene.views:
                assert add(l3d, v)
            assert l3d.numCameras() == len(scene.views)
            l3d.compute3Dmodel(False)
            return _model_bytes(l3d, scene, n_segs)
        finally:
            l3d.close()

    caches = lambda: sorted(f for f in os.listdir(tmp_path) if f.startswith("segments_"))
    ref, n_lines = run(lambda l, v: l.addImage_fixed_sim(v["id"], 640, 360, detected[v["id"]], v["K"], v["R"], v["t"], v["sims"]))
    print("wiring scene: %d views, %d..%d segments per view, %d 3-D lines" % (len(scene.views), min(n_segs.values()), max(n_segs.values()), n_lines))
    got, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False))
    assert got == ref
    assert caches() == []
    got, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=True))
    assert got == ref
    assert len(caches()) == len(scene.views)
    blank = {i: np.full_like(img, 128) for i, img in images.items()}         # the caches stand in for the pixels
    got, _ = run(lambda l, v: l.add_image_pixels_fixed_sim(v["id"], blank[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=True))
    assert got == ref
    # flag off: the stale caches go, and a flat image adds no view without being an error
    l3d = Line3D(str(tmp_path), matchingNeighbors=6)
    try:
        v = scene.views[0]
        assert l3d.add_image_pixels_fixed_sim(v["id"], blank[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False)
        assert l3d.numCameras() == 0
        assert len(caches()) == len(scene.views) - 1
    finally:
        l3d.close()
