"""The add family with a lens (l3d_line3d_add_image_entry_lens, l3d_line3d_add_images_lens and their device forms) on the six-view wiring scene of
tests/test_gpu_add_images.py (tests/golden/jpeg_ref.npz): host pixels, JPEG bytes and device tensors, single and batched.  A BROWN(k1, k2) lens
without a camera of its own is the entry with dist = (k1, k2); a general lens is undistorting first and adding without one; an entry with both
fails alone."""
import ctypes as C
import os

import numpy as np
import pytest

from line3d_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ref.npz")
SCENE = dict(noise_px=0.0, width=320, height=200, f=250.0, seg_len=(0.3, 0.8), seed=11)
DIST = (-0.2, 0.03)
INVALID, UNSUPPORTED = 1, 5


def _general(K):
    """a fisheye taken with a longer focal length and another principal point than the view's K"""
    return capi.lens("fisheye", [-0.03, 0.01, -0.002, 0.0004], camera=(1.2 * K[0, 0], 1.2 * K[1, 1], K[0, 2] - 2.0, K[1, 2] + 1.5))


@pytest.fixture(scope="module")
def wiring(gpu_ctx):
    from line3d_amd.synth import make_scene
    g = np.load(GOLDEN)
    scene = make_scene(6, 30, 6, **SCENE)
    files = {v["id"]: g["view%d/bytes" % k].tobytes() for k, v in enumerate(scene.views)}
    images = {i: gpu_ctx.decode_jpeg(d) for i, d in files.items()}
    undist = {v["id"]: gpu_ctx.undistort(images[v["id"]], v["K"], lens=_general(v["K"])) for v in scene.views}
    assert all(not np.array_equal(undist[i], images[i]) for i in images)
    return scene, files, images, undist


def _source(kind, i, files, images):
    if kind == "jpeg":
        return "data", files[i]
    if kind == "device":
        import torch
        return "img", torch.from_numpy(images[i].copy()).cuda()
    return "img", images[i]


def _run(directory, scene, entries, batched, expect=None, prepare=True):
    """-> ({view id: segment bytes}, {cache file name: bytes}, statuses)"""
    from line3d_amd.pipeline import Line3D
    os.makedirs(directory, exist_ok=True)
    l3d = Line3D(str(directory) + os.sep, matchingNeighbors=6)
    try:
        if batched:
            status = l3d.add_images(entries, loadAndStoreSegments=True)
        else:
            status = []
            for e in entries:
                e = dict(e)
                links = dict(viewSimilarity=e.pop("viewSimilarity"))
                if "data" in e:
                    l3d.add_image_jpeg_fixed_sim(e["imageID"], e["data"], e["K"], e["R"], e["t"], links["viewSimilarity"], dist=e.get("dist"), lens=e.get("lens"))
                else:
                    l3d.add_image_pixels_fixed_sim(e["imageID"], e["img"], e["K"], e["R"], e["t"], links["viewSimilarity"], dist=e.get("dist"), lens=e.get("lens"))
                status.append(l3d.last_rc)
        assert status == (expect or [0] * len(entries)), l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        message = l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        if prepare:
            l3d.prepare()           # writes the caches of the new views
        segs = {}
        for e, st in zip(entries, status):
            if st == 0:
                out, n = [], 0
                while True:
                    o = (C.c_float * 4)()
                    if l3d.lib.l3d_line3d_get_segment2D(l3d.h, C.c_uint(e["imageID"]), C.c_uint(n), o) != 0:
                        break
                    out.append(list(o))
                    n += 1
                segs[e["imageID"]] = np.array(out, np.float32).tobytes()
        caches = {}
        for f in sorted(os.listdir(directory)):
            if f.startswith("segments_"):
                with open(os.path.join(directory, f), "rb") as fh:
                    caches[f] = fh.read()
        return segs, caches, message
    finally:
        l3d.close()


def _entries(scene, kind, files, images, **extra):
    out = []
    for v in scene.views:
        key, val = _source(kind, v["id"], files, images)
        e = dict(imageID=v["id"], K=v["K"], R=v["R"], t=v["t"], viewSimilarity=v["sims"])
        e[key] = val
        for name, fn in extra.items():
            e[name] = fn(v)
        out.append(e)
    return out


@pytest.fixture(scope="module")
def references(wiring, tmp_path_factory):
    """computed once: the views with dist = (k1, k2), and the views of the images undistorted with the general lens first"""
    scene, files, images, undist = wiring
    with_dist = _run(tmp_path_factory.mktemp("dist"), scene, _entries(scene, "pixels", files, images, dist=lambda v: DIST), False)
    undistorted_first = _run(tmp_path_factory.mktemp("first"), scene, _entries(scene, "pixels", files, undist), False)
    plain = _run(tmp_path_factory.mktemp("plain"), scene, _entries(scene, "pixels", files, images), False)
    for r in (with_dist, undistorted_first, plain):
        assert len(r[0]) == 6 and len(r[1]) == 6 and min(len(b) for b in r[0].values()) > 0
    assert with_dist[0] != plain[0] and undistorted_first[0] != plain[0] and with_dist[0] != undistorted_first[0]
    return with_dist, undistorted_first


@pytest.mark.parametrize("batched", [False, True], ids=["single", "add_images"])
@pytest.mark.parametrize("kind", ["pixels", "jpeg", "device"])
def test_lens_views(wiring, references, tmp_path, kind, batched):
    scene, files, images, _ = wiring
    with_dist, undistorted_first = references
    # BROWN(k1, k2) with a zero source camera: the view dist = (k1, k2) gives -- size (in the cache's name), segments, cache bytes
    got = _run(tmp_path / "brown", scene, _entries(scene, kind, files, images, lens=lambda v: capi.lens("brown", DIST)), batched)
    assert got[0] == with_dist[0] and got[1] == with_dist[1]
    # a general lens: undistorting first and adding without a lens
    got = _run(tmp_path / "general", scene, _entries(scene, kind, files, images, lens=lambda v: _general(v["K"])), batched)
    assert got[0] == undistorted_first[0] and got[1] == undistorted_first[1]


@pytest.mark.parametrize("batched", [False, True], ids=["single", "add_images"])
@pytest.mark.parametrize("kind", ["pixels", "jpeg", "device"])
def test_an_entry_with_dist_and_lens_fails_alone(wiring, references, tmp_path, kind, batched):
    scene, files, images, _ = wiring
    entries = _entries(scene, kind, files, images, lens=lambda v: capi.lens("brown", DIST))
    entries[2]["dist"] = DIST
    entries[4]["lens"] = capi.lens(7, [0.1])                 # and one with a lens the checks refuse
    skew = entries[5]["K"].copy()
    skew[0, 1] = 0.5
    entries[5]["K"] = skew                                    # and an active lens with a skewed K
    # (no prepare: the three views that were added name neighbours that were not)
    segs, _, message = _run(tmp_path, scene, entries, batched, expect=[0, 0, INVALID, 0, INVALID, UNSUPPORTED], prepare=False)
    assert len(segs) == 3
    assert all(segs[i] == references[0][0][i] for i in segs)
    if batched:
        assert "both dist" in message and "unknown model" in message and "skew" in message


def test_object_undistort_and_the_sfm_flow(gpu_ctx, wiring, tmp_path):
    from line3d_amd import sfm
    from line3d_amd.pipeline import Line3D
    scene, files, images, undist = wiring
    v = scene.views[0]
    K = np.ascontiguousarray(v["K"], np.float64)
    lens = _general(K)
    l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
    try:
        img = images[v["id"]]
        out = np.zeros_like(img)
        call = lambda Kc, le, dst: l3d.lib.l3d_line3d_undistort_image_lens(l3d.h, img.ctypes.data_as(C.c_void_p), C.c_int(320), C.c_int(200), C.c_int(img.shape[2] if img.ndim == 3 else 1),
                                                                           C.c_size_t(img.strides[0]), Kc.ctypes.data_as(C.c_void_p), C.byref(le), dst.ctypes.data_as(C.c_void_p),
                                                                           C.c_size_t(img.strides[0]))
        assert call(K, lens, out) == 0 and out.tobytes() == undist[v["id"]].tobytes()
        skew = K.copy()
        skew[0, 1] = 0.5
        assert call(skew, lens, out) == UNSUPPORTED and "skew" in l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        assert call(skew, capi.lens("brown", [0.0] * 8), out) == 0 and out.tobytes() == img.tobytes()      # a lens that passes through: no K rule
        assert call(K, capi.Lens(), out) == INVALID
    finally:
        l3d.close()
    # the drivers' flow over cameras that carry `lens` and `K`, as read_colmap gives them
    cams = [dict(name="img%d.jpg" % w["id"], focal=250.0, dist=np.zeros(2), cv_dist=None, R=w["R"], t=w["t"], worldpoints=np.arange(10, dtype=np.uint32),
                 lens=_general(w["K"]), K=w["K"], size=(320, 200)) for w in scene.views]
    s = sfm.SfmScene(cams, 10)
    ids = [w["id"] for w in scene.views]
    with pytest.raises(RuntimeError, match="reconstruct_from_images"):
        sfm.reconstruct(s, [np.zeros((1, 4), np.float32)] * 6, [(320, 200)] * 6)
    l3d = sfm.reconstruct_from_images(s, lambda i, name: files[ids[i]] if i % 2 else images[ids[i]], str(tmp_path) + os.sep, neighbors=4, load_and_store_segments=False)
    try:
        assert l3d.numCameras() == 6
        for k, i in enumerate(ids):
            want = gpu_ctx.detect_segments(undist[i])
            assert np.array([l3d.getSegment2D(k, n) for n in range(len(want))], np.float32).tobytes() == want.tobytes()
    finally:
        l3d.close()
