"""Baseline JPEG on the device (k_jpg_idct, k_jpg_assemble; host half l3d_jpeg.cpp) against Pillow's pixels (tests/golden/jpeg_ref.npz, libjpeg-turbo at
its defaults) AND against the contract as tests/jpeg_model.py states it: byte for byte, every case.  Then the wiring into the detector and into addImage
(exact: the JPEG entry points must give what the pixel entry points give on the decoded arrays), the cache rule, and the refusals.  No test here
imports Pillow."""
import os

import numpy as np
import pytest

import jpeg_model as jm
from line3d_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ref.npz")
# the wiring scene of the fixture (tests/golden/make_golden_jpeg.py draws view0..view5 from it): the four views the feature was specified with give
# no 3-D line (a line needs support from enough other cameras), which would leave the comparison of kept matches and lines empty; six views with six
# neighbours, the scene of tests/test_gpu_undistort.py, do
SCENE = dict(n_views=6, n_segments=30, n_neighbors=6, seed=11, noise_px=0.0, width=320, height=200, f=250.0, seg_len=(0.3, 0.8))
DIST = (-0.2, 0.03)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {str(n): (z[str(n) + "/bytes"].tobytes(), z[str(n) + "/pixels"]) for n in z["names"]}, {str(n): z[str(n) + "/bytes"].tobytes() for n in z["refusals"]}


@pytest.fixture(scope="module")
def model(golden):
    """the model's pixels per case, computed once"""
    return {n: jm.decode(d) for n, (d, _) in golden[0].items()}


def _check(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, "%s: %d samples differ, first at %s: device %s, expected %s" % (what, len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])


def test_decode_equals_pillow_and_model(gpu_ctx, golden, model):
    cases, _ = golden
    by_size = sorted(cases, key=lambda n: (-cases[n][1].size, n))
    # descending: each call follows one on an image at least as large, whose coefficients, planes and pixels must not show.  In front of the
    # largest: a larger image of noise through the detector's pixel buffer
    gpu_ctx.detect_segments(np.random.default_rng(1).integers(0, 256, size=(260, 400, 3), dtype=np.uint8))
    first = {}
    for n in by_size:
        got = gpu_ctx.decode_jpeg(cases[n][0])
        _check(got, cases[n][1], n + " against Pillow")
        _check(got, model[n], n + " against the model")
        first[n] = got
    # ascending, in a context of its own: every buffer grows again and again; and two contexts give the same bytes
    ctx = capi.Context(0)
    try:
        for n in reversed(by_size):
            got = ctx.decode_jpeg(cases[n][0])
            _check(got, cases[n][1], n + " (ascending) against Pillow")
            _check(got, model[n], n + " (ascending) against the model")
            assert got.tobytes() == first[n].tobytes()
    finally:
        ctx.close()


def test_detect_segments_jpeg_equals_decode_then_detect(gpu_ctx, golden):
    cases, _ = golden
    found = 0
    for n in ("view0", "view1", "view2", "view3", "37x29_grey", "264x24_444", "50x33_420"):
        data = cases[n][0]
        img = gpu_ctx.decode_jpeg(data)
        a, b = gpu_ctx.detect_segments_jpeg(data), gpu_ctx.detect_segments(img)
        assert a.tobytes() == b.tobytes(), n
        found += len(a)
        h, w = img.shape[:2]
        cam = (250.0, 250.0, w / 2.0, h / 2.0) + DIST
        a, b = gpu_ctx.detect_segments_jpeg(data, camera=cam), gpu_ctx.detect_segments(img, camera=cam)
        assert a.tobytes() == b.tobytes(), n
    assert found > 0
    data = cases["view0"][0]
    img = gpu_ctx.decode_jpeg(data)
    cam = (250.0, 250.0, 160.0, 100.0) + DIST
    a = gpu_ctx.detect_segments_jpeg(data, new_size=(240, 150), min_length=2.0, max_segments=50, camera=cam)
    b = gpu_ctx.detect_segments(img, new_size=(240, 150), min_length=2.0, max_segments=50, camera=cam)
    assert len(a) > 0 and a.tobytes() == b.tobytes()
    assert a.tobytes() != gpu_ctx.detect_segments_jpeg(data, new_size=(240, 150), min_length=2.0, max_segments=50).tobytes()      # (the camera matters)


def test_8x8_file_behaves_as_an_8x8_image(gpu_ctx, golden):
    cases, _ = golden
    data = cases["8x8_grey"][0]
    img = gpu_ctx.decode_jpeg(data)
    assert img.shape == (8, 8)
    assert gpu_ctx.detect_segments_jpeg(data).tobytes() == gpu_ctx.detect_segments(img).tobytes()
    for n in ("1x1_420", "7x23_422"):          # below 8x8: refused as the pixel call refuses it
        with pytest.raises(capi.L3DError) as e1:
            gpu_ctx.detect_segments_jpeg(cases[n][0])
        with pytest.raises(capi.L3DError) as e2:
            gpu_ctx.detect_segments(gpu_ctx.decode_jpeg(cases[n][0]))
        assert e1.value.code == e2.value.code == 1 and str(e1.value) == str(e2.value)


# ---- wiring into addImage
@pytest.fixture(scope="module")
def wiring(gpu_ctx, golden):
    from line3d_amd.synth import make_scene
    scene = make_scene(SCENE["n_views"], SCENE["n_segments"], SCENE["n_neighbors"], **{k: v for k, v in SCENE.items() if k not in ("n_views", "n_segments", "n_neighbors")})
    files = {v["id"]: golden[0]["view%d" % k][0] for k, v in enumerate(scene.views)}
    images = {i: gpu_ctx.decode_jpeg(d) for i, d in files.items()}
    for k, v in enumerate(scene.views):
        _check(images[v["id"]], golden[0]["view%d" % k][1], "view%d" % k)
    n_segs = {}
    for dist in (None, DIST):
        for v in scene.views:
            K = v["K"]
            cam = None if dist is None else (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) + dist
            n_segs[(v["id"], dist)] = len(gpu_ctx.detect_segments(images[v["id"]], camera=cam))
    assert min(n_segs.values()) > 0
    return scene, files, images, n_segs


def _lines_bytes(l3d):
    parts = []
    lines = l3d.getResult()
    for seg2, seg3 in lines:
        parts.append(np.array(sorted((int(c), int(s)) for c, s in seg2), np.int64).tobytes())
        parts.append(np.array([np.concatenate(p) for p in seg3], np.float64).tobytes())
    return b"".join(parts), len(lines)


def _run(scene, n_segs, dist, add, directory, **kw):
    """add every view, compute3Dmodel, then the bytes of the model.  An ordinary object: segments, kept matches and lines.  A node object
    (devices=...): segments and lines -- l3d_line3d_view_matches is refused on a node object (one kept list per rank), so its kept matches
    show only through the lines they lead to"""
    from line3d_amd.pipeline import Line3D
    from test_gpu_undistort import _model_bytes
    node = "devices" in kw
    l3d = Line3D(str(directory) + os.sep, matchingNeighbors=6, **kw)
    try:
        if not node:
            l3d.keep_view_matches(True)
        for v in scene.views:
            assert add(l3d, v), l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        assert l3d.numCameras() == len(scene.views)
        ns = {v["id"]: n_segs[(v["id"], dist)] for v in scene.views}
        l3d.compute3Dmodel(False)
        if node:
            segs = b"".join(np.array([l3d.getSegment2D(v["id"], s) for s in range(ns[v["id"]])], np.float32).tobytes() for v in scene.views)
            lines, n_lines = _lines_bytes(l3d)
            return segs, lines, n_lines
        return _model_bytes(l3d, scene, ns)          # (bytes, number of lines)
    finally:
        l3d.close()


def _caches(d):
    return sorted(f for f in os.listdir(d) if f.startswith("segments_"))


def test_add_image_jpeg_equals_add_image_pixels(gpu_ctx, wiring, tmp_path):
    scene, files, images, n_segs = wiring
    px = lambda dist: (lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False, dist=dist))
    jp = lambda dist, store=False: (lambda l, v: l.add_image_jpeg_fixed_sim(v["id"], files[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=store, dist=dist))
    ref = _run(scene, n_segs, None, px(None), tmp_path)
    print("wiring scene: %d views, %d bytes of segments, kept matches and lines, %d 3-D lines" % (len(scene.views), len(ref[0]), ref[1]))
    assert ref[1] > 0                                     # (lines, and with them kept matches: the comparison is not an empty one)
    assert _run(scene, n_segs, None, jp(None), tmp_path) == ref
    assert _run(scene, n_segs, None, jp((0.0, 0.0)), tmp_path) == ref
    ref_d = _run(scene, n_segs, DIST, px(DIST), tmp_path)
    assert ref_d != ref and ref_d[1] > 0
    assert _run(scene, n_segs, DIST, jp(DIST), tmp_path) == ref_d
    assert _caches(tmp_path) == []
    # loadAndStoreSegments twice: written once, then the cache serves
    assert _run(scene, n_segs, DIST, jp(DIST, True), tmp_path) == ref_d
    written = _caches(tmp_path)
    assert len(written) == len(scene.views)
    stamps = [os.stat(os.path.join(tmp_path, f)).st_mtime_ns for f in written]
    assert _run(scene, n_segs, DIST, jp(DIST, True), tmp_path) == ref_d
    assert _caches(tmp_path) == written and [os.stat(os.path.join(tmp_path, f)).st_mtime_ns for f in written] == stamps


def test_add_image_jpeg_on_a_node_object_and_with_worldpoints(gpu_ctx, wiring, tmp_path):
    from line3d_amd.pipeline import Line3D
    scene, files, images, n_segs = wiring
    expect = {None: b"".join(gpu_ctx.detect_segments(images[v["id"]]).tobytes() for v in scene.views),
              DIST: b"".join(gpu_ctx.detect_segments(images[v["id"]], camera=(v["K"][0, 0], v["K"][1, 1], v["K"][0, 2], v["K"][1, 2]) + DIST).tobytes() for v in scene.views)}
    for dist in (None, DIST):
        jp = lambda l, v: l.add_image_jpeg_fixed_sim(v["id"], files[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False, dist=dist)
        px = lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=False, dist=dist)
        node_jp = _run(scene, n_segs, dist, jp, tmp_path, devices=[0, 0])
        node_px = _run(scene, n_segs, dist, px, tmp_path, devices=[0, 0])
        print("node object, dist %s: %d bytes of segments, %d 3-D lines" % (dist, len(node_jp[0]), node_jp[2]))
        assert node_jp[2] > 0
        assert node_jp[0] == node_px[0] == expect[dist]           # segments
        assert node_jp[1] == node_px[1] and node_jp[2] == node_px[2]          # lines (the kept matches lead to them)
        # the node object's model is the ordinary object's: the same lines from the same file
        one = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6, device=0)
        try:
            for v in scene.views:
                assert jp(one, v)
            one.compute3Dmodel(False)
            assert _lines_bytes(one) == (node_jp[1], node_jp[2])
        finally:
            one.close()
    l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
    try:
        v = scene.views[0]
        assert l3d.add_image_jpeg(v["id"], files[v["id"]], v["K"], v["R"], v["t"], [1, 2, 3], loadAndStoreSegments=False)
        n = n_segs[(v["id"], None)]
        assert np.array([l3d.getSegment2D(v["id"], s) for s in range(n)], np.float32).tobytes() == gpu_ctx.detect_segments(images[v["id"]]).tobytes()
        _check(l3d.decode_jpeg(files[v["id"]]), images[v["id"]], "Line3D.decode_jpeg")
    finally:
        l3d.close()


def test_reconstruct_from_images_takes_jpeg_bytes(gpu_ctx, wiring, tmp_path):
    from line3d_amd import sfm
    scene, files, images, n_segs = wiring
    ids = [v["id"] for v in scene.views]
    cams = [dict(name="img%d.jpg" % v["id"], focal=250.0, dist=np.array([-DIST[0], 0.0]), cv_dist=np.array(DIST), R=v["R"], t=v["t"],
                 worldpoints=np.arange(10, dtype=np.uint32)) for v in scene.views]
    got = {}
    for kind, load in (("bytes", lambda i, name: files[ids[i]]), ("arrays", lambda i, name: images[ids[i]])):
        l3d = sfm.reconstruct_from_images(sfm.SfmScene(cams, 10), load, str(tmp_path) + os.sep, neighbors=6, load_and_store_segments=False)
        try:
            assert l3d.numCameras() == len(ids)
            got[kind] = b"".join(np.array([l3d.getSegment2D(k, s) for s in range(n_segs[(i, DIST)])], np.float32).tobytes() for k, i in enumerate(ids))
        finally:
            l3d.close()
    assert got["bytes"] == got["arrays"] and len(got["bytes"]) > 0


def test_a_wanted_cache_stands_in_for_the_entropy_data(gpu_ctx, wiring, tmp_path):
    from line3d_amd.pipeline import Line3D
    scene, files, images, n_segs = wiring
    hollow = {}
    for i, data in files.items():
        at = jm.parse(data)["scan_offset"]
        hollow[i] = data[:at] + bytes(len(data) - at)          # headers intact, the entropy-coded data (and EOI) zeroed
        assert capi.jpeg_info(hollow[i]) == (320, 200, 3)
    add = lambda src, store: (lambda l, v: l.add_image_jpeg_fixed_sim(v["id"], src[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=store))
    ref = _run(scene, n_segs, None, add(files, True), tmp_path)
    written = _caches(tmp_path)
    assert len(written) == len(scene.views)
    assert _run(scene, n_segs, None, add(hollow, True), tmp_path) == ref          # served by the caches: the files' data is never looked at
    assert _caches(tmp_path) == written
    l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
    try:
        v = scene.views[0]
        assert not add(hollow, False)(l3d, v)                                      # cache unwanted: the file has to be decoded, and cannot be
        assert l3d.last_rc == 1 and l3d.numCameras() == 0
        assert "jpeg" in l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        assert add(files, False)(l3d, v) and l3d.numCameras() == 1
    finally:
        l3d.close()


def test_refusals_leave_the_context_usable(gpu_ctx, golden, tmp_path):
    from line3d_amd.pipeline import Line3D
    cases, refusals = golden
    good, pixels = cases["17x9_420"]
    view = cases["view0"][0]
    bad = [(refusals["progressive"], 5, "progressive"), (refusals["cmyk"], 5, "components"), (view[:len(view) // 2], 1, "truncated"),
           (b"\x89PNG\r\n\x1a\n" + bytes(64), 1, "SOI")]
    K, R, t = np.array([[250.0, 0, 160], [0, 250.0, 100], [0, 0, 1]]), np.eye(3), np.zeros(3)
    l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
    try:
        for data, code, word in bad:
            headers_ok = word == "truncated"
            if not headers_ok:
                with pytest.raises(capi.L3DError) as e:
                    capi.jpeg_info(data)
                assert e.value.code == code and word in str(e.value)
            out = np.zeros((200, 320, 3), np.uint8)
            ptr, n = capi._bytes_arguments(data)
            assert gpu_ctx.lib.l3d_decode_jpeg(gpu_ctx.h, ptr, n, capi._p(out), capi.C.c_size_t(960)) == code
            assert word in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode()
            seg, cnt = capi.C.POINTER(capi.C.c_float)(), capi.C.c_int(0)
            assert gpu_ctx.lib.l3d_detect_segments_jpeg(gpu_ctx.h, ptr, n, capi.C.c_int(0), capi.C.c_int(0), capi.C.c_float(1.0), capi.C.c_int(10), None,
                                                        capi.C.byref(seg), capi.C.byref(cnt)) == code
            assert word in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode() and cnt.value == 0
            assert l3d.lib.l3d_line3d_decode_jpeg(l3d.h, ptr, n, capi._p(out), capi.C.c_size_t(960)) == code
            assert not l3d.add_image_jpeg(7, data, K, R, t, [1, 2, 3], loadAndStoreSegments=False) and l3d.last_rc == code
            assert word in l3d.lib.l3d_line3d_last_error(l3d.h).decode()
            assert not l3d.add_image_jpeg_fixed_sim(8, data, K, R, t, {1: 0.5}, loadAndStoreSegments=False, dist=DIST) and l3d.last_rc == code
            assert l3d.numCameras() == 0
            # ... and both go on: a good file afterwards is byte-exact
            _check(gpu_ctx.decode_jpeg(good), pixels, "after a refusal")
            _check(l3d.decode_jpeg(good), pixels, "after a refusal (Line3D)")
        assert l3d.add_image_jpeg(7, view, K, R, t, [1, 2, 3], loadAndStoreSegments=False) and l3d.numCameras() == 1
    finally:
        l3d.close()
