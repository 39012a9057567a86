"""Line3D.add_images (l3d_line3d_add_images) against the single calls it stands for, on the six-view, six-neighbour wiring scene of the JPEG tests
(tests/golden/jpeg_ref.npz: view0..view5): segments, kept matches and 3-D lines are the single calls', byte for byte; the cache rules, a failing entry,
a duplicate id, a node object and the drivers' flow."""
import os

import numpy as np
import pytest

from line3d_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ref.npz")
SCENE = dict(n_views=6, n_segments=30, n_neighbors=6, seed=11, noise_px=0.0, width=320, height=200, f=250.0, seg_len=(0.3, 0.8))
DIST = (-0.2, 0.03)
DISTORTED_VIEW = 2              # position in the scene of the one entry that comes with distortion coefficients
WORLDPOINTS = list(range(10))


@pytest.fixture(scope="module")
def wiring(gpu_ctx):
    from line3d_amd.synth import make_scene
    g = np.load(GOLDEN)
    scene = make_scene(SCENE["n_views"], SCENE["n_segments"], SCENE["n_neighbors"], **{k: v for k, v in SCENE.items() if k not in ("n_views", "n_segments", "n_neighbors")})
    files = {v["id"]: g["view%d/bytes" % k].tobytes() for k, v in enumerate(scene.views)}
    images = {i: gpu_ctx.decode_jpeg(d) for i, d in files.items()}
    n_segs = {}
    for k, v in enumerate(scene.views):
        K = v["K"]
        cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) + DIST if k == DISTORTED_VIEW else None
        n_segs[v["id"]] = len(gpu_ctx.detect_segments(images[v["id"]], camera=cam))
    assert min(n_segs.values()) > 0
    return scene, files, images, n_segs, g["progressive/bytes"].tobytes()


def _entry(k, v, files, images, links):
    """pixels for the even positions, the file for the odd ones; one entry with distortion"""
    e = dict(imageID=v["id"], K=v["K"], R=v["R"], t=v["t"])
    e["img" if k % 2 == 0 else "data"] = images[v["id"]] if k % 2 == 0 else files[v["id"]]
    e["viewSimilarity" if links == "sims" else "worldpointIDs"] = v["sims"] if links == "sims" else WORLDPOINTS
    if k == DISTORTED_VIEW:
        e["dist"] = DIST
    return e


def _single(l3d, e, store):
    """the single call an entry stands for"""
    dist = e.get("dist")
    if "img" in e:
        if "viewSimilarity" in e:
            return l3d.add_image_pixels_fixed_sim(e["imageID"], e["img"], e["K"], e["R"], e["t"], e["viewSimilarity"], loadAndStoreSegments=store, dist=dist)
        return l3d.add_image_pixels(e["imageID"], e["img"], e["K"], e["R"], e["t"], e["worldpointIDs"], loadAndStoreSegments=store, dist=dist)
    if "viewSimilarity" in e:
        return l3d.add_image_jpeg_fixed_sim(e["imageID"], e["data"], e["K"], e["R"], e["t"], e["viewSimilarity"], loadAndStoreSegments=store, dist=dist)
    return l3d.add_image_jpeg(e["imageID"], e["data"], e["K"], e["R"], e["t"], e["worldpointIDs"], loadAndStoreSegments=store, dist=dist)


def _lines_bytes(l3d):
    parts = []
    lines = l3d.getResult()
    for seg2, seg3 in lines:
        parts.append(np.array(sorted((int(c), int(s)) for c, s in seg2), np.int64).tobytes())
        parts.append(np.array([np.concatenate(p) for p in seg3], np.float64).tobytes())
    return b"".join(parts), len(lines)


def _segments_bytes(l3d, scene, n_segs):
    return b"".join(np.array([l3d.getSegment2D(v["id"], s) for s in range(n_segs[v["id"]])], np.float32).tobytes() for v in scene.views)


def _run(wiring, directory, links, batched, store=False, count=None, **kw):
    """-> (segments, kept matches, lines, number of lines); count: a dict that receives the k_det_region launches of the adding"""
    from line3d_amd.pipeline import Line3D
    scene, files, images, n_segs, _ = wiring
    node = "devices" in kw
    entries = [_entry(k, v, files, images, links) for k, v in enumerate(scene.views)]
    l3d = Line3D(str(directory) + os.sep, matchingNeighbors=6, **kw)
    try:
        if not node:
            l3d.keep_view_matches(True)
        ctx = l3d.context() if count is not None else None
        if ctx:
            ctx.profile_enable(True)
            ctx.profile_reset()
        if batched:
            assert l3d.add_images(entries, loadAndStoreSegments=store) == [0] * len(entries), l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        else:
            for e in entries:
                assert _single(l3d, e, store), l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        if ctx:
            count["k_det_region"] = ctx.profile_get("k_det_region")[0]
            ctx.profile_enable(False)
        assert l3d.numCameras() == len(entries)
        l3d.compute3Dmodel(False)
        matches = b"" if node else b"".join(l3d.view_matches(v["id"])[0].tobytes() for v in scene.views)
        return (_segments_bytes(l3d, scene, n_segs), matches) + _lines_bytes(l3d)
    finally:
        l3d.close()


def _caches(d):
    return sorted(f for f in os.listdir(d) if f.startswith("segments_"))


@pytest.mark.parametrize("links", ["sims", "worldpoints"])
def test_add_images_equals_the_single_calls(gpu_ctx, wiring, tmp_path, links):
    ref = _run(wiring, tmp_path, links, batched=False)
    got = _run(wiring, tmp_path, links, batched=True)
    print("%s: %d bytes of segments, %d of kept matches, %d 3-D lines" % (links, len(ref[0]), len(ref[1]), ref[3]))
    assert len(ref[0]) > 0 and len(ref[1]) > 0 and ref[3] > 0
    assert got[0] == ref[0], "segments"
    assert got[1] == ref[1], "kept matches"
    assert got[2:] == ref[2:], "lines"
    assert _caches(tmp_path) == []


def test_add_images_through_the_cache(gpu_ctx, wiring, tmp_path):
    scene = wiring[0]
    ref = _run(wiring, tmp_path, "sims", batched=False)
    count = {}
    assert _run(wiring, tmp_path, "sims", batched=True, store=True, count=count) == ref
    assert count["k_det_region"] == 3                      # six images of one size: one chunk, three rounds
    written = _caches(tmp_path)
    assert len(written) == len(scene.views)
    stamps = [os.stat(os.path.join(tmp_path, f)).st_mtime_ns for f in written]
    assert _run(wiring, tmp_path, "sims", batched=True, store=True, count=count) == ref
    assert count["k_det_region"] == 0                      # every view from its cache: nothing decoded, nothing detected
    assert _caches(tmp_path) == written and [os.stat(os.path.join(tmp_path, f)).st_mtime_ns for f in written] == stamps
    assert _run(wiring, tmp_path, "sims", batched=True, store=False, count=count) == ref
    assert count["k_det_region"] == 3 and _caches(tmp_path) == []


def test_a_failing_entry_fails_alone(gpu_ctx, wiring, tmp_path):
    from line3d_amd.pipeline import Line3D
    scene, files, images, n_segs, progressive = wiring
    entries = [_entry(k, v, files, images, "sims") for k, v in enumerate(scene.views)]
    bad = dict(entries[3])
    bad["data"] = progressive
    l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
    try:
        assert l3d.add_images(entries[:3] + [bad] + entries[4:], loadAndStoreSegments=False) == [0, 0, 0, 5, 0, 0]
        message = l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        assert message.startswith("image %d: jpeg" % bad["imageID"]) and "progressive" in message and "\n" not in message
        assert l3d.numCameras() == 5
        for k, v in enumerate(scene.views):
            if k != 3:
                n = n_segs[v["id"]]
                cam = (v["K"][0, 0], v["K"][1, 1], v["K"][0, 2], v["K"][1, 2]) + DIST if k == DISTORTED_VIEW else None
                assert np.array([l3d.getSegment2D(v["id"], s) for s in range(n)], np.float32).tobytes() == gpu_ctx.detect_segments(images[v["id"]], camera=cam).tobytes()
        # the entry's single call says the same
        assert not _single(l3d, bad, False) and l3d.last_rc == 5
        assert ("image %d: " % bad["imageID"]) + l3d.lib.l3d_line3d_last_error(l3d.h).decode() == message
        # a second view of an id, in one call and across calls; a truncated file; a flat image is no error and no view
        cut = dict(entries[3], data=files[scene.views[3]["id"]][:3000])
        flat = dict(entries[3], imageID=77)
        del flat["data"]
        flat["img"] = np.full((200, 320), 128, np.uint8)
        again = dict(entries[3])
        assert l3d.add_images([entries[0], cut, flat, entries[3], again], loadAndStoreSegments=False) == [1, 1, 0, 0, 1]
        lines = l3d.lib.l3d_line3d_last_error(l3d.h).decode().split("\n")
        assert len(lines) == 3 and "imageID already in use!" in lines[0] and "jpeg" in lines[1] and "imageID already in use!" in lines[2]
        assert l3d.numCameras() == 6
    finally:
        l3d.close()


def test_add_images_on_a_node_object(gpu_ctx, wiring, tmp_path):
    one = _run(wiring, tmp_path, "sims", batched=True)
    node = _run(wiring, tmp_path, "sims", batched=True, devices=[0, 0])
    assert node[3] > 0 and node[0] == one[0] and node[2:] == one[2:]


def test_reconstruct_from_images_gives_the_lines_of_the_single_calls(gpu_ctx, wiring, tmp_path):
    from line3d_amd import sfm
    from line3d_amd.pipeline import Line3D
    scene, files, images, n_segs, _ = wiring
    ids = [v["id"] for v in scene.views]
    cams = [dict(name="img%d.jpg" % v["id"], focal=250.0, dist=np.array([-DIST[0], 0.0]), cv_dist=np.array(DIST), R=v["R"], t=v["t"],
                 worldpoints=np.arange(10, dtype=np.uint32)) for v in scene.views]
    load = lambda i, name: files[ids[i]] if i % 2 else images[ids[i]]
    before = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)         # what the per-image loop did
    try:
        for i, cam in enumerate(cams):
            K = sfm.intrinsics(cam["focal"], 320, 200)
            add = before.add_image_jpeg if i % 2 else before.add_image_pixels
            assert add(i, load(i, None), K, cam["R"], cam["t"], cam["worldpoints"], loadAndStoreSegments=False, dist=cam["cv_dist"])
        before.compute3Dmodel(False)
        n = {i: len(gpu_ctx.detect_segments(images[ids[i]], camera=(250.0, 250.0, K[0, 2], K[1, 2]) + DIST)) for i in range(len(ids))}
        ref = (b"".join(np.array([before.getSegment2D(i, s) for s in range(n[i])], np.float32).tobytes() for i in range(len(ids))),) + _lines_bytes(before)
    finally:
        before.close()
    assert ref[2] > 0
    for batch in (16, 4):
        l3d = sfm.reconstruct_from_images(sfm.SfmScene(cams, 10), load, str(tmp_path) + os.sep, neighbors=6, load_and_store_segments=False, batch=batch)
        try:
            assert l3d.numCameras() == len(ids)
            got = (b"".join(np.array([l3d.getSegment2D(i, s) for s in range(n[i])], np.float32).tobytes() for i in range(len(ids))),) + _lines_bytes(l3d)
        finally:
            l3d.close()
        assert got == ref, batch
