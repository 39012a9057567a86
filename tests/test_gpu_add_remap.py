"""The add family with a remap (l3d_line3d_add_image_entry_remap, l3d_line3d_add_images_remap and their device forms; "A REMAP" in
include/line3d_amd.h) on the six-view wiring scene of tests/test_gpu_add_images.py (tests/golden/jpeg_ref.npz): host pixels, JPEG bytes and device
tensors, single and batched, all give the view that results from undistorting first and adding the result with the same mask -- size, K, segments
and cache file bytes; the cache file carries the OUTPUT size in its name.  Then the driver: sfm.reconstruct_from_images(alpha=) on the COLMAP
fixture adds every view with the planner's K and size."""
import ctypes as C
import os

import numpy as np
import pytest

from line3d_amd import capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_ref.npz")
SCENE = dict(noise_px=0.0, width=320, height=200, f=250.0, seg_len=(0.3, 0.8), seed=11)
OUT = (240, 150)
INVALID, UNSUPPORTED = 1, 5


def _lens(K):
    """a fisheye with the view's own camera as its source camera"""
    return capi.lens("fisheye", [-0.03, 0.01, -0.002, 0.0004], camera=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def _mask():
    """the caller's plane in the source grid: a timestamp in a corner and a band in the middle"""
    m = np.ones((SCENE["height"], SCENE["width"]), np.uint8)
    m[180:, :90] = 0
    m[95:103, 100:230] = 0
    return m


@pytest.fixture(scope="module")
def wiring(gpu_ctx):
    """the scene; per view the file, the pixels, the planned camera, and the image undistorted first with its validity plane"""
    from line3d_amd.synth import make_scene
    g = np.load(GOLDEN)
    scene = make_scene(6, 30, 6, **SCENE)
    files = {v["id"]: g["view%d/bytes" % k].tobytes() for k, v in enumerate(scene.views)}
    images = {i: gpu_ctx.decode_jpeg(d) for i, d in files.items()}
    plan, first = {}, {}
    for v in scene.views:
        K2, wh = capi.undistort_plan(_lens(v["K"]), (SCENE["width"], SCENE["height"]), 0.7, OUT)
        assert wh == OUT
        plan[v["id"]] = K2
        first[v["id"]] = gpu_ctx.undistort(images[v["id"]], K2, lens=_lens(v["K"]), out_size=OUT, mask=_mask(), return_mask=True)
        assert 0.05 < (first[v["id"]][1] == 0).mean() < 0.6
    return scene, files, images, plan, first


def _run(directory, entries, batched, expect=None, prepare=True):
    """-> ({view id: segment bytes}, {cache file name: bytes}, message).  The view's size shows in the cache file's name (which carries the size the
    detector worked at); the library has no getter for a view's K, which is compared through the entries instead (test_driver_plans_every_camera)"""
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
                args = (e.pop("imageID"), e.pop("data") if "data" in e else e.pop("img"), e.pop("K"), e.pop("R"), e.pop("t"), e.pop("viewSimilarity"))
                (l3d.add_image_jpeg_fixed_sim if isinstance(args[1], bytes) else l3d.add_image_pixels_fixed_sim)(*args, **e)
                status.append(l3d.last_rc)
        message = l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        assert status == (expect or [0] * len(entries)), message
        if prepare:
            l3d.prepare()           # writes the caches of the new views
        views = {}
        for e, st in zip(entries, status):
            if st == 0:
                out, n = [], 0
                while True:
                    o = (C.c_float * 4)()
                    if l3d.lib.l3d_line3d_get_segment2D(l3d.h, C.c_uint(e["imageID"]), C.c_uint(n), o) != 0:
                        break
                    out.append(list(o))
                    n += 1
                views[e["imageID"]] = np.array(out, np.float32).tobytes()
        caches = {}
        for f in sorted(os.listdir(directory)):
            if f.startswith("segments_"):
                with open(os.path.join(directory, f), "rb") as fh:
                    caches[f] = fh.read()
        return views, caches, message
    finally:
        l3d.close()


def _entries(scene, kind, files, images, plan, remap=True):
    out = []
    for v in scene.views:
        e = dict(imageID=v["id"], K=plan[v["id"]], R=v["R"], t=v["t"], viewSimilarity=v["sims"])
        if kind == "jpeg":
            e["data"] = files[v["id"]]
        elif kind == "device":
            import torch
            e["img"] = torch.from_numpy(images[v["id"]].copy()).cuda()
        else:
            e["img"] = images[v["id"]]
        if remap:
            e.update(lens=_lens(v["K"]), out_size=OUT, mask=_mask())
        out.append(e)
    return out


@pytest.fixture(scope="module")
def reference(wiring, tmp_path_factory):
    """computed once: the views of the images undistorted first, added with the validity plane that came with them as the mask"""
    scene, files, images, plan, first = wiring
    entries = [dict(imageID=v["id"], K=plan[v["id"]], R=v["R"], t=v["t"], viewSimilarity=v["sims"], img=first[v["id"]][0], mask=first[v["id"]][1]) for v in scene.views]
    ref = _run(tmp_path_factory.mktemp("first"), entries, False)
    unmasked = _run(tmp_path_factory.mktemp("unmasked"), [{k: v for k, v in e.items() if k != "mask"} for e in entries], False)
    assert len(ref[0]) == 6 and len(ref[1]) == 6 and min(len(b) for b in ref[0].values()) > 0
    assert ref[0] != unmasked[0]                                    # the plane matters on this scene
    assert all("_%dx%d_" % OUT in name for name in ref[1])          # the cache file carries the output size in its name
    return ref


@pytest.mark.parametrize("batched", [False, True], ids=["single", "add_images"])
@pytest.mark.parametrize("kind", ["pixels", "jpeg", "device"])
def test_remap_views(wiring, reference, tmp_path, kind, batched):
    scene, files, images, plan, _ = wiring
    got = _run(tmp_path / "remap", _entries(scene, kind, files, images, plan), batched)
    assert got[0] == reference[0]                                   # the segments (in pixels of the output)
    assert got[1] == reference[1]                                   # the cache files: names (the output size) and bytes
    # a second run loads the caches: the image is not needed, and the views are the same
    again = _run(tmp_path / "remap", _entries(scene, kind, files, images, plan), batched)
    assert again[0] == reference[0] and again[1] == reference[1]


def test_max_img_width_acts_on_the_output_size(wiring, tmp_path):
    """240 x 150 with maxImgWidth = 120: the detector works at 120 x 75, which names the cache files"""
    from line3d_amd.pipeline import Line3D
    scene, files, images, plan, _ = wiring
    l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
    try:
        assert l3d.add_images(_entries(scene, "pixels", files, images, plan), maxImgWidth=120) == [0] * 6
        l3d.prepare()
        names = sorted(f for f in os.listdir(tmp_path) if f.startswith("segments_"))
        assert len(names) == 6 and all("_120x75_" in f for f in names), names
    finally:
        l3d.close()


def test_refusals_fail_alone(wiring, tmp_path):
    scene, files, images, plan, _ = wiring
    entries = _entries(scene, "pixels", files, images, plan)
    entries[1]["dist"] = (-0.2, 0.03)                               # dist beside a remap
    entries[2].pop("lens")                                          # an output size without a lens
    skew = np.array(entries[3]["K"]).copy()
    skew[0, 1] = 0.5
    entries[3]["K"] = skew                                          # a remap that resamples with a skewed K
    entries[4]["out_size"] = (7, 150)                               # an output below 8 x 8
    for batched in (False, True):
        _, _, message = _run(tmp_path / str(batched), entries, batched, expect=[0, INVALID, INVALID, UNSUPPORTED, INVALID, 0], prepare=False)
        if batched:             # (one line per failed entry; the single calls leave the last failure's words)
            assert "remap" in message and "skewed" in message and "8x8" in message


@pytest.mark.parametrize("kind", ["pixels", "jpeg", "device"])
def test_a_mask_of_another_extent_is_refused(gpu_ctx, wiring, tmp_path, kind):
    """the library reads width x height bytes of a mask: one whose extent is not the source's (a file's: its headers') fails alone, with the extents in
    the message, on every path -- the single add calls, add_images, and the detector's call for a file"""
    scene, files, images, plan, _ = wiring
    for k, wrong in enumerate((np.ones((199, 320), np.uint8), np.ones((200, 319), np.uint8), np.ones((150, 240), np.uint8))):
        entries = _entries(scene, kind, files, images, plan)
        entries[1]["mask"] = wrong
        entries[3].pop("lens")
        entries[3].pop("out_size")
        entries[3]["mask"] = wrong                                      # a mask alone, nothing resampled
        for batched in (False, True):
            _, _, message = _run(tmp_path / ("%d%s" % (k, batched)), entries, batched, expect=[0, INVALID, 0, INVALID, 0, 0], prepare=False)
            assert "the mask is %d x %d, the source image 320 x 200" % wrong.shape[::-1] in message
    with pytest.raises(capi.L3DError) as e:
        gpu_ctx.detect_segments_jpeg(files[scene.views[0]["id"]], mask=np.ones((199, 320), np.uint8))
    assert e.value.code == INVALID and "the mask is 320 x 199" in str(e.value)


def test_driver_plans_every_camera(gpu_ctx, tmp_path, monkeypatch):
    """sfm.reconstruct_from_images(alpha=0.5) over the nine cameras with a lens of the COLMAP fixture, with images of the test's own: every view is
    added with the planner's K and size (the entries the driver hands to add_images, and the views' cache files); without alpha and out_size the
    driver hands over what it did before.  (The reconstruction itself is not this test's: compute3Dmodel is stood in for by prepare.)"""
    import importlib.util
    import shutil
    from line3d_amd import sfm
    from line3d_amd.pipeline import Line3D
    spec = importlib.util.spec_from_file_location("make_golden_colmap", os.path.join(HERE, "golden", "make_golden_colmap.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    model = tmp_path / "model"
    os.makedirs(model)
    shutil.copy(os.path.join(HERE, "golden", "colmap_small", "txt", "cameras.txt"), model)
    with open(model / "images.txt", "w") as f:                          # an image file that names each camera once
        for k, cam in enumerate(gen.CAMERAS):
            f.write("%d 1 0 0 0 0 0 %g %d im%d.jpg\n\n" % (k + 1, 0.1 * k, cam[0], k))
    read = sfm.read_colmap(str(model))
    cams = [dict(c, worldpoints=np.arange(10, dtype=np.uint32)) for c in read.cameras if c.get("lens") is not None]
    assert len(cams) == 9
    scene = sfm.SfmScene(cams, 10)
    rng = np.random.default_rng(2)

    def load(i, name):
        w, h = cams[i]["size"]
        img = np.full((h, w), 90, np.uint8)
        for _ in range(12):                                             # bright rectangles: something to detect
            x, y = int(rng.integers(20, w - 130)), int(rng.integers(20, h - 100))
            img[y:y + int(rng.integers(30, 80)), x:x + int(rng.integers(40, 110))] = int(rng.integers(150, 255))
        return img
    seen = []
    add_images = Line3D.add_images

    def recording(self, entries, **kw):
        seen.extend(dict(e) for e in entries)
        return add_images(self, entries, **kw)
    monkeypatch.setattr(Line3D, "add_images", recording)
    monkeypatch.setattr(Line3D, "compute3Dmodel", lambda self, diffusion=False: self.prepare())
    for alpha, directory in ((0.5, tmp_path / "planned"), (None, tmp_path / "as_before")):
        os.makedirs(directory)
        del seen[:]
        l3d = sfm.reconstruct_from_images(scene, load, str(directory) + os.sep, neighbors=4, alpha=alpha, batch=4)
        try:
            assert l3d.numCameras() == 9 and len(seen) == 9
            names = sorted(f for f in os.listdir(directory) if f.startswith("segments_"))
            planned = 0
            for i, (cam, en) in enumerate(zip(cams, seen)):
                lens = cam["lens"]
                active = lens.model == capi.LENS_FISHEYE or any(abs(c) > 1e-12 for c in lens.k)
                if alpha is not None and active:
                    K2, wh = capi.undistort_plan(lens, cam["size"], alpha)
                    assert np.array_equal(np.asarray(en["K"]), K2) and tuple(en["out_size"]) == wh and en["lens"] is not None and "dist" not in en
                    planned += 1
                else:
                    wh = tuple(cam["size"])
                    assert np.array_equal(np.asarray(en["K"]), np.asarray(cam["K"])) and en.get("out_size") is None
                assert any(n.startswith("segments_%d_%dx%d_" % (i, wh[0], wh[1])) for n in names), (i, wh, names)
            assert planned == (7 if alpha is not None else 0)           # (PINHOLE and SIMPLE_PINHOLE have nothing to plan)
        finally:
            l3d.close()
