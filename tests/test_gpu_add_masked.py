"""The segment-taking adds behind a segment mask (l3d_line3d_add_image_masked, l3d_line3d_add_image_cached_masked) on a synthetic scene of 6 views x 60
segments, 640 x 480: the masked add followed by compute3Dmodel gives, bit for bit, the result of the plain add fed the segments that the model of
tests/segmask_model.py leaves -- from given segments, from segment caches written by the existing path (whose collinearities are not taken over),
and on a two-rank node object with virtual ranks on one device; an all-valid mask gives the result of the unmasked scene; a mask of the wrong extent
is refused and adds no view; a masked add that leaves nothing returns L3D_OK and adds no view."""
import hashlib
import os

import numpy as np
import pytest

import segmask_cases as sc
import segmask_model as sm
from helpers import assert_lines_equal

pytestmark = pytest.mark.gpu

N = 6
W, H = 640, 480
KW = dict(mode=sm.SPLIT, threshold=1, keep_permille=500, max_gap=1, min_length=6.0)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def scene():
    from line3d_amd.synth import make_scene
    return make_scene(6, 60, N, seed=19, width=W, height=H, f=500.0)


@pytest.fixture(scope="module")
def masks(scene):
    return {v["id"]: sc.blocks(W, H, 100 + v["id"], cell=48, p=0.72) for v in scene.views}


@pytest.fixture(scope="module")
def filtered(scene, masks):
    """what the model leaves of every view's segments"""
    out = {v["id"]: sm.filter_segments(v["segments"], masks[v["id"]], **KW)[0] for v in scene.views}
    total, before = sum(len(s) for s in out.values()), sum(len(v["segments"]) for v in scene.views)
    assert all(len(s) > 10 for s in out.values()) and total != before
    assert any(not np.array_equal(out[v["id"]], v["segments"][:len(out[v["id"]])]) for v in scene.views)
    return out


def _finish(l):
    l.compute3Dmodel(False)
    A, n_nodes = l.affinity()
    out = dict(lines=l.getResult(), A=_sha(A), n_A=len(A), n_nodes=n_nodes, kept=l.chain_summary()["n_kept"].copy(), cams=l.numCameras())
    l.close()
    return out


def _assert_same(got, ref):
    assert got["cams"] == ref["cams"]
    assert got["n_nodes"] == ref["n_nodes"] and got["n_A"] == ref["n_A"] and got["A"] == ref["A"], "the affinity list differs"
    assert np.array_equal(got["kept"], ref["kept"]), "the per-view kept counts differ"
    assert_lines_equal(got["lines"], ref["lines"], 0.0)


def _plain(scene, segments, **kw):
    from line3d_amd.pipeline import Line3D
    l = Line3D("", matchingNeighbors=N, **(kw or dict(device=0)))
    for v in scene.views:
        assert l.addImage_fixed_sim(v["id"], W, H, segments[v["id"]], v["K"], v["R"], v["t"], v["sims"])
    return _finish(l)


@pytest.fixture(scope="module")
def reference(scene, filtered):
    ref = _plain(scene, filtered)
    assert ref["cams"] == 6 and int(ref["kept"].sum()) > 0
    return ref


def _mask_of(masks, v):
    from line3d_amd import capi
    return capi.segment_mask(masks[v["id"]], **KW)


def test_masked_add_equals_plain_add_of_the_models_segments(scene, masks, reference):
    from line3d_amd.pipeline import Line3D
    l = Line3D("", matchingNeighbors=N, device=0)
    for v in scene.views:
        assert l.addImage_fixed_sim(v["id"], W, H, v["segments"], v["K"], v["R"], v["t"], v["sims"], segment_mask=_mask_of(masks, v))
    _assert_same(_finish(l), reference)


def test_cached_masked_add_equals_it_too(scene, masks, reference, tmp_path):
    """the caches come from the existing path: an object with a data directory, addImage_ex with loadAndStoreSegments, prepare() writes the files --
    segments and collinearities.  The masked form filters the segments and computes the collinearities anew; the files stay as they were"""
    from line3d_amd.io import read_segment_cache, segment_cache_filename
    from line3d_amd.pipeline import Line3D
    data = str(tmp_path) + os.sep
    w = Line3D(data, matchingNeighbors=N, device=0)
    for v in scene.views:
        assert w.addImage_ex(v["id"], W, H, v["segments"], v["K"], v["R"], v["t"], v["sims"], maxImgWidth=-1, loadAndStoreSegments=True, fixed_sim=True)
    w.compute3Dmodel(False)
    w.close()
    files = {v["id"]: data + segment_cache_filename(v["id"], W, H, True) for v in scene.views}
    before = {}
    for v in scene.views:
        with open(files[v["id"]], "rb") as f:
            before[v["id"]] = f.read()
        assert np.array_equal(read_segment_cache(files[v["id"]]).segments, v["segments"])
    l = Line3D("", matchingNeighbors=N, device=0)
    for v in scene.views:
        assert l.addImage_cached(v["id"], W, H, files[v["id"]], v["K"], v["R"], v["t"], v["sims"], segment_mask=_mask_of(masks, v))
    _assert_same(_finish(l), reference)
    for v in scene.views:
        with open(files[v["id"]], "rb") as f:
            assert f.read() == before[v["id"]], "a cache file was changed"
    assert sorted(os.listdir(data)) == sorted(os.path.basename(p) for p in files.values()), "a cache file was written"


def test_masked_add_on_a_two_rank_node_object(scene, masks, filtered, reference):
    """virtual ranks on one device: the filter runs once, on rank 0's device, every rank gets the result -- the node's own plain add of the model's
    segments and the single device's both agree"""
    from line3d_amd.pipeline import Line3D
    l = Line3D("", matchingNeighbors=N, devices=[0, 0])
    assert l.num_ranks() == 2
    for v in scene.views:
        assert l.addImage_fixed_sim(v["id"], W, H, v["segments"], v["K"], v["R"], v["t"], v["sims"], segment_mask=_mask_of(masks, v))
    got = _finish(l)
    _assert_same(got, _plain(scene, filtered, devices=[0, 0]))
    _assert_same(got, reference)


def test_all_valid_mask_gives_the_unmasked_scene(scene):
    from line3d_amd import capi
    from line3d_amd.pipeline import Line3D
    full = np.full((H, W), 255, np.uint8)
    for mode in ("drop", "clip", "split"):
        l = Line3D("", matchingNeighbors=N, device=0)
        for v in scene.views:
            assert l.addImage_fixed_sim(v["id"], W, H, v["segments"], v["K"], v["R"], v["t"], v["sims"],
                                        segment_mask=capi.segment_mask(full, mode=mode, keep_permille=1000, min_length=1.0))
        _assert_same(_finish(l), _plain(scene, {v["id"]: v["segments"] for v in scene.views}))


def test_sfm_reconstruct_with_masks_equals_it_with_the_models_segments():
    """sfm.reconstruct(masks=...): the callable is asked by image name, an image without a mask is added as before, and the result is that of the same
    flow fed the model-filtered segments; views carry world point ids here (Line3D::addImage)"""
    from line3d_amd import sfm
    from line3d_amd.synth import make_scene_scattered
    sc8 = make_scene_scattered(8, 70, seed=5, n_worldpoints=300, width=W, height=H, f=500.0)
    cams = [dict(name="img%02d.jpg" % v["id"], focal=500.0, dist=np.zeros(2), cv_dist=np.zeros(2), R=v["R"], t=v["t"], worldpoints=v["worldpoints"]) for v in sc8.views]
    scene = sfm.SfmScene(cams, 300)
    planes = {c["name"]: sc.blocks(W, H, 300 + i, cell=48, p=0.72) for i, c in enumerate(cams) if i != 2}          # (image 2 has no mask)
    asked = []

    def masks(name):
        asked.append(name)
        return planes.get(name)

    segs = [v["segments"] for v in sc8.views]
    sizes = [(W, H)] * len(cams)
    kw = dict(mask_mode="clip", mask_max_gap=1, mask_min_length=6.0)
    got = sfm.reconstruct(scene, segs, sizes, neighbors=N, masks=masks, **kw)
    assert asked == [c["name"] for c in cams]
    want_segs = [s if c["name"] not in planes else sm.filter_segments(s, planes[c["name"]], mode=sm.CLIP, max_gap=1, min_length=6.0)[0] for s, c in zip(segs, cams)]
    assert all(len(s) for s in want_segs) and sum(len(s) for s in want_segs) < sum(len(s) for s in segs)
    want = sfm.reconstruct(scene, want_segs, sizes, neighbors=N)
    assert got.numCameras() == want.numCameras() == len(cams)
    A, n_nodes = got.affinity()
    B, m_nodes = want.affinity()
    assert n_nodes == m_nodes and _sha(A) == _sha(B)
    assert_lines_equal(got.getResult(), want.getResult(), 0.0)
    got.close()
    want.close()


def test_wrong_extent_is_refused_and_an_empty_result_adds_no_view(scene, masks):
    from line3d_amd import capi
    from line3d_amd.pipeline import Line3D
    l = Line3D("", matchingNeighbors=N, device=0)
    v = scene.views[0]
    for shape in ((H, W - 1), (H + 1, W), (W, H)):
        assert not l.addImage_fixed_sim(v["id"], W, H, v["segments"], v["K"], v["R"], v["t"], v["sims"], segment_mask=capi.segment_mask(np.full(shape, 255, np.uint8)))
        assert l.last_rc == 1 and "the view %d x %d" % (W, H) in l.lib.l3d_line3d_last_error(l.h).decode()
        assert l.numCameras() == 0
    # nothing left after the filter: L3D_OK and no view, as when the detector finds nothing -- and the id stays free
    assert l.addImage_fixed_sim(v["id"], W, H, v["segments"], v["K"], v["R"], v["t"], v["sims"], segment_mask=capi.segment_mask(np.zeros((H, W), np.uint8), mode="split"))
    assert l.last_rc == 0 and l.numCameras() == 0
    assert l.addImage_fixed_sim(v["id"], W, H, v["segments"], v["K"], v["R"], v["t"], v["sims"], segment_mask=capi.segment_mask(masks[v["id"]], **KW))
    assert l.numCameras() == 1
    # a lens puts the mask in another grid: its extent is then its own
    lens = capi.lens("brown", [-0.1, 0.02], camera=(700.0, 700.0, 480.0, 320.0))
    v1 = scene.views[1]
    m = capi.segment_mask(np.full((640, 960), 255, np.uint8), lens=lens, camera=(v1["K"][0, 0], v1["K"][1, 1], v1["K"][0, 2], v1["K"][1, 2]), mode="clip")
    assert l.addImage_fixed_sim(v1["id"], W, H, v1["segments"], v1["K"], v1["R"], v1["t"], v1["sims"], segment_mask=m)
    assert l.numCameras() == 2
    l.close()
