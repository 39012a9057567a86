"""The result over the views ("PROJECTION AND OVERLAYS", 3 in include/line3d_amd.h) on the smoke scene make_scene(8, 120, 6, seed=3): project_result for
ALL and for OBSERVED equals the model of tests/project_model.py fed with getResult and the views' cameras as they were added, OBSERVED being the subset
of ALL whose lines have a member in the view; overlay on a grey 1920 x 1080 x 3 image, host and device, equals tests/draw_model.py applied layer by
layer and changes pixels; a node object of two ranks on one device gives the same bytes; a call before compute3Dmodel is refused."""
import numpy as np
import pytest

import draw_model as dm
import project_model as pm

pytestmark = pytest.mark.gpu

N = 6
VIEWS = (0, 5)              # indices of the views whose overlays are compared (each costs the model about a second)


@pytest.fixture(scope="module")
def scene():
    from line3d_amd.synth import make_scene
    return make_scene(8, 120, N, seed=3)


def _computed(scene, **kw):
    from line3d_amd.pipeline import Line3D, load_scene
    l = Line3D("", matchingNeighbors=N, **kw)
    load_scene(l, scene)
    l.compute3Dmodel(False)
    return l


@pytest.fixture(scope="module")
def done(scene):
    """the computed object, its result, the result's 3-D segments as one array and the line of each"""
    l = _computed(scene, device=0)
    res = l.getResult()
    seg3d = np.array([np.concatenate(s) for _, segs in res for s in segs], np.float64).reshape(-1, 6)
    line_of = np.array([li for li, (_, segs) in enumerate(res) for _ in segs], np.int32)
    yield l, res, seg3d, line_of
    l.close()


def _cams(scene):
    return [(v["K"], v["R"], v["t"], v["width"], v["height"]) for v in scene.views]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_scene_gives_lines(done):
    l, res, seg3d, line_of = done
    print("%d lines, %d 3-D segments" % (len(res), len(seg3d)))
    assert len(res) > 0 and len(seg3d) >= len(res)


def test_project_result_equals_the_model(scene, done):
    l, res, seg3d, line_of = done
    ids = [v["id"] for v in scene.views]
    want = pm.project(seg3d, _cams(scene), 1e-6, 0.0)
    got = l.project_result(ids, select="all")
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[2]) and np.array_equal(got[4], want[3])
    assert np.array_equal(got[2], line_of[got[1]])
    assert len(got[1]) > 0
    # the caller's cameras, without view ids: the same numbers
    again = l.project_result(None, cameras=_cams(scene), select="all")
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    # OBSERVED: the subset of ALL whose lines have a member in the view, in the same order
    obs = l.project_result(ids, select="observed")
    total = 0
    for c, vid in enumerate(ids):
        seen = np.array([any(cam == vid for cam, _ in seg2) for seg2, _ in res])
        a0, a1 = got[4][c], got[4][c + 1]
        keep = seen[got[2][a0:a1]]
        o0, o1 = obs[4][c], obs[4][c + 1]
        assert o1 - o0 == int(keep.sum())
        assert np.array_equal(_bits(obs[0][o0:o1]), _bits(got[0][a0:a1][keep])) and np.array_equal(obs[1][o0:o1], got[1][a0:a1][keep])
        assert np.array_equal(obs[2][o0:o1], got[2][a0:a1][keep]) and np.array_equal(obs[3][o0:o1], got[3][a0:a1][keep])
        total += int(keep.sum())
    assert 0 < total == len(obs[1]) < len(got[1])


def _model_overlay(scene, done, k, grey):
    """draw_model layer by layer: the view's member segments in line order (width 1), then the projected result of the observed lines (near 1e-6,
    margin 34, width 2), both coloured palette[line % 12]"""
    from line3d_amd import capi
    l, res, seg3d, line_of = done
    v = scene.views[k]
    pal = capi.default_palette()
    members = [(v["segments"][seg], li) for li, (seg2, _) in enumerate(res) for cam, seg in seg2 if cam == v["id"]]
    img = dm.draw(grey, np.array([m[0] for m in members], np.float32).reshape(-1, 4), pal, np.array([m[1] % 12 for m in members], np.int32), 1.0, 255)
    seen = np.array([any(cam == v["id"] for cam, _ in seg2) for seg2, _ in res])
    sel = np.flatnonzero(seen[line_of])
    segs, src, _, _ = pm.project(seg3d[sel], [_cams(scene)[k]], 1e-6, 34.0)
    return dm.draw(img, segs, pal, (line_of[sel[src]] % 12).astype(np.int32), 2.0, 255), len(members), len(segs)


@pytest.fixture(scope="module")
def overlays(scene, done):
    grey = np.full((1080, 1920, 3), 128, np.uint8)
    return grey, {k: _model_overlay(scene, done, k, grey) for k in VIEWS}


@pytest.mark.parametrize("k", VIEWS)
def test_overlay_host_and_device_equal_the_model(scene, done, overlays, k):
    import torch
    l = done[0]
    grey, want = overlays
    model, n_members, n_model = want[k]
    assert n_members > 0 and n_model > 0
    vid = scene.views[k]["id"]
    got = l.overlay(vid, grey)
    assert np.array_equal(got, model)
    assert (got != grey).any(), "the overlay changed no pixel"
    t = torch.from_numpy(grey).to("cuda:0")
    assert l.overlay(vid, t) is t
    assert np.array_equal(t.cpu().numpy(), model)
    # one layer alone, fixed colours: not the same picture
    only = l.overlay(vid, grey, layers=("model",), by_line=False, color_model=(255, 0, 0, 255), select="all")
    assert (only != grey).any() and not np.array_equal(only, got)


def test_a_node_object_gives_the_same_bytes(scene, done, overlays):
    l = done[0]
    grey, want = overlays
    ids = [v["id"] for v in scene.views]
    node = _computed(scene, devices=[0, 0])
    try:
        assert node.num_ranks() == 2
        a, b = l.project_result(ids, select="observed"), node.project_result(ids, select="observed")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        k = VIEWS[0]
        assert np.array_equal(node.overlay(scene.views[k]["id"], grey), want[k][0])
    finally:
        node.close()


def test_refusals(scene, done):
    from line3d_amd import capi
    from line3d_amd.pipeline import Line3D, load_scene
    l = done[0]
    grey = np.full((1080, 1920, 3), 128, np.uint8)
    with pytest.raises(capi.L3DError, match="error 1.*unknown view"):
        l.overlay(12345, grey)
    with pytest.raises(capi.L3DError, match="error 1.*unknown view"):
        l.project_result([12345])
    with pytest.raises(capi.L3DError, match="error 1.*the view"):
        l.overlay(scene.views[0]["id"], grey[:-1])
    with pytest.raises(capi.L3DError, match="error 1.*view ids"):
        l.project_result(None, cameras=_cams(scene), select="observed")
    fresh = Line3D("", matchingNeighbors=N, device=0)
    try:
        load_scene(fresh, scene)
        with pytest.raises(capi.L3DError, match="error 1.*no result yet"):
            fresh.project_result([scene.views[0]["id"]])
        with pytest.raises(capi.L3DError, match="error 1.*no result yet"):
            fresh.overlay(scene.views[0]["id"], grey)
    finally:
        fresh.close()
