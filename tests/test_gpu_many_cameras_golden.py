"""The line fit's camera overflow as the PRODUCT reaches it: make_scene(72, 40, 71, seed=571) -- 72 views, every one a neighbour of every other
-- against tests/golden/many_cameras.npz, which the ORACLE ALONE produced (tests/golden/make_golden_many_cameras.py, about 10 s).  Three of its
83 lines are seen from more than 64 cameras: their clusters leave k_fit_clusters' register sweep for the sequential one (l3d_linefit.hip).

Every view's kept list and median bit for bit, the affinity list bit for bit, the lines within the 1e-4 of the acceptance rule -- and for the
lines with more than 64 cameras the structure: which input point every emitted end point is (tests/linefit_model.py on the oracle's
inverse-transformed member end points, which the golden holds).  The product's hypotheses agree with the oracle's to 1e-12 relative, not bit
for bit (the scene normalisation goes through an SVD, tests/test_gpu_pipeline_parity.py::_check_resident_products_against_oracle), so the
index check is: the member point nearest to the emitted end point is the model's, and it is within 1e-9 -- three orders above that
disagreement at coordinates of a few units, three below the smallest distance between two different member points (the generator asserts > 1e-6)."""
import hashlib
import os

import numpy as np
import pytest

import linefit_model as lm
from helpers import assert_lines_equal

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "many_cameras.npz")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _golden_lines(g, tag):
    ids, id_off, pts, pt_off = g[tag + "_ids"], g[tag + "_id_off"], g[tag + "_pts"], g[tag + "_pt_off"]
    out = []
    for k in range(len(id_off) - 1):
        seg2 = [(int(c), int(s)) for c, s in ids[id_off[k]:id_off[k + 1]]]
        seg3 = [(p[:3], p[3:]) for p in pts[pt_off[k]:pt_off[k + 1]]]
        out.append((seg2, seg3))
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def product(golden):
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    V, S, N, seed = (int(x) for x in golden["shape"])
    scene = make_scene(V, S, N, seed=seed)
    l = Line3D("", matchingNeighbors=N)
    l.keep_view_matches(True)
    load_scene(l, scene)
    l.compute3Dmodel(False)
    yield l, scene
    l.close()


def test_many_cameras_every_kept_list_and_median_equals_the_oracles(golden, product):
    l, scene = product
    assert len(golden["kept_sha256"]) == len(scene.views) == 72
    for k, v in enumerate(scene.views):
        m, med = l.view_matches(v["id"])
        assert len(m) == int(golden["kept_n"][k]), "view %d: %d kept matches, the oracle keeps %d" % (v["id"], len(m), int(golden["kept_n"][k]))
        assert _sha(m) == str(golden["kept_sha256"][k]), "view %d: kept list differs from the oracle's" % v["id"]
        if int(golden["kept_n"][k]) and k + 1 < len(scene.views):          # the early-return view leaves the median untouched (cudawrapper.cu:877-878)
            assert np.float32(med) == golden["median"][k], "view %d: median" % v["id"]
    edges, n_nodes = l.affinity()
    assert len(edges) == int(golden["affinity_n"]) and n_nodes == int(golden["n_nodes"])
    assert _sha(edges) == str(golden["affinity_sha256"]), "affinity list (clusterSegments2D) differs from the oracle's"


def test_many_cameras_lines_and_the_structure_of_the_overflowing_ones(golden, product):
    l, _scene = product
    got = l.getResult()
    exp = _golden_lines(golden, "plain")
    assert len(exp) == 83
    assert assert_lines_equal(got, exp, tol=1e-4) <= 1e-4
    by_ids = {tuple(sorted(seg2)): seg3 for seg2, seg3 in got}
    assert len(golden["big_line"]) >= 3
    for n, k in enumerate(golden["big_line"]):
        seg2, exp3 = exp[int(k)]
        cams = [c for c, _s in seg2]
        assert seg2 == sorted(seg2) and len(set(cams)) > 64 and lm.path_of(len(cams), cams) == "overflow"
        pts = golden["big_pts"][golden["big_off"][n]:golden["big_off"][n + 1]]
        assert len(pts) == 2 * len(seg2)
        structure = lm.fit_cluster(pts, cams)["structure"]
        seg3 = by_ids[tuple(seg2)]
        assert len(seg3) == len(structure) == len(exp3) >= 1
        for (s, e), (ms, me) in zip(seg3, structure):
            for p, want in ((s, ms), (e, me)):
                d = np.abs(pts - p).max(axis=1)
                assert int(np.argmin(d)) == want and d[want] <= 1e-9, "line %d: end point %r is member point %d (%.3g away), the model's is %d (%.3g away)" % (
                    int(k), p, int(np.argmin(d)), d.min(), want, d[want])
