"""Generates tests/golden/many_cameras.npz: make_scene(72, 40, 71, seed=571) -- 72 small views, every view a neighbour of every other,
built as tests/test_gpu_pipeline_parity.py::test_many_neighbours_parity builds its scenes -- through the ORACLE ALONE, no GPU input:

    python tests/golden/make_golden_many_cameras.py [--out tests/golden/many_cameras.npz]

The scene is there for the clusters it gives the line fit: with more than 64 views a 3-D line can be seen from more than 64 cameras, and
k_fit_clusters (l3d_linefit.hip) then leaves its register sweep for the sequential one (and, above 128 members, its LDS arrays for
global scratch).  The generator asserts that at least 3 lines have more than 64 cameras.  About 10 s on one core.

Fixture = data only, in the layout of config2_full.npz (make_golden_config2.py): per view the sha256 of the kept list, its size and
median; the affinity list's digest; the final lines without diffusion (2-D segment ids and 3-D end points).  For the lines with more
than 64 cameras additionally the oracle's inverse-transformed end points of their members (big_line: the line's index, big_off / big_pts:
2 points per member in member order), so that the GPU test can state which input point every emitted end point is
(tests/linefit_model.py); the generator asserts that the model and the oracle's align() agree on that for these lines."""
import argparse
import os
import sys
import time
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import l3d_oracle_pipeline as op  # noqa: E402
import linefit_model as lm  # noqa: E402
from line3d_amd.synth import make_scene  # noqa: E402
from make_golden_config2 import match_view_threaded, pack_lines, sha  # noqa: E402

V, S, N, SEED = 72, 40, 71, 571


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "many_cameras.npz"))
    a = ap.parse_args()
    t0 = time.time()
    scene = make_scene(V, S, N, seed=SEED)
    o = op.OracleLine3D(matching_neighbors=N)
    for v in scene.views:
        o.add_image_fixed_sim(v["id"], v["width"], v["height"], v["segments"], v["K"], v["R"], v["t"], v["sims"])
    o.computation = True
    o.track_potential = True
    o.matched, o.potential, o.result = {}, {}, []
    o.find_visual_neighbors()
    o.transform_geometry()
    g = {"shape": np.array([V, S, N, SEED], np.int64)}
    kept_sha, kept_n, medians = [], [], []
    for v in sorted(o.visual_neighbors):                      # match_views, line3D.cc:620-648
        for n in o.visual_neighbors[v]:
            o._fundamental(v, n)
        _mv, _in_arr, matches, median = match_view_threaded(o, v, 1)
        o.matching_commit(v, matches, median)
        kept_sha.append(sha(matches))
        kept_n.append(len(matches))
        medians.append(np.float32(median))
    g["kept_sha256"] = np.array(kept_sha)
    g["kept_n"] = np.array(kept_n, np.int64)
    g["median"] = np.array(medians, np.float32)
    o.greedy_selection()
    g["n_hypotheses"] = np.int64(len(o.best_match))
    o.cluster_segments_2D(False)
    ids, id_off, pts, pt_off = pack_lines(o.result)
    g["plain_ids"], g["plain_id_off"], g["plain_pts"], g["plain_pt_off"] = ids, id_off, pts, pt_off
    g["affinity_sha256"] = np.array(sha(o.affinity))
    g["affinity_n"] = np.int64(len(o.affinity))
    g["n_nodes"] = np.int64(len(o.local2global))
    big_line, big_pts, big_off = [], [], [0]
    for k, (seg2, seg3) in enumerate(o.result):
        cams = [int(c) for c, _s in seg2]
        if len(set(cams)) <= 64:
            continue
        rows = []
        for key in seg2:
            s3 = o.best_match[key]["seg3D"]
            rows += [o.inverse_transform(s3[0:3]), o.inverse_transform(s3[3:6])]
        # the model against the oracle's own align() on these members: the same input points emitted
        index = {id(p): i for i, p in enumerate(rows)}
        t3 = OrderedDict((key, (rows[2 * m], rows[2 * m + 1])) for m, key in enumerate(seg2))
        by_align = [(index[id(s)], index[id(e)]) for s, e in o.align(t3)]
        fit = lm.fit_cluster(np.array(rows), cams)
        assert by_align == fit["structure"] and len(by_align) == len(seg3)
        for (s, e), (P, Q) in zip(by_align, seg3):
            assert rows[s].tobytes() == np.asarray(P).tobytes() and rows[e].tobytes() == np.asarray(Q).tobytes()
        P = np.array(rows)
        sep = min(np.abs(P - p).max(axis=1)[np.abs(P - p).max(axis=1) > 0].min() for p in P)
        assert sep > 1e-6, sep                                # (distinct member points are far apart against the 1e-9 of the GPU test's index check)
        print("line %d: %d members, %d cameras, %d segments, path %s, margins %r" % (k, len(seg2), len(set(cams)), len(seg3), lm.path_of(len(cams), cams),
                                                                                      lm.linefit_conditions(P, fit)), flush=True)
        big_line.append(k)
        big_pts += rows
        big_off.append(len(big_pts))
    assert len(big_line) >= 3, "only %d lines with more than 64 cameras" % len(big_line)
    g["big_line"], g["big_pts"], g["big_off"] = np.array(big_line, np.int64), np.array(big_pts, np.float64).reshape(-1, 3), np.array(big_off, np.int64)
    np.savez_compressed(a.out, **g)
    print("%d kept matches, %d hypotheses, %d lines, %d of them with more than 64 cameras; written %s (%d bytes) in %.0f s"
          % (int(g["kept_n"].sum()), len(o.best_match), len(o.result), len(big_line), a.out, os.path.getsize(a.out), time.time() - t0))


if __name__ == "__main__":
    main()
