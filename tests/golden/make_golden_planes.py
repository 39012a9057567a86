"""Writes tests/golden/planes_small.npz (CPU only: python tests/golden/make_golden_planes.py): the planes of the lines of tests/golden/junction_small.npz
-- the oracle's lines of make_scene_boxes(32, 8, 6, seed 1) with the junctions' own tolerances -- by the model of tests/plane_model.py alone.  The seeds
are the L and T records of the junction golden, in record order; the parameters are the object's defaults (the lines' own tol, 10 degrees, min_lines 3;
cos_max is the junctions').  Face truth comes from scene.corners and scene.corner_edges: a face is covered when at least 3 of its 4 edges have a line,
recalled when one plane has members on at least 3 of its edges.  Conditions: at least 9 of 10 covered faces are recalled, no plane's seeds mix boxes,
and the true corners of every recalled face lie within 1.0 x the largest member tolerance of its plane.
Stored: lines, tol, seeds; planes, members, hyp_plane, counts of the model; edge_of (the majority ground-truth edge of every line), line_box; covered,
recalled (face indices 6 box + 2 axis + side), plane_of (per recalled face), mixed, unmatched (plane indices), corner_ratio."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import plane_model as pm  # noqa: E402
from line3d_amd.synth import make_scene_boxes  # noqa: E402

COS10 = math.cos(10.0 * math.pi / 180.0)
INTERIOR = 2


def seeds_of(records):
    """the L and T records of a junction search as seed pairs, in record order"""
    keep = (records["where_i"] != INTERIOR) | (records["where_j"] != INTERIOR)
    return np.stack([records["i"][keep], records["j"][keep]], axis=1).astype(np.int32).reshape(-1, 2)


def main():
    g = np.load(os.path.join(HERE, "junction_small.npz"))
    shape = [int(x) for x in g["scene"]]
    scene = make_scene_boxes(shape[0], shape[1], shape[2], seed=shape[3])
    views = {int(v["id"]): v for v in scene.views}
    ids, off = g["ids"], g["id_off"]
    edge_of = np.array([np.bincount([int(views[int(c)]["gt"][int(s)]) for c, s in ids[off[l]:off[l + 1]]]).argmax() for l in range(len(off) - 1)], np.int32)
    lines, tol, seeds = g["lines"], g["tol"], seeds_of(g["records"])
    out = pm.planes(lines, tol, seeds, COS10, COS10, 3)
    fr = pm.face_recall(scene.corners, scene.corner_edges, edge_of, g["line_box"], tol, out)
    print("%d lines, %d seeds, counts %s; faces covered %d, recalled %d; planes that mix boxes %d, that match no face %d; corner ratio %.3f; hypotheses per plane %d to %d, "
          "lines per plane %d to %d" % (len(lines), len(seeds), out["counts"].tolist(), len(fr["covered"]), len(fr["recalled"]), len(fr["mixed"]), len(fr["unmatched"]),
                                        fr["corner_ratio"], out["planes"]["n_hyp"].min(), out["planes"]["n_hyp"].max(), out["planes"]["n_lines"].min(),
                                        out["planes"]["n_lines"].max()))
    if 10 * len(fr["recalled"]) < 9 * len(fr["covered"]) or fr["mixed"] or not fr["corner_ratio"] <= 1.0:
        raise SystemExit("the conditions are not met")
    path = os.path.join(HERE, "planes_small.npz")
    np.savez_compressed(path, lines=lines, tol=tol, seeds=seeds, planes=out["planes"], members=out["members"], hyp_plane=out["hyp_plane"], counts=out["counts"],
                        edge_of=edge_of, line_box=g["line_box"], covered=np.array(fr["covered"], np.int32), recalled=np.array(fr["recalled"], np.int32),
                        plane_of=np.array(fr["plane_of"], np.int32), mixed=np.array(fr["mixed"], np.int32), unmatched=np.array(fr["unmatched"], np.int32),
                        corner_ratio=np.float64(fr["corner_ratio"]))
    print("wrote planes_small.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
