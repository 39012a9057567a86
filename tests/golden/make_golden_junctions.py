"""Writes tests/golden/junction_small.npz (CPU only: python tests/golden/make_golden_junctions.py): the junctions of the lines of
make_scene_boxes(32, 8, 6, seed) by the ORACLE pipeline alone (its result, no diffusion) and the model of tests/junction_model.py (the rule, the
tolerances and extensions; defaults 4 px, 12 px, 10 degrees, 0.25).  The first seed from SEEDS on is taken that meets both conditions:
  * no decision of the rule on the oracle's lines lies within MARGIN = 1e-3 of its threshold, relative to the larger of the threshold's size and the
    two lines' lengths (1 for the cosine): the device's lines may differ from the oracle's by 1e-4 in their end points (tests/test_gpu_config2_golden.py),
    which then cannot flip a decision.  The decisions: whether a pair passes, over all pairs (a pair that passes: every comparison of the pair test
    clears its threshold by the margin; a pair that does not: at least one comparison fails by the margin, all comparisons being evaluated whatever
    the others say -- an edge of another box whose angle happens to lie at 10 degrees is rejected by its gap, safely); where on a line; the longest
    line of every component with an edge against its runner-up; the smallest gap of every attached end against the next;
  * at least 0.8 of the covered true corners are recalled.  A corner is COVERED when at least two reconstructed lines that show edges of that corner
    (majority ground truth) have an end within their tol + ext of it; it is RECALLED when one vertex holds such ends of at least two of these lines.
Stored: scene (views, boxes, neighbours, seed), the oracle's lines as ids (camera, segment), id_off, pts (6 per 3-D segment), pt_off; lines, tol, ext;
records, node_vertex, vertices, node_attach, counts of the model; per_line (vertex of P, vertex of Q, line P rests on, line Q rests on); line_box (the
box of every line's majority edge); covered, recalled (corner indices)."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import junction_model as jm  # noqa: E402
import l3d_oracle_pipeline as op  # noqa: E402
from line3d_amd.synth import make_scene_boxes  # noqa: E402

SHAPE = (32, 8, 6)
SEEDS = range(1, 40)
MARGIN = 1e-3
COS_MAX = math.cos(10.0 * math.pi / 180.0)


def closest_decision(tab, out):
    """the smallest relative distance of a decision from its threshold, and which decision it is"""
    worst = (np.inf, "")

    def see(x, thr, scale, what):
        nonlocal worst
        m = abs(float(x) - float(thr)) / max(abs(float(thr)), scale)
        if m < worst[0]:
            worst = (m, what)

    def rel(x, thr, scale):
        m = abs(float(x) - float(thr)) / max(abs(float(thr)), scale)
        return m if np.isfinite(m) else 0.0

    n = len(tab)
    for i in range(n):
        for j in range(i + 1, n):
            li, lj = tab[i], tab[j]
            t = jm.pair_terms(li, lj)
            scale = float(max(li["L"], lj["L"]))
            tol = max(li["tol"], lj["tol"])
            # the comparisons of the pair test, all of them evaluated: (holds, distance from the threshold)
            cond = [(bool(abs(t["b"]) <= COS_MAX), rel(abs(t["b"]), COS_MAX, 1.0)), (bool(t["g"] <= tol), rel(t["g"], tol, scale))]
            for par, l in ((t["s"], li), (t["t"], lj)):
                cond.append((bool(-l["ext"] <= par), rel(par, -l["ext"], scale)))
                cond.append((bool(par <= l["L"] + l["ext"]), rel(par, l["L"] + l["ext"], scale)))
            failed = [m for ok, m in cond if not ok]
            if failed:                               # rejected: as safely as the comparison that fails by the most
                see(max(failed), 0.0, 1.0, "rejection of %d %d" % (i, j))
                continue
            see(min(m for _, m in cond), 0.0, 1.0, "acceptance of %d %d" % (i, j))
            for par, l in ((t["s"], li), (t["t"], lj)):
                for thr in (l["ext"], l["L"] / 2, l["L"] - l["ext"]):
                    see(par, thr, scale, "where %d %d" % (i, j))
    comp = out["comp"]
    for c in set(comp.tolist()):
        mem = np.nonzero(comp == c)[0]
        if len(mem) >= 2:
            L = sorted({float(tab[v >> 1]["L"]) for v in mem}, reverse=True)
            if len(L) >= 2:
                see(L[1], L[0], 0.0, "representative of component %d" % c)
    rec = out["records"]
    kinds = jm.kinds_of(rec)
    for v in np.nonzero(out["node_attach"] >= 0)[0]:
        gaps = sorted(float(r["gap"]) for r, k in zip(rec, kinds) if k == jm.KIND_T and v in (2 * r["i"] + r["where_i"], 2 * r["j"] + r["where_j"]))
        if len(gaps) >= 2:
            see(gaps[1], gaps[0], float(tab[v >> 1]["L"]), "attachment of node %d" % v)
    return worst


def build(seed):
    scene = make_scene_boxes(SHAPE[0], SHAPE[1], SHAPE[2], seed=seed)
    views = {int(v["id"]): v for v in scene.views}
    o = op.run_scene(scene, SHAPE[2], False)
    result = [([(int(c), int(s)) for c, s in m], np.array([list(P) + list(Q) for P, Q in segs], np.float64).reshape(-1, 6)) for m, segs in o.result]
    lines, tol, ext = jm.result_table(result, views)
    out = jm.junctions(lines, tol, ext, COS_MAX)
    tab = [jm.prepare(lines[k], tol[k], ext[k]) for k in range(len(lines))]
    return scene, views, result, lines, tol, ext, out, tab


def main():
    for seed in SEEDS:
        scene, views, result, lines, tol, ext, out, tab = build(seed)
        if any(t is None for t in tab):
            print("seed %d: a line is not eligible" % seed)
            continue
        margin, what = closest_decision(tab, out)
        covered, recalled, line_box = jm.corner_recall(scene, result, views, lines, tol, ext, out["node_vertex"])
        share = len(recalled) / max(1, len(covered))
        mixed = sum(1 for k in range(len(out["vertices"])) if len({int(line_box[v >> 1]) for v in np.nonzero(out["node_vertex"] == k)[0]}) > 1)
        print("seed %d: %d lines, counts %s, closest decision %.2e (%s), corners covered %d, recalled %d (%.3f), vertices that mix boxes %d"
              % (seed, len(lines), out["counts"].tolist(), margin, what, len(covered), len(recalled), share, mixed))
        if margin <= MARGIN or share < 0.8 or mixed:
            continue
        n = len(lines)
        per_line = np.full((n, 4), -1, np.int32)
        for l in range(n):
            for e in (0, 1):
                per_line[l, e] = out["node_vertex"][2 * l + e]
                a = out["node_attach"][2 * l + e]
                if a >= 0:
                    r = out["records"][a]
                    per_line[l, 2 + e] = r["j"] if r["i"] == l else r["i"]
        data = dict(scene=np.array(SHAPE + (seed,), np.int64), margin=np.float64(margin),
                    ids=np.array([k for m, _ in result for k in m], np.int32).reshape(-1, 2), id_off=np.cumsum([0] + [len(m) for m, _ in result]).astype(np.int64),
                    pts=np.concatenate([s for _, s in result]), pt_off=np.cumsum([0] + [len(s) for _, s in result]).astype(np.int64),
                    lines=lines, tol=tol, ext=ext, records=out["records"], node_vertex=out["node_vertex"], vertices=out["vertices"], node_attach=out["node_attach"],
                    counts=out["counts"], per_line=per_line, line_box=line_box, covered=np.array(covered, np.int32), recalled=np.array(recalled, np.int32))
        path = os.path.join(HERE, "junction_small.npz")
        np.savez_compressed(path, **data)
        print("wrote junction_small.npz: seed %d, %d bytes" % (seed, os.path.getsize(path)))
        return
    raise SystemExit("no seed of %s meets the conditions" % list(SEEDS))


if __name__ == "__main__":
    main()
