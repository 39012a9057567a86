"""Writes tests/golden/merge_small.npz (CPU only: python tests/golden/make_golden_merge.py): the merging of duplicate lines on
make_scene(32, 100, 6, seed=11), with and without the diffusion, by the ORACLE alone (its result and its own align as the refit) and the model of
tests/merge_model.py (the rule, the tolerances, the rounds; defaults dist 4 px, 5 degrees, gap 0, 3 rounds).  Per kind ("plain", "rdd") and round r:
<kind>_r<r>_pairs, _group, and the result after the round as _ids (camera, segment), _id_off, _pts (6 per 3-D segment), _pt_off; per kind
_counts (lines before, lines after, rounds, pairs of round 1, groups merged, lines released, empty refits, 0), _final_index, _n_sources, _gt (the
majority ground-truth id of every line of the last result) and _r0_* for the oracle's result before any merging."""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import l3d_oracle_pipeline as op  # noqa: E402
import merge_model as mm  # noqa: E402
from line3d_amd.synth import make_scene  # noqa: E402

SCENE = (32, 100, 6, 11)


def pack(out, prefix, result):
    ids = np.array([k for m, _ in result for k in m], np.int32).reshape(-1, 2)
    pts = np.concatenate([np.asarray(s, np.float64).reshape(-1, 6) for _, s in result]) if result else np.zeros((0, 6))
    out[prefix + "_ids"], out[prefix + "_pts"] = ids, pts
    out[prefix + "_id_off"] = np.cumsum([0] + [len(m) for m, _ in result]).astype(np.int64)
    out[prefix + "_pt_off"] = np.cumsum([0] + [len(np.asarray(s).reshape(-1, 6)) for _, s in result]).astype(np.int64)


def main():
    scene = make_scene(SCENE[0], SCENE[1], SCENE[2], seed=SCENE[3])
    views = {int(v["id"]): v for v in scene.views}
    out = {"scene": np.array(SCENE, np.int64)}
    for kind, diffusion in (("plain", False), ("rdd", True)):
        o = op.run_scene(scene, SCENE[2], diffusion)

        def refit(union):
            t3 = OrderedDict()
            for seg in union:
                if seg in o.best_match:
                    s3 = o.best_match[seg]["seg3D"]
                    t3[seg] = (o.inverse_transform(s3[0:3]), o.inverse_transform(s3[3:6]))
            return np.array([list(P) + list(Q) for P, Q in o.align(t3)], np.float64).reshape(-1, 6)

        start = [([(int(c), int(s)) for c, s in m], np.array([list(P) + list(Q) for P, Q in segs], np.float64).reshape(-1, 6)) for m, segs in o.result]
        merged, rounds, final_index, n_sources = mm.merge_rounds(start, views, refit)
        pack(out, kind + "_r0", start)
        for r, rec in enumerate(rounds, 1):
            out["%s_r%d_pairs" % (kind, r)], out["%s_r%d_group" % (kind, r)] = rec["pairs"], rec["group"]
            pack(out, "%s_r%d" % (kind, r), rec["result"])
        out[kind + "_counts"] = np.array([len(start), len(merged), len(rounds), len(rounds[0]["pairs"]), sum(r["merged"] for r in rounds),
                                          sum(r["released"] for r in rounds), sum(r["empty_refits"] for r in rounds), 0], np.int32)
        out[kind + "_final_index"], out[kind + "_n_sources"] = final_index, n_sources
        gt_of = lambda m: np.bincount([int(views[c]["gt"][s]) for c, s in m])
        out[kind + "_gt"] = np.array([gt_of(m).argmax() for m, _ in merged], np.int32)
        mixed = sum(1 for (m, _), ns in zip(merged, n_sources) if ns > 1 and (gt_of(m) > 0).sum() > 1)
        print("%s: lines per round %s, pairs %s, released %s, empty refits %s; %d true segments covered before, %d after; %d merged lines mix ids; "
              "3-D segments per merged line: at most %d"
              % (kind, [len(start)] + [r["n_after"] for r in rounds], [len(r["pairs"]) for r in rounds], [r["released"] for r in rounds],
                 [r["empty_refits"] for r in rounds], len({gt_of(m).argmax() for m, _ in start}), len(set(out[kind + "_gt"].tolist())), mixed,
                 max([len(s) for (_, s), ns in zip(merged, n_sources) if ns > 1] or [0])))
    np.savez_compressed(os.path.join(HERE, "merge_small.npz"), **out)
    print("wrote merge_small.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "merge_small.npz")))


if __name__ == "__main__":
    main()
