#!/usr/bin/env python3
"""What the planes of 3-D lines cost: finish() of config 2 (64 x 2000 x 12, seed 20260) with the option off and on, alternating round by round in one
process, and the kernels of l3d_plane_lines on the result's own lines with the seeds of its junction search.  Writes profiles/planes_times.txt.

    python scripts/time_planes.py [--out F]

The procedure of scripts/time_junctions.py: the library is measured in a process of its own, warm-up rounds first; a round is prepare-once, then
matchViews + finish() with only finish() timed.  With the option on, finish() also runs the junction search (the junctions option itself stays off), so
the difference is the price of both.  Nothing is held to a time: the file records what came out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_junctions import SEED, SHAPE, stats, table_of  # noqa: E402

KERNELS = ("plane_prepare", "plane_hyp", "plane_count", "plane_scan", "plane_write", "plane_cc_hook", "plane_cc_compress", "plane_rep", "plane_star", "plane_flag",
           "plane_cscan", "plane_keys", "plane_sort", "plane_param", "plane_mcount", "plane_keep", "plane_pscan", "plane_mmask", "plane_mscan", "plane_mwrite", "plane_seed",
           "plane_extent", "plane_finish")


def kernel_times(ctx, lines, tol, seeds, reps):
    ctx.plane_lines(lines, tol, seeds)                        # warm-up: code objects, buffers
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = ctx.plane_lines(lines, tol, seeds)
    wall = (time.perf_counter() - t0) * 1e3 / reps
    prof = {k: ctx.profile_get(k) for k in KERNELS}
    ctx.profile_enable(False)
    return {"n": len(lines), "m": len(seeds), "counts": out["counts"].tolist(), "call_ms": wall, "kernels": {k: [int(v[0]) // reps, float(v[1]) / reps] for k, v in prof.items()}}


def worker(a):
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    scene = make_scene(*SHAPE, seed=SEED)
    l3d = Line3D("", matchingNeighbors=SHAPE[2])
    load_scene(l3d, scene)
    l3d.prepare()
    out = {"off": [], "on": []}
    for k in range(a.warmup + a.rounds):
        for v in ("off", "on"):
            l3d.set_planes(v == "on")
            l3d.match_views()
            t0 = time.perf_counter()
            l3d.finish(False)
            if k >= a.warmup:
                out[v].append((time.perf_counter() - t0) * 1e3)
    l3d.set_planes(True)
    l3d.match_views()
    l3d.finish(False)
    info = {"object": {k: v for k, v in l3d.planes().items() if not hasattr(v, "shape")}}
    ctx = l3d.context()
    lines, tol, ext = table_of(scene, l3d.getResult())
    rec = ctx.junction_lines(lines, tol, ext)["records"]
    keep = (rec["where_i"] != 2) | (rec["where_j"] != 2)
    seeds = np.stack([rec["i"][keep], rec["j"][keep]], axis=1).astype(np.int32).reshape(-1, 2)
    info["call"] = kernel_times(ctx, lines, tol, seeds, 10)
    l3d.close()
    print("RESULT " + json.dumps({"ms": out, "info": info}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(a.warmup), "--rounds", str(a.rounds)], capture_output=True, text=True,
                       timeout=a.worker_timeout)
    if r.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    this = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    b, on = float(np.median(this["ms"]["off"])), float(np.median(this["ms"]["on"]))
    s = this["info"]["call"]
    k = s["kernels"]
    lines = ["finish() of config 2 (%d x %d x %d, seed %d), warm-up %d, %d timed rounds per variant, variants alternating" % (SHAPE + (SEED, a.warmup, a.rounds)),
             "  planes off   %s" % stats(this["ms"]["off"]), "  planes on    %s" % stats(this["ms"]["on"]),
             "  planes on (defaults: 4 px, 10 degrees, 3 lines; junctions off, so their search runs for the seeds) cost %.3f ms of finish() (medians); what they found: %s"
             % (on - b, json.dumps(this["info"]["object"])),
             "  l3d_plane_lines on the result's lines: n = %d, m = %d seeds, counts (eligible lines, hypotheses, edges, components, released, dropped, planes, members) %r; "
             "the whole call %.3f ms (upload, kernels, download)" % (s["n"], s["m"], s["counts"], s["call_ms"]),
             "    per call, event brackets (launches, ms): " + "  ".join("%s %d %.3f" % (n[6:], k[n][0], k[n][1]) for n in KERNELS)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
