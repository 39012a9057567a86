#!/usr/bin/env python3
"""What the refinement of the result costs and what it buys: finish() of config 2 (64 x 2000 x 12) with the option off and on, k_refine_lines alone, the
pixel rms before and after, and the distance of the lines to the synthetic scene's ground truth.  Writes profiles/refine_times.txt.

    python scripts/time_refine.py --parent /path/to/the/parent/commit's/libline3d_amd.so [--out F]

The procedure of scripts/time_batch.py: a library is measured in a process of its own (L3D_LIBRARY), warm-up rounds first, the variants of a process
alternating round by round; a round is prepare-once, then matchViews + finish() with only finish() timed.  (a) the parent commit's build, option off (it
has no other), run twice -- before and after; (b) this build, off and on alternating.  Off may not be slower than the parent by more than the parent's two
runs differ; the last lines of the file say how that came out.  For the option on no time is claimed: the file records what came out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (64, 2000, 12)


def truth_distance(scene, result):
    """mean distance of the lines' 3-D end points to the ground-truth line most of their 2-D segments come from (units of the scene)"""
    gt = {v["id"]: v["gt"] for v in scene.views}
    dist = []
    for seg2, seg3 in result:
        if not seg3:
            continue
        ids = np.array([gt[c][s] for c, s in seg2])
        k = int(np.bincount(ids).argmax())
        a, b = scene.segs3d[k, :3], scene.segs3d[k, 3:]
        e = (b - a) / np.linalg.norm(b - a)
        pts = np.array([p for pair in seg3 for p in pair])
        dist.append(float(np.linalg.norm(np.cross(pts - a, e), axis=1).mean()))
    return float(np.mean(dist)), len(dist)


def worker(a):
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    scene = make_scene(*SHAPE, seed=1234)
    l3d = Line3D("", matchingNeighbors=SHAPE[2])
    load_scene(l3d, scene)
    l3d.prepare()
    variants = ["off", "on"] if a.with_on else ["off"]
    out = {v: [] for v in variants}
    info = {}
    ctx = l3d.context()
    for k in range(a.warmup + a.rounds):
        for v in variants:
            if a.with_on:
                l3d.set_refinement(v == "on")
            l3d.match_views()
            t0 = time.perf_counter()
            l3d.finish(False)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                out[v].append(dt)
    for v in variants:
        if a.with_on:
            l3d.set_refinement(v == "on")
        l3d.match_views()
        if v == "on":
            ctx.profile_enable(True)
            ctx.profile_only("refine_lines")
            ctx.profile_reset()
        l3d.finish(False)
        res = l3d.getResult()
        d, n = truth_distance(scene, res)
        info[v] = {"lines": len(res), "members": int(sum(len(s2) for s2, _ in res)), "truth_distance": d, "lines_measured": n}
        if v == "on":
            launches, ms = ctx.profile_get("refine_lines")
            ctx.profile_enable(False)
            ref = l3d.refinement()
            info[v].update(kernel_ms=ms, kernel_launches=launches, status=np.bincount(ref["status"], minlength=4).tolist(),
                           rms_before=float(np.sqrt(np.mean(ref["rms_before"] ** 2))), rms_after=float(np.sqrt(np.mean(ref["rms_after"] ** 2))),
                           rms_rose=int((ref["rms_after"] > ref["rms_before"]).sum()))
    l3d.close()
    print("RESULT " + json.dumps({"ms": out, "info": info}))


def run_worker(a, library, with_on):
    env = dict(os.environ)
    if library:
        env["L3D_LIBRARY"] = library
    else:
        env.pop("L3D_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(a.warmup), "--rounds", str(a.rounds)] + (["--with-on"] if with_on else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def stats(ms):
    ms = np.array(ms)
    return "median %8.3f ms   p10 %8.3f  p90 %8.3f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's build of the library (kept outside the repository's history)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--with-on", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent:
        ap.error("--parent is needed")
    p1 = run_worker(a, os.path.abspath(a.parent), False)
    this = run_worker(a, None, True)
    p2 = run_worker(a, os.path.abspath(a.parent), False)
    lines = ["finish() of config 2 (%d x %d x %d), warm-up %d, %d timed rounds per variant, variants alternating; a library per process" % (SHAPE + (a.warmup, a.rounds)),
             "  parent, run 1, off   %s" % stats(p1["ms"]["off"]), "  this build,    off   %s" % stats(this["ms"]["off"]), "  this build,    on    %s" % stats(this["ms"]["on"]),
             "  parent, run 2, off   %s" % stats(p2["ms"]["off"])]
    a1, a2, b, on = (float(np.median(x)) for x in (p1["ms"]["off"], p2["ms"]["off"], this["ms"]["off"], this["ms"]["on"]))
    i_on, i_off = this["info"]["on"], this["info"]["off"]
    lines += ["  k_refine_lines alone (event brackets, one launch): %.3f ms for %d lines with %d members" % (i_on["kernel_ms"], i_on["lines"], i_on["members"]),
              "  refinement on costs %.3f ms of finish() (medians)" % (on - b),
              "  status counts (0 refined, 1 start kept, 2 degenerate, 3 sweep empty): %r; lines whose rms rose: %d" % (i_on["status"], i_on["rms_rose"]),
              "  pooled pixel rms of the members' end points: before %.4f, after %.4f" % (i_on["rms_before"], i_on["rms_after"]),
              "  mean distance of the lines' end points to their ground-truth lines (scene units; %d lines): unrefined %.6f, refined %.6f"
              % (i_on["lines_measured"], i_off["truth_distance"], i_on["truth_distance"]),
              "option off: parent %.3f / %.3f (spread %.3f), this build %.3f: %s" % (a1, a2, abs(a1 - a2), b, "not slower" if b - min(a1, a2) <= abs(a1 - a2) else
                                                                                   "SLOWER than the spread of the parent's two runs allows (a miss)")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
