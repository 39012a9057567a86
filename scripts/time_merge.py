#!/usr/bin/env python3
"""What the merging of duplicate lines costs and what it does: finish() of config 2 (64 x 2000 x 12, seed 20260) with the option off and on against the
parent commit, the kernels of the pair search on the result's own lines and on a synthetic table of 10^5 lines, the line counts per round, and the
distance of the lines to the synthetic scene's ground truth before and after.  Writes profiles/merge_times.txt.

    python scripts/time_merge.py --parent /path/to/the/parent/commit's/libline3d_amd.so [--out F]

The procedure of scripts/time_refine.py: a library is measured in a process of its own (L3D_LIBRARY), warm-up rounds first, the variants of a process
alternating round by round; a round is prepare-once, then matchViews + finish() with only finish() timed.  (a) the parent commit's build, option off (it
has no other), run twice -- before and after; (b) this build, off and on alternating.  Off may not be slower than the parent by more than the parent's two
runs differ; the last line of the file says how that came out.  For the option on no time is claimed: the file records what came out."""
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
SEED = 20260
KERNELS = ("merge_prepare", "merge_count", "merge_scan", "merge_write", "merge_cc_hook", "merge_cc_compress", "merge_rep", "merge_star", "merge_group")


def truth_distance(scene, result):
    """mean distance of the lines' 3-D end points to the ground-truth line most of their 2-D segments come from (units of the scene), and the number of
    ground-truth segments that more than one line reports"""
    gt = {v["id"]: v["gt"] for v in scene.views}
    dist, ids_seen = [], []
    for seg2, seg3 in result:
        if not seg3:
            continue
        ids = np.array([gt[c][s] for c, s in seg2])
        k = int(np.bincount(ids).argmax())
        ids_seen.append(k)
        a, b = scene.segs3d[k, :3], scene.segs3d[k, 3:]
        e = (b - a) / np.linalg.norm(b - a)
        pts = np.array([p for pair in seg3 for p in pair])
        dist.append(float(np.linalg.norm(np.cross(pts - a, e), axis=1).mean()))
    return float(np.mean(dist)), len(dist), int((np.bincount(ids_seen) > 1).sum())


def lines_and_tol(scene, result, dist_px):
    """the table the pipeline hands to l3d_merge_lines in its first round: P, Q and dist_px times the mean of z / f over the members' views"""
    R2 = np.array([v["R"][2] for v in scene.views])
    t2 = np.array([v["t"][2] for v in scene.views])
    f = np.array([(abs(v["K"][0, 0]) + abs(v["K"][1, 1])) / 2.0 for v in scene.views])
    index = {v["id"]: i for i, v in enumerate(scene.views)}
    lines = np.array([np.concatenate([s3[0][0], s3[-1][1]]) for _, s3 in result])
    tol = np.zeros(len(lines))
    for k, (s2, _) in enumerate(result):
        cams = np.array([index[c] for c, _ in s2])
        q = (R2[cams] @ ((lines[k, :3] + lines[k, 3:]) / 2.0) + t2[cams]) / f[cams]
        q = q[q > 0]
        tol[k] = dist_px * q.mean() if len(q) else 0.0
    return lines, tol


def synthetic(n, seed=1):
    """n lines: four near-copies each of n / 4 random lines of length 1 to 3 in a box of 100 units, tolerance 0.05"""
    rng = np.random.default_rng(seed)
    m = n // 4
    P = rng.uniform(-50, 50, (m, 3))
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    base = np.hstack([P, P + d * rng.uniform(1, 3, (m, 1))])
    return base[np.arange(n) % m] + rng.uniform(-0.01, 0.01, (n, 6)), np.full(n, 0.05)


def kernel_times(ctx, lines, tol, reps):
    ctx.merge_lines(lines, tol)                               # warm-up: code objects, buffers
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = ctx.merge_lines(lines, tol)
    wall = (time.perf_counter() - t0) * 1e3 / reps
    prof = {k: ctx.profile_get(k) for k in KERNELS}
    ctx.profile_enable(False)
    return {"n": len(lines), "pairs": len(out["pairs"]), "counts": out["counts"].tolist(), "call_ms": wall,
            "kernels": {k: [int(v[0]) // reps, float(v[1]) / reps] for k, v in prof.items()}}


def worker(a):
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    scene = make_scene(*SHAPE, seed=SEED)
    l3d = Line3D("", matchingNeighbors=SHAPE[2])
    load_scene(l3d, scene)
    l3d.prepare()
    variants = ["off", "on"] if a.with_on else ["off"]
    out = {v: [] for v in variants}
    info = {}
    for k in range(a.warmup + a.rounds):
        for v in variants:
            if a.with_on:
                l3d.set_merging(v == "on")
            l3d.match_views()
            t0 = time.perf_counter()
            l3d.finish(False)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                out[v].append(dt)
    if a.with_on:
        for diffusion in (False, True):
            tag = "rdd" if diffusion else "plain"
            l3d.set_merging(False)
            l3d.match_views()
            l3d.finish(diffusion)
            res = l3d.getResult()
            d, n, dup = truth_distance(scene, res)
            info[tag] = {"off": {"lines": len(res), "truth_distance": d, "lines_measured": n, "reported_more_than_once": dup}, "rounds": []}
            if not diffusion:
                lines, tol = lines_and_tol(scene, res, 4.0)
            for rounds in (1, 2, 3, 6):
                l3d.set_merging(True, max_rounds=rounds)
                l3d.match_views()
                l3d.finish(diffusion)
                st = l3d.merging()
                info[tag]["rounds"].append({k: v for k, v in st.items() if not hasattr(v, "shape")})
                if rounds == 3:
                    res = l3d.getResult()
                    d, n, dup = truth_distance(scene, res)
                    info[tag]["on"] = {"lines": len(res), "truth_distance": d, "lines_measured": n, "reported_more_than_once": dup}
        ctx = l3d.context()
        info["search_result"] = kernel_times(ctx, lines, tol, 10)
        info["search_1e5"] = kernel_times(ctx, *synthetic(100000), 5)
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


def search_lines(title, s):
    k = s["kernels"]
    return ["  %s: n = %d, %d pairs, counts (eligible, components, released, groups) %r; the whole call %.3f ms (upload, kernels, download)" % (title, s["n"], s["pairs"], s["counts"], s["call_ms"]),
            "    per call, event brackets (launches, ms): " + "  ".join("%s %d %.3f" % (n[6:], k[n][0], k[n][1]) for n in KERNELS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's build of the library (kept outside the repository's history)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--with-on", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent:
        ap.error("--parent is needed")
    p1 = run_worker(a, os.path.abspath(a.parent), False)
    this = run_worker(a, None, True)
    p2 = run_worker(a, os.path.abspath(a.parent), False)
    lines = ["finish() of config 2 (%d x %d x %d, seed %d), warm-up %d, %d timed rounds per variant, variants alternating; a library per process" % (SHAPE + (SEED, a.warmup, a.rounds)),
             "  parent, run 1, off   %s" % stats(p1["ms"]["off"]), "  this build,    off   %s" % stats(this["ms"]["off"]), "  this build,    on    %s" % stats(this["ms"]["on"]),
             "  parent, run 2, off   %s" % stats(p2["ms"]["off"])]
    a1, a2, b, on = (float(np.median(x)) for x in (p1["ms"]["off"], p2["ms"]["off"], this["ms"]["off"], this["ms"]["on"]))
    info = this["info"]
    lines.append("  merging on (defaults: 4 px, 5 degrees, gap 0, 3 rounds) costs %.3f ms of finish() (medians)" % (on - b))
    for tag in ("plain", "rdd"):
        i = info[tag]
        lines.append("  %s: %d lines without the option; with max_rounds 1, 2, 3, 6: %s" % (tag, i["off"]["lines"], "; ".join(
            "%d lines after %d rounds (%d pairs in the first, %d groups merged, %d released, %d empty refits)"
            % (r["lines_after"], r["rounds"], r["pairs_first_round"], r["groups_merged"], r["lines_released"], r["empty_refits"]) for r in i["rounds"])))
        lines.append("  %s: mean distance of the lines' end points to their ground-truth lines (scene units): off %.6f (%d lines), on %.6f (%d lines); true segments reported "
                     "more than once: off %d, on %d" % (tag, i["off"]["truth_distance"], i["off"]["lines_measured"], i["on"]["truth_distance"], i["on"]["lines_measured"],
                                                       i["off"]["reported_more_than_once"], i["on"]["reported_more_than_once"]))
    lines += search_lines("l3d_merge_lines on the plain result's lines", info["search_result"])
    lines += search_lines("l3d_merge_lines on a synthetic table", info["search_1e5"])
    lines.append("option off: parent %.3f / %.3f (spread %.3f), this build %.3f: %s" % (a1, a2, abs(a1 - a2), b, "not slower" if b - min(a1, a2) <= abs(a1 - a2) else
                                                                                       "SLOWER than the spread of the parent's two runs allows (a miss)"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
