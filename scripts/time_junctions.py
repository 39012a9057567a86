#!/usr/bin/env python3
"""What the junctions of 3-D lines cost: finish() of config 2 (64 x 2000 x 12, seed 20260) with the option off and on, alternating round by round in one
process, and the kernels of l3d_junction_lines on the result's own lines and on a synthetic table of 65536 lines (corners of three edges each).  Writes
profiles/junction_times.txt.

    python scripts/time_junctions.py [--parent /path/to/the/parent/commit's/libline3d_amd.so] [--out F]

The procedure of scripts/time_merge.py: a library is measured in a process of its own (L3D_LIBRARY), warm-up rounds first; a round is prepare-once, then
matchViews + finish() with only finish() timed.  With --parent the parent commit's build (option off: it has no other) runs before and after this build.
No time is claimed for the option on: the file records what came out.  Pair tests per second: n (n - 1) / 2 tests in each of the count and the write
pass, over the sum of the two kernels' times."""
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
KERNELS = ("junc_prepare", "junc_count", "junc_scan", "junc_write", "junc_cc_hook", "junc_cc_compress", "junc_rep", "junc_star", "junc_flag", "junc_vscan", "junc_keys",
           "junc_sort", "junc_vertex", "junc_attach", "junc_finish")


def table_of(scene, result, dist_px=4.0, ext_px=12.0, max_ext_rel=0.25):
    """the table the pipeline hands to l3d_junction_lines: P, Q, dist_px x sigma, min(ext_px x sigma, max_ext_rel x L) (vectorised: not bit-exact)"""
    R2 = np.array([v["R"][2] for v in scene.views])
    t2 = np.array([v["t"][2] for v in scene.views])
    f = np.array([(abs(v["K"][0, 0]) + abs(v["K"][1, 1])) / 2.0 for v in scene.views])
    index = {v["id"]: i for i, v in enumerate(scene.views)}
    lines = np.array([np.concatenate([s3[0][0], s3[-1][1]]) for _, s3 in result])
    sigma = np.zeros(len(lines))
    for k, (s2, _) in enumerate(result):
        cams = np.array([index[c] for c, _ in s2])
        q = (R2[cams] @ ((lines[k, :3] + lines[k, 3:]) / 2.0) + t2[cams]) / f[cams]
        q = q[q > 0]
        sigma[k] = q.mean() if len(q) else 0.0
    L = np.linalg.norm(lines[:, 3:] - lines[:, :3], axis=1)
    return lines, dist_px * sigma, np.minimum(ext_px * sigma, max_ext_rel * L)


def synthetic(n, seed=1):
    """n lines: the three edges of n // 3 corners with random frames in a box of 100 units, ends up to 0.05 short of the corner; tol 0.05, ext 0.1"""
    rng = np.random.default_rng(seed)
    m = max(1, n // 3)
    c = rng.uniform(-50, 50, (m, 3))
    frames = np.linalg.qr(rng.normal(size=(m, 3, 3)))[0]
    k = np.arange(n)
    a = frames[k % m, :, (k // m) % 3]
    P = c[k % m] + a * rng.uniform(-0.02, 0.05, (n, 1)) + rng.uniform(-0.005, 0.005, (n, 3))
    return np.hstack([P, P + a * rng.uniform(1, 3, (n, 1))]), np.full(n, 0.05), np.full(n, 0.1)


def kernel_times(ctx, lines, tol, ext, reps):
    ctx.junction_lines(lines, tol, ext)                       # warm-up: code objects, buffers
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = ctx.junction_lines(lines, tol, ext)
    wall = (time.perf_counter() - t0) * 1e3 / reps
    prof = {k: ctx.profile_get(k) for k in KERNELS}
    ctx.profile_enable(False)
    return {"n": len(lines), "records": len(out["records"]), "counts": out["counts"].tolist(), "call_ms": wall,
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
                l3d.set_junctions(v == "on")
            l3d.match_views()
            t0 = time.perf_counter()
            l3d.finish(False)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                out[v].append(dt)
    if a.with_on:
        l3d.set_junctions(True)
        l3d.match_views()
        l3d.finish(False)
        j = l3d.junctions()
        info["object"] = {k: v for k, v in j.items() if not hasattr(v, "shape")}
        ctx = l3d.context()
        info["search_result"] = kernel_times(ctx, *table_of(scene, l3d.getResult()), 10)
        info["search_65536"] = kernel_times(ctx, *synthetic(65536), 5)
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
    pairs = s["n"] * (s["n"] - 1) / 2.0
    both = (k["junc_count"][1] + k["junc_write"][1]) * 1e-3
    return ["  %s: n = %d, %d records, counts (eligible, L, T, X, components, vertices, released, attached) %r; the whole call %.3f ms (upload, kernels, download)"
            % (title, s["n"], s["records"], s["counts"], s["call_ms"]),
            "    per call, event brackets (launches, ms): " + "  ".join("%s %d %.3f" % (n[5:], k[n][0], k[n][1]) for n in KERNELS),
            "    %.3g pair tests a pass; %.3g pair tests per second over count + write" % (pairs, 2.0 * pairs / both if both > 0 else float("nan"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's build of the library (kept outside the repository's history)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--with-on", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "junction_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    p1 = run_worker(a, os.path.abspath(a.parent), False) if a.parent else None
    this = run_worker(a, None, True)
    p2 = run_worker(a, os.path.abspath(a.parent), False) if a.parent else None
    lines = ["finish() of config 2 (%d x %d x %d, seed %d), warm-up %d, %d timed rounds per variant, variants alternating; a library per process" % (SHAPE + (SEED, a.warmup, a.rounds))]
    if p1:
        lines.append("  parent, run 1, off   %s" % stats(p1["ms"]["off"]))
    lines += ["  this build,    off   %s" % stats(this["ms"]["off"]), "  this build,    on    %s" % stats(this["ms"]["on"])]
    if p2:
        lines.append("  parent, run 2, off   %s" % stats(p2["ms"]["off"]))
    b, on = float(np.median(this["ms"]["off"])), float(np.median(this["ms"]["on"]))
    info = this["info"]
    lines.append("  junctions on (defaults: 4 px, 12 px, 10 degrees, 0.25, no snap) cost %.3f ms of finish() (medians); what they found: %s" % (on - b, json.dumps(info["object"])))
    lines += search_lines("l3d_junction_lines on the result's lines", info["search_result"])
    lines += search_lines("l3d_junction_lines on a synthetic table", info["search_65536"])
    if p1 and p2:
        a1, a2 = float(np.median(p1["ms"]["off"])), float(np.median(p2["ms"]["off"]))
        lines.append("option off: parent %.3f / %.3f (spread %.3f), this build %.3f: %s" % (a1, a2, abs(a1 - a2), b, "not slower" if b - min(a1, a2) <= abs(a1 - a2) else
                                                                                           "SLOWER than the spread of the parent's two runs allows (a miss)"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
