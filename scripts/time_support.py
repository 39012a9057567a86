#!/usr/bin/env python3
"""What the support of 3-D lines costs and what it finds: finish() of config 2 (64 x 2000 x 12, seed 20260) with the option off and on against the parent
commit, l3d_support_lines alone with its kernels' times from event brackets on the plain result's own lines (every view's 2000 segments) and on a
synthetic input of 10^5 3-D segments x 64 cameras x 2000 segments, the pair tests per second of both, the share of lanes the projection leaves without a
row, and what the gather reports on the result.  Writes profiles/support_times.txt.

    python scripts/time_support.py --parent /path/to/the/parent/commit's/libline3d_amd.so [--out F]

The procedure of scripts/time_merge.py: a library is measured in a process of its own (L3D_LIBRARY), warm-up rounds first, the variants of a process
alternating round by round; a round is prepare-once, then matchViews + finish() with only finish() timed.  (a) the parent commit's build, option off (it
has no other), run twice -- before and after; (b) this build with the option never touched, measured as the parent is; (c) this build, off and on
alternating.  Off (b) may not be slower than the parent by more than the parent's two runs differ; the last line of the file says how that came out.  For
the option on no time is claimed: the file records what came out."""
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
KERNELS = ("sup_prepare", "sup_count", "sup_scan", "sup_write", "sup_best")


def synthetic(n, m, per_camera, seed=1):
    """n 3-D segments of length 0.5 to 2 in a box of 20 units, m cameras on a circle of radius 40 around it looking at its centre (1920 x 1080, f 1600),
    and per camera `per_camera` 2-D segments: stretches of the projections of random 3-D segments, half a pixel of noise"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-10, 10, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    seg3d = np.hstack([P, P + d * rng.uniform(0.5, 2.0, (n, 1))])
    K = np.array([[1600.0, 0.0, 960.0], [0.0, 1600.0, 540.0], [0.0, 0.0, 1.0]])
    cams, segs = [], []
    for c in range(m):
        a = 2.0 * np.pi * c / m
        C = np.array([40.0 * np.cos(a), 40.0 * np.sin(a), 5.0])
        z = -C / np.linalg.norm(C)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        t = -R @ C
        cams.append((K, R, t, 1920, 1080))
        pick = rng.integers(0, n, per_camera)
        lo = rng.uniform(0.0, 0.4, (per_camera, 1))
        hi = lo + rng.uniform(0.5, 0.6, (per_camera, 1))
        ends = []
        for f in (lo, hi):
            X = seg3d[pick, :3] + f * (seg3d[pick, 3:] - seg3d[pick, :3])
            x3 = X @ R.T + t
            ends.append((x3[:, :2] / x3[:, 2:]) * 1600.0 + [960.0, 540.0])
        segs.append((np.hstack(ends) + rng.normal(0.0, 0.5, (per_camera, 4))).astype(np.float32))
    return seg3d, cams, segs


def kernel_times(ctx, seg3d, cams, segs, reps):
    from line3d_amd import capi
    arr = capi.cameras(cams)
    ctx.support_lines(seg3d, arr, segs)                       # warm-up: code objects, buffers
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = ctx.support_lines(seg3d, arr, segs)
    wall = (time.perf_counter() - t0) * 1e3 / reps
    prof = {k: ctx.profile_get(k) for k in KERNELS}
    ctx.profile_enable(False)
    tests = float(sum(len(s) for s in segs)) * len(seg3d)
    return {"n": len(seg3d), "m": len(cams), "columns": int(sum(len(s) for s in segs)), "counts": out["counts"].tolist(), "call_ms": wall, "pair_tests": tests,
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
                l3d.set_support(v == "on")
            l3d.match_views()
            t0 = time.perf_counter()
            l3d.finish(False)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                out[v].append(dt)
    if a.with_on:
        views = sorted(scene.views, key=lambda v: int(v["id"]))
        gt = {int(v["id"]): v["gt"] for v in views}
        for tag, merge in (("plain", False), ("merged", True)):
            l3d.set_support(False)
            l3d.set_merging(merge)
            l3d.match_views()
            l3d.finish(False)
            res = l3d.getResult()
            g = l3d.gather_support()
            rec, start = g["records"], g["line_start"]
            right = 0
            for li, (s2, _) in enumerate(res):
                major = int(np.bincount([int(gt[c][s]) for c, s in s2]).argmax())
                r = rec[start[li]:start[li + 1]]
                right += sum(1 for c, s in zip(r["view_id"].tolist(), r["seg"].tolist()) if int(gt[c][s]) == major)
            l3d.set_support(True)
            l3d.match_views()
            l3d.finish(False)
            st = l3d.support()
            info[tag] = {"lines": len(res), "counts": g["counts"].tolist(), "with_gt_id": right, "member_views_median": float(np.median(g["line_views"][:, 0])),
                         "record_views_median": float(np.median(g["line_views"][:, 1])), "record_views_min": int(g["line_views"][:, 1].min()),
                         "members_before": int(st["members_before"].sum()), "members_added": int(st["members_added"].sum()),
                         "views_before_median": float(np.median(st["views_before"])), "views_after_median": float(np.median(st["views_after"]))}
            if not merge:
                seg3d = np.array([np.concatenate([p, q]) for _, s3 in res for p, q in s3])
        l3d.set_merging(False)
        l3d.set_support(False)
        ctx = l3d.context()
        cams = [(v["K"], v["R"], v["t"], int(v["width"]), int(v["height"])) for v in views]
        info["search_result"] = kernel_times(ctx, seg3d, cams, [v["segments"] for v in views], 10)
        info["search_1e5"] = kernel_times(ctx, *synthetic(100000, 64, 2000), 3)
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
    search_ms = k["sup_count"][1] + k["sup_write"][1]
    rows, lanes = s["counts"][0], s["n"] * s["m"]
    return ["  %s: %d 3-D segments x %d cameras, %d 2-D segments: %.3g pair tests a pass; counts (rows, eligible columns, records, columns with a best row) %r; the whole call %.3f ms "
            "(upload, kernels, download)" % (title, s["n"], s["m"], s["columns"], s["pair_tests"], s["counts"], s["call_ms"]),
            "    per call, event brackets (launches, ms): " + "  ".join("%s %d %.3f" % (n[4:], k[n][0], k[n][1]) for n in KERNELS),
            "    count and write run the pair tests once each: %.3g pair tests per second over the two (the merge search: 4.4e11); lanes without a row (the projection "
            "drops the pair): %d of %d, %.1f %%" % (2.0 * s["pair_tests"] / (search_ms * 1e-3) if search_ms > 0 else 0.0, lanes - rows, lanes, 100.0 * (lanes - rows) / lanes)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's build of the library (kept outside the repository's history)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--with-on", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "support_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent:
        ap.error("--parent is needed")
    p1 = run_worker(a, os.path.abspath(a.parent), False)
    alone = run_worker(a, None, False)                      # this build as the parent is measured: a process that never turns the option on
    this = run_worker(a, None, True)
    p2 = run_worker(a, os.path.abspath(a.parent), False)
    lines = ["finish() of config 2 (%d x %d x %d, seed %d), warm-up %d, %d timed rounds per variant, variants alternating; a library per process" % (SHAPE + (SEED, a.warmup, a.rounds)),
             "  parent, run 1, off   %s" % stats(p1["ms"]["off"]), "  this build,    off   %s   (a process of its own, as the parent's)" % stats(alone["ms"]["off"]),
             "  this build,    off   %s   (alternating with on)" % stats(this["ms"]["off"]), "  this build,    on    %s" % stats(this["ms"]["on"]),
             "  parent, run 2, off   %s" % stats(p2["ms"]["off"])]
    a1, a2, b, on = (float(np.median(x)) for x in (p1["ms"]["off"], p2["ms"]["off"], alone["ms"]["off"], this["ms"]["on"]))
    b_alt = float(np.median(this["ms"]["off"]))
    info = this["info"]
    lines.append("  support on (defaults: 3 px, 5 degrees, overlap 0.5) costs %.3f ms of finish() (medians of the alternating process)" % (on - b_alt))
    for tag in ("plain", "merged"):
        i = info[tag]
        c = i["counts"]
        lines.append("  %s result (%s): %d lines; views with a member, median per line %g; views with a supporting segment, median / min per line %g / %d; %d records, %d with the "
                     "line's ground-truth id (%.2f %%); members found again %d of %d; segments on a line and members of none %d"
                     % (tag, "merging off" if tag == "plain" else "merging on, defaults", i["lines"], i["member_views_median"], i["record_views_median"], i["record_views_min"], c[0],
                        i["with_gt_id"], 100.0 * i["with_gt_id"] / max(1, c[0]), c[1], c[1] + c[2], c[3]))
        lines.append("  %s result, option on: %d members before, %d added; views with a member, median per line %g before, %g after"
                     % (tag, i["members_before"], i["members_added"], i["views_before_median"], i["views_after_median"]))
    lines += search_lines("l3d_support_lines on the plain result's 3-D segments", info["search_result"])
    lines += search_lines("l3d_support_lines on a synthetic input", info["search_1e5"])
    lines.append("option off: parent %.3f / %.3f (spread %.3f), this build %.3f: %s" % (a1, a2, abs(a1 - a2), b, "not slower" if b - min(a1, a2) <= abs(a1 - a2) else
                                                                                       "SLOWER than the spread of the parent's two runs allows (a miss)"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
