#!/usr/bin/env python3
"""What the remap and its validity plane cost, and that the old paths were left alone: per-image milliseconds of detect_segments_batch at 640x480
and 1920x1080, batches of 1 and 16, with a k1-k2 camera (k_det_undistort) and a plain FISHEYE lens (k_det_undistort_lens) on the parent commit's
build and on this build, and on this build FISHEYE with a remap and border mask (k_det_undistort_remap, k_det_valid_*) against FISHEYE without.
Writes profiles/remap_times.txt.

    python scripts/time_remap.py --parent /path/to/the/parent/commit's/libline3d_amd.so [--out F]
    python scripts/time_remap.py --kernels [--out F]       # appends: the new kernels alone, from the library's event brackets, and segment counts

The procedure of scripts/time_lens.py and time_batch.py: seeded scenes (four per size, cycled), warm-up 5, the variants alternating call by call,
each call ending with the segments on the host; a library is measured in a process of its own (L3D_LIBRARY).  The two builds are compared on the
two OLD paths alone, the processes alternating parent, this, parent, this, parent, this: three runs each.  The run-to-run spread is the largest
minus the smallest of the parent's three medians, and each of this build's three medians must lie within that spread of the parent's range: the
last line of the first part says how that came out.  40 timed rounds per variant: with 12, the medians of the single calls at 1920x1080 (which
scatter between 2.7 and 4.1 ms from call to call on either build) moved by more from run to run than three of them showed as a spread.
A last process times the remap beside the plain FISHEYE lens (same lens, same output camera and size, so that both detect on the same pixels);
its difference is reported, not judged."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIZES = ("640x480", "1920x1080")
BATCHES = (1, 16)
K1, K2 = -0.12, 0.01
FISHEYE = (-0.03, 0.008, -0.002, 0.0004)
OLD = ("k1-k2 camera", "FISHEYE")


def cameras(w, h):
    """the k1-k2 camera / output camera of time_lens.py, and the fisheye's source camera (1.3 x its focal length: the output shows a black rim)"""
    cam = (0.9 * w, 0.9 * w, w / 2.0, h / 2.0)
    return cam, (1.3 * cam[0], 1.3 * cam[1], cam[2], cam[3])


def worker(a):
    """this process's library; prints {size: {"<variant>, batch <b>": [ms per image]}}"""
    from line3d_amd import capi
    from time_undistort import scenes
    ctx = capi.Context(0)
    out = {}
    for size in SIZES:
        imgs = scenes(size, 4)
        h, w = imgs[0].shape[:2]
        cam, src = cameras(w, h)
        fish = capi.lens("fisheye", FISHEYE, camera=src)
        variants = [("k1-k2 camera", dict(cameras=cam + (K1, K2))), ("FISHEYE", dict(cameras=cam, lenses=fish))]
        if a.remap:
            variants = [("FISHEYE", dict(cameras=cam, lenses=fish)), ("FISHEYE, remap + border mask", dict(cameras=cam, lenses=fish, out_sizes=(w, h)))]
        out[size] = {"%s, batch %d" % (name, b): [] for name, _ in variants for b in BATCHES}
        for k in range(a.warmup + a.rounds):
            for b in BATCHES:
                for name, kw in variants:
                    batch = [imgs[(k + j) % len(imgs)] for j in range(b)]
                    t0 = time.perf_counter()
                    ctx.detect_segments_batch(batch, **{key: [val] * b for key, val in kw.items()})
                    if k >= a.warmup:
                        out[size]["%s, batch %d" % (name, b)].append((time.perf_counter() - t0) * 1e3 / b)
    ctx.close()
    print("RESULT " + json.dumps(out))


def kernels(a):
    """the new kernels alone (the library's event brackets, a pass per kernel: 3 calls to warm up, 10 timed), single image and a chunk of 16, at both
    sizes; and the number of segments the scenes give with and without the plane"""
    from line3d_amd import capi
    from time_undistort import scenes
    ctx = capi.Context(0)
    lines = ["the new kernels alone, ms per launch (event brackets; 3 calls to warm up, 10 timed); FISHEYE, remap + border mask, output = source size:"]
    counts = ["segments returned on the script's scenes (4 per size; cap 3000), FISHEYE without and with the plane:"]
    ctx.profile_enable(True)
    for size in SIZES:
        imgs = scenes(size, 4)
        h, w = imgs[0].shape[:2]
        cam, src = cameras(w, h)
        fish = capi.lens("fisheye", FISHEYE, camera=src)
        batch = [imgs[j % len(imgs)] for j in range(16)]
        calls = (("single", lambda: ctx.detect_segments(imgs[0], camera=cam, lens=fish, out_size=(w, h))),
                 ("chunk of 16", lambda: ctx.detect_segments_batch(batch, cameras=[cam] * 16, lenses=[fish] * 16, out_sizes=[(w, h)] * 16)))
        for kern in ("k_det_undistort_remap", "k_det_valid_x", "k_det_valid_y", "k_det_valid_apply", "k_det_undistort_lens"):
            for what, call in calls:
                if kern == "k_det_undistort_lens":          # the old kernel on the same images, for scale
                    call = (lambda: ctx.detect_segments(imgs[0], camera=cam, lens=fish)) if what == "single" else (lambda: ctx.detect_segments_batch(batch, cameras=[cam] * 16, lenses=[fish] * 16))
                ctx.profile_only(kern)
                for _ in range(3):
                    call()
                ctx.profile_reset()
                for _ in range(10):
                    call()
                n, ms = ctx.profile_get(kern)
                lines.append("  %-10s %-12s %-24s %2d launches, %.4f ms per launch" % (size, what, kern, n, ms / max(1, n)))
        # the two kernels the calls above never reach, and the resampling onto another size: a call that rescales (k_det_valid_grey), a call with a
        # mask and no lens (k_det_valid_from_mask), and the planner's view at alpha 1 that keeps the focal length, scaled down to the source's width
        mask = np.ones((h, w), np.uint8)
        mask[h // 3:h // 2, w // 4:w // 2] = 0
        K2, wh = capi.undistort_plan(fish, (w, h), 1.0, "keep_focal", max_dim=w)
        cam2 = (K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2])
        nw = (3 * w // 4, 3 * h // 4)
        extra = (("k_det_valid_grey", "rescaled to %dx%d" % nw, lambda: ctx.detect_segments(imgs[0], new_size=nw, camera=cam, lens=fish, out_size=(w, h)),
                  lambda: ctx.detect_segments_batch(batch, new_sizes=[nw] * 16, cameras=[cam] * 16, lenses=[fish] * 16, out_sizes=[(w, h)] * 16)),
                 ("k_det_valid_from_mask", "a mask, no lens", lambda: ctx.detect_segments(imgs[0], mask=mask), lambda: ctx.detect_segments_batch(batch, masks=[mask] * 16)),
                 ("k_det_undistort_remap", "onto %dx%d, alpha 1" % wh, lambda: ctx.detect_segments(imgs[0], camera=cam2, lens=fish, out_size=wh),
                  lambda: ctx.detect_segments_batch(batch, cameras=[cam2] * 16, lenses=[fish] * 16, out_sizes=[wh] * 16)))
        for kern, note, single, chunk in extra:
            for what, call in (("single", single), ("chunk of 16", chunk)):
                ctx.profile_only(kern)
                for _ in range(3):
                    call()
                ctx.profile_reset()
                for _ in range(10):
                    call()
                n, ms = ctx.profile_get(kern)
                lines.append("  %-10s %-12s %-24s %2d launches, %.4f ms per launch   (%s)" % (size, what, kern, n, ms / max(1, n), note))
        ctx.profile_only("")
        plain = [len(ctx.detect_segments(im, camera=cam, lens=fish)) for im in imgs]
        plane = [len(ctx.detect_segments(im, camera=cam, lens=fish, out_size=(w, h))) for im in imgs]
        counts.append("  %-10s without %s, with %s" % (size, plain, plane))
    ctx.close()
    text = "\n".join(lines + counts) + "\n"
    print(text, end="")
    with open(a.out, "a") as f:
        f.write(text)


def run_worker(a, library, remap):
    env = dict(os.environ)
    if library:
        env["L3D_LIBRARY"] = library
    else:
        env.pop("L3D_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(a.warmup), "--rounds", str(a.rounds)] + (["--remap"] if remap else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def stats(ms):
    ms = np.array(ms)
    return "median %7.3f ms   p10 %7.3f  p90 %7.3f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's build of the library (kept outside the repository's history)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--remap", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.kernels:
        return kernels(a)
    if not a.parent:
        ap.error("--parent is needed")
    # (the parent's worker runs from this tree with the parent's library: the two old variants use nothing the parent's library lacks)
    parent = os.path.abspath(a.parent)
    runs = []
    for r in (1, 2, 3):
        runs.append(("parent, run %d" % r, run_worker(a, parent, False)))
        runs.append(("this, run %d" % r, run_worker(a, None, False)))
    runs.append(("this, remap", run_worker(a, None, True)))
    lines = ["detect_segments_batch with an undistortion in front, ms per image, warm-up %d, %d timed rounds per variant, variants alternating; a library per process"
             % (a.warmup, a.rounds),
             "k1-k2 camera: k1 = %g, k2 = %g; FISHEYE: %s, source focal length 1.3 x the output's; f = 0.9 width; remap: the same lens, camera and size, border mask on" % (K1, K2, FISHEYE)]
    ok = True
    outside = {1: 0, 2: 0, 3: 0}
    for size in SIZES:
        lines.append(size)
        med = {}
        for name, res in runs:
            for variant, ms in res[size].items():
                med[(name, variant)] = float(np.median(ms))
                lines.append("  %-14s %-40s %s" % (name, variant, stats(ms)))
        for b in BATCHES:
            for old in OLD:
                v = "%s, batch %d" % (old, b)
                ps = [med[("parent, run %d" % r, v)] for r in (1, 2, 3)]
                ts = [med[("this, run %d" % r, v)] for r in (1, 2, 3)]
                spread = max(ps) - min(ps)
                fine = all(min(ps) - spread <= t <= max(ps) + spread for t in ts)
                ok = ok and fine
                for r, t in zip((1, 2, 3), ts):
                    outside[r] += not (min(ps) - spread <= t <= max(ps) + spread)
                calls = np.concatenate([res[size][v] for name, res in runs if name.startswith("parent")])
                lines.append("  %s: parent %.3f / %.3f / %.3f (run-to-run spread %.3f; its single calls: p10 %.3f, p90 %.3f), this build %.3f / %.3f / %.3f: %s"
                             % (v, ps[0], ps[1], ps[2], spread, np.percentile(calls, 10), np.percentile(calls, 90), ts[0], ts[1], ts[2],
                                "agrees" if fine else "DIFFERS by more than the spread"))
            d = med[("this, remap", "FISHEYE, remap + border mask, batch %d" % b)] - med[("this, remap", "FISHEYE, batch %d" % b)]
            lines.append("  FISHEYE with remap and border mask, batch %d: %+.3f ms per image against FISHEYE without, in the same process" % (b, d))
    # where a cell differs: is it the code (every run of this build off, in that cell) or a process (one run off, in many cells)?
    for r in (1, 2, 3):
        lines.append("this build, run %d: %d of %d cells outside the parent's range by more than its spread" % (r, outside[r], len(SIZES) * len(BATCHES) * len(OLD)))
    lines.append("the old paths (k1-k2 camera, plain FISHEYE lens) on this build agree with the parent's build within the run-to-run spread at every size and batch: %s"
                 % ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
