#!/usr/bin/env python3
"""What the lens costs, and that the k1-k2 path was left alone: per-image milliseconds of detect_segments_batch at 640x480 and 1920x1080, batches of
1 and 16, with a k1-k2 camera (k_det_undistort) on the parent commit's build and on this build, and on this build with a BROWN lens of all eight
coefficients and with a FISHEYE lens (k_det_undistort_lens).  Writes profiles/lens_times.txt.

    python scripts/time_lens.py --parent /path/to/the/parent/commit's/libline3d_amd.so [--out F]
    python scripts/time_lens.py --kernels [--out F]        # appends: the two undistortion kernels alone, from the library's event brackets

The procedure of scripts/time_batch.py: its seeded scenes (four per size, cycled), warm-up 5, the variants alternating call by call so that all see the
same machine, each call ending with the segments on the host; a library is measured in a process of its own (L3D_LIBRARY).
The comparison of the two builds: the k1-k2 camera ALONE, by the same procedure on both (a variant timed between calls of other variants starts on
other host caches -- time_batch.py met the same), the processes alternating parent, this, parent, this, parent.  The run-to-run spread this script
reports is the largest minus the smallest of the parent's three medians -- what the same code on the same machine gives from one run to the next --
and each of this build's two medians must lie within that spread of the parent's range: the last line of the file says how that came out.
(Two runs of the parent, the first form of this script, gave a spread that was now and then 0.000 ms at three decimals: too few runs to call
it a spread.)  A last process times the lens variants beside the k1-k2 camera; they are reported, not judged."""
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
BROWN8 = (-0.12, 0.01, 0.002, -0.0015, 0.004, 0.01, -0.006, 0.002)
FISHEYE = (-0.03, 0.008, -0.002, 0.0004)


def worker(a):
    """this process's library; prints {size: {"<variant>, batch <b>": [ms per image]}}"""
    from line3d_amd import capi
    from time_undistort import scenes
    ctx = capi.Context(0)
    out = {}
    for size in SIZES:
        imgs = scenes(size, 4)
        h, w = imgs[0].shape[:2]
        cam = (0.9 * w, 0.9 * w, w / 2.0, h / 2.0)
        variants = [("k1-k2 camera", dict(cameras=cam + (K1, K2)))]
        if a.lenses:
            variants += [("BROWN, 8 coefficients", dict(cameras=cam, lenses=capi.lens("brown", BROWN8))),
                         ("FISHEYE", dict(cameras=cam, lenses=capi.lens("fisheye", FISHEYE, camera=(1.3 * cam[0], 1.3 * cam[1], cam[2], cam[3]))))]
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
    """k_det_undistort and k_det_undistort_lens alone at 1920x1080x3 (the library's event brackets, a pass of its own: 3 calls to warm up, 10 timed):
    single undistort calls and the one launch of a 16-image chunk.  What a lens costs in the whole detector call beyond this is the detector's work on
    another image: the resampled image shows another part of the scene, with a black border where the source has no pixels"""
    from line3d_amd import capi
    from time_undistort import scenes
    ctx = capi.Context(0)
    imgs = scenes("1920x1080", 4)
    h, w = imgs[0].shape[:2]
    cam = (0.9 * w, 0.9 * w, w / 2.0, h / 2.0)
    K = np.array([[cam[0], 0.0, cam[2]], [0.0, cam[1], cam[3]], [0.0, 0.0, 1.0]])
    brown = capi.lens("brown", BROWN8)
    fish = capi.lens("fisheye", FISHEYE, camera=(1.3 * cam[0], 1.3 * cam[1], cam[2], cam[3]))
    batch = [imgs[j % len(imgs)] for j in range(16)]
    ctx.profile_enable(True)
    lines = ["the undistortion kernels alone, 1920x1080x3, ms per launch (event brackets; 3 calls to warm up, 10 timed):"]
    for name, kern, call in (("k1-k2 camera, single undistort", "k_det_undistort", lambda: ctx.undistort(imgs[0], K, K1, K2)),
                             ("BROWN, 8 coefficients, single undistort", "k_det_undistort_lens", lambda: ctx.undistort(imgs[0], K, lens=brown)),
                             ("FISHEYE, single undistort", "k_det_undistort_lens", lambda: ctx.undistort(imgs[0], K, lens=fish)),
                             ("k1-k2 camera, chunk of 16", "k_det_undistort", lambda: ctx.detect_segments_batch(batch, cameras=[cam + (K1, K2)] * 16)),
                             ("BROWN, 8 coefficients, chunk of 16", "k_det_undistort_lens", lambda: ctx.detect_segments_batch(batch, cameras=[cam] * 16, lenses=[brown] * 16)),
                             ("FISHEYE, chunk of 16", "k_det_undistort_lens", lambda: ctx.detect_segments_batch(batch, cameras=[cam] * 16, lenses=[fish] * 16))):
        ctx.profile_only(kern)
        for _ in range(3):
            call()
        ctx.profile_reset()
        for _ in range(10):
            call()
        n, ms = ctx.profile_get(kern)
        lines.append("  %-42s %-22s %2d launches, %.4f ms per launch" % (name, kern, n, ms / max(1, n)))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "a") as f:
        f.write(text)


def run_worker(a, library, lenses):
    env = dict(os.environ)
    if library:
        env["L3D_LIBRARY"] = library
    else:
        env.pop("L3D_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(a.warmup), "--rounds", str(a.rounds)] + (["--lenses"] if lenses else [])
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
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lenses", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.kernels:
        return kernels(a)
    if not a.parent:
        ap.error("--parent is needed")
    # (the parent's Python layer has no lenses: its worker runs from this tree with the parent's library, the k1-k2 variant only)
    parent = os.path.abspath(a.parent)
    runs = [("parent, run 1", run_worker(a, parent, False)), ("this, run 1", run_worker(a, None, False)), ("parent, run 2", run_worker(a, parent, False)),
            ("this, run 2", run_worker(a, None, False)), ("parent, run 3", run_worker(a, parent, False)), ("this, lenses", run_worker(a, None, True))]
    lines = ["detect_segments_batch with an undistortion in front, ms per image, warm-up %d, %d timed rounds per variant, variants alternating; a library per process"
             % (a.warmup, a.rounds),
             "k1-k2 camera: k1 = %g, k2 = %g; BROWN: %s; FISHEYE: %s, source focal length 1.3 x the output's; f = 0.9 width" % (K1, K2, BROWN8, FISHEYE)]
    ok = True
    for size in SIZES:
        lines.append(size)
        med = {}
        for name, res in runs:
            for variant, ms in res[size].items():
                med[(name, variant)] = float(np.median(ms))
                lines.append("  %-14s %-32s %s" % (name, variant, stats(ms)))
        for b in BATCHES:
            v = "k1-k2 camera, batch %d" % b
            ps = [med[("parent, run %d" % r, v)] for r in (1, 2, 3)]
            ts = [med[("this, run %d" % r, v)] for r in (1, 2)]
            spread = max(ps) - min(ps)
            fine = all(min(ps) - spread <= t <= max(ps) + spread for t in ts)
            ok = ok and fine
            lines.append("  %s: parent %.3f / %.3f / %.3f (run-to-run spread %.3f), this build %.3f / %.3f: %s"
                         % (v, ps[0], ps[1], ps[2], spread, ts[0], ts[1], "agrees" if fine else "DIFFERS by more than the spread"))
            t = med[("this, lenses", v)]
            for lens in ("BROWN, 8 coefficients", "FISHEYE"):
                lines.append("  %s, batch %d: %+.3f ms per image against the k1-k2 camera in the same process" % (lens, b, med[("this, lenses", "%s, batch %d" % (lens, b))] - t))
    lines.append("the k1-k2 camera on this build agrees with the parent's build within the run-to-run spread at every size and batch: %s" % ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
