#!/usr/bin/env python3
"""What filing the world point links costs (include/line3d_amd.h, "CO-VISIBILITY"): the host bookkeeping (Line3D::processWorldpointList through
l3d_test_covisibility_host: the product's function, list after list) against l3d_covisibility on the device, end to end (upload, sort, kernels,
download), and the kernels alone.  Writes profiles/covisibility_times.txt.

    python scripts/time_covisibility.py [--rounds N] [--out F] [--shapes 256x8000,2048x8000]

Synthetic tracks, seed 7: every point has a centre view and is seen, with probability 1/2, by each view within +-6 of it (the centre included); the
number of points is chosen so that a view lists about `observations per view` of them; every list is shuffled.  Per shape, in one process: the host
replay once (it takes seconds), the device call after warm-up rounds by the host's clock (the call ends in a stream synchronise) with the profile
brackets off, then rounds of their own with the kernels bracketed by events.  The device result is compared with the host replay's before anything
is timed."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 7
KERNELS = ("covis_keys", "covis_sort", "covis_runs", "covis_count", "covis_scan", "covis_write")


def make_lists(n_views, per_view, half_width=6, seed=SEED):
    rng = np.random.default_rng(seed)
    n_points = int(round(n_views * per_view / (0.5 * (2 * half_width + 1))))
    ids = rng.choice(1 << 31, n_points, replace=False).astype(np.uint32)
    centre = rng.integers(0, n_views, n_points)
    views, points = [], []
    for d in range(-half_width, half_width + 1):
        v = centre + d
        keep = (v >= 0) & (v < n_views) & (rng.random(n_points) < 0.5)
        views.append(v[keep])
        points.append(ids[keep])
    views, points = np.concatenate(views), np.concatenate(points)
    order = rng.permutation(len(views))
    views, points = views[order], points[order]
    order = np.argsort(views, kind="stable")
    views, points = views[order], points[order]
    start = np.zeros(n_views + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(views, minlength=n_views))
    return np.ascontiguousarray(points), start


def stats(ms):
    ms = np.array(ms)
    return "median %9.3f ms   min %9.3f  max %9.3f" % (np.median(ms), ms.min(), ms.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--shapes", default="256x8000,2048x8000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covisibility_times.txt"))
    a = ap.parse_args()
    from line3d_amd import capi
    lib = capi.load_library()
    ctx = capi.Context(0)
    lines = ["co-visibility counting: synthetic tracks, seed %d, every point seen with probability 1/2 by each view within +-6 of its centre view" % SEED,
             "warm-up %d, %d timed rounds of the device call; the host replay once; the device result equals the host replay's, integer for integer" % (a.warmup, a.rounds)]
    for shape in a.shapes.split(","):
        V, per_view = (int(x) for x in shape.split("x"))
        ids, start = make_lists(V, per_view)

        def device():
            rc, out = capi._covisibility_call(lib.l3d_covisibility, (ctx.h,), capi._p(ids), capi._p(start), V)
            ctx._chk(rc)
            return out

        t0 = time.perf_counter()
        rc, host = capi._covisibility_call(lib.l3d_test_covisibility_host, (), capi._p(ids), capi._p(start), V)
        t_host = time.perf_counter() - t0
        if rc != 0:
            raise SystemExit("the host replay failed (%d)" % rc)
        got = device()
        if got[4] != 0 or not all(np.array_equal(x, y) for x, y in zip(got[:4], host[:4])):
            raise SystemExit("%s: the device call differs from the host replay" % shape)
        call = []
        for k in range(a.warmup + a.rounds):
            t0 = time.perf_counter()
            device()
            if k >= a.warmup:
                call.append((time.perf_counter() - t0) * 1e3)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for k in range(a.rounds):
            device()
        kern = {k: ctx.profile_get(k) for k in KERNELS}
        ctx.profile_enable(False)
        lines.append("%d views x %d observations per view (%d observations, %d non-zero counts):" % (V, per_view, len(ids), len(host[2])))
        lines.append("  host replay (l3d_test_covisibility_host, once)        %9.3f ms" % (t_host * 1e3))
        lines.append("  l3d_covisibility end to end (host clock)              %s" % stats(call))
        lines.append("  host replay / device median                           %9.1f" % (t_host * 1e3 / np.median(call)))
        lines.append("  the kernels alone (event brackets, mean of %d launches each): " % a.rounds + "   ".join("%s %.3f ms" % (k, kern[k][1] / max(1, kern[k][0])) for k in KERNELS))
        lines.append("  sum of the kernels                                    %9.3f ms" % sum(kern[k][1] / max(1, kern[k][0]) for k in KERNELS))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
