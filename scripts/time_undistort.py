#!/usr/bin/env python3
"""Milliseconds per 3-channel image of l3d_detect_segments with and without the undistortion in front (camera=...), at 640x480 and 1920x1080,
and k_det_undistort's own time from the library's event brackets (ProfScope).  Writes profiles/undistort_times.txt.

    python scripts/time_undistort.py                       # both parts
    python scripts/time_undistort.py --plain-only --out F  # detect_segments without a camera only (to compare two builds: L3D_LIBRARY)

The scenes are those of scripts/time_detect.py (filled rotated rectangles, noise sigma 2) in three channels.  Each timed call ends with the
segments on the host, so the window holds the upload, every kernel and the download.  Warm-up first; the two variants alternate image by image, so
both see the same machine; median and p10 / p90 of the timed images are reported.  The kernel's time comes from a pass of its own with the
brackets on (they synchronise nothing, but they are not free), never from the timed pass."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SIZES = {"640x480": (640, 480, 20), "1920x1080": (1920, 1080, 20)}
K1, K2 = -0.12, 0.01


def scenes(size, count, seed=99):
    from make_golden_detect import noisy, render_rects
    w, h, n = SIZES[size]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        g = noisy(render_rects(rng, w, h, n), rng, 2)
        out.append(np.ascontiguousarray(np.stack([g, g, g], axis=-1)))
    return out


def camera(size):
    w, h, _ = SIZES[size]
    f = 0.9 * w
    return (f, f, w / 2.0, h / 2.0, K1, K2)


def stats(ms):
    ms = np.array(ms)
    return "median %7.2f ms   p10 %7.2f  p90 %7.2f   min %7.2f  max %7.2f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90), ms.min(), ms.max())


def time_size(ctx, size, warmup, images, plain_only):
    imgs = scenes(size, 4)
    cam = camera(size)
    variants = [("plain", None)] if plain_only else [("plain", None), ("camera", cam)]
    for k in range(warmup):
        for _, c in variants:
            ctx.detect_segments(imgs[k % len(imgs)], camera=c) if c else ctx.detect_segments(imgs[k % len(imgs)])
    ms = {name: [] for name, _ in variants}
    for k in range(images):
        for name, c in variants:
            img = imgs[k % len(imgs)]
            t0 = time.perf_counter()
            ctx.detect_segments(img, camera=c) if c else ctx.detect_segments(img)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def kernel_time(ctx, size, images):
    imgs = scenes(size, 4)
    cam = camera(size)
    ctx.profile_enable(True)
    ctx.profile_only("k_det_undistort")
    ctx.detect_segments(imgs[0], camera=cam)
    ctx.profile_reset()
    for k in range(images):
        ctx.detect_segments(imgs[k % len(imgs)], camera=cam)
    n, total = ctx.profile_get("k_det_undistort")
    ctx.profile_only(None)
    ctx.profile_enable(False)
    return n, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_times.txt"))
    a = ap.parse_args()
    from line3d_amd import capi
    ctx = capi.Context(0)
    lines = ["l3d_detect_segments on 3-channel images, ms per image (upload, all kernels, download), warm-up %d, %d timed images per variant, variants alternating%s"
             % (a.warmup, a.images, ("; " + a.label) if a.label else "")]
    for size in SIZES:
        ms = time_size(ctx, size, a.warmup, a.images, a.plain_only)
        for name in ms:
            lines.append("%-10s %-7s %s" % (size, name, stats(ms[name])))
    if not a.plain_only:
        lines.append("k_det_undistort alone (the library's event brackets, a pass of its own), k1 = %g, k2 = %g, f = 0.9 width:" % (K1, K2))
        for size in SIZES:
            w, h, _ = SIZES[size]
            n, total = kernel_time(ctx, size, a.images)
            us = 1e3 * total / max(n, 1)
            lines.append("%-10s %d launches, %.1f us each; %.1f MB read + written per launch (2 x width x height x 3): %.0f GB/s"
                         % (size, n, us, 2e-6 * w * h * 3, 2.0 * w * h * 3 / (us * 1e-6) / 1e9 if us > 0 else 0.0))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
