#!/usr/bin/env python3
"""Milliseconds per image of the device line segment detector (l3d_detect_segments) at 640x480 and 1920x1080, on scenes rendered the way
the golden generator renders them (filled rotated rectangles, noise sigma 2), and the per-kernel split of one separate
rocprofv3 --kernel-trace --stats run.  Writes profiles/detect_times.txt.

    python scripts/time_detect.py                  # both parts
    python scripts/time_detect.py --no-trace       # the timing only
    python scripts/time_detect.py --child SIZE     # what the rocprofv3 run executes: a few images of one size, nothing timed

Each timed call ends with the segments on the host (the call synchronises the stream to copy them back), so the window holds the upload,
every kernel and the download.  Warm-up first (arenas, code objects, the sampler's tables); the median and the spread of >= 20 images are
reported, never a single run."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SIZES = {"640x480": (640, 480, 20), "1920x1080": (1920, 1080, 20)}


def scenes(size, count, seed=99):
    from make_golden_detect import noisy, render_rects
    w, h, n = SIZES[size]
    rng = np.random.default_rng(seed)
    return [noisy(render_rects(rng, w, h, n), rng, 2) for _ in range(count)]


def time_size(ctx, size, warmup, images):
    imgs = scenes(size, 4)
    for k in range(warmup):
        ctx.detect_segments(imgs[k % len(imgs)])
    ms, segs = [], []
    for k in range(images):
        t0 = time.perf_counter()
        s = ctx.detect_segments(imgs[k % len(imgs)])         # returns with the segments on the host: the stream is synchronised inside
        ms.append((time.perf_counter() - t0) * 1e3)
        segs.append(len(s))
    ms = np.array(ms)
    return dict(size=size, images=images, median=float(np.median(ms)), p10=float(np.percentile(ms, 10)), p90=float(np.percentile(ms, 90)),
                min=float(ms.min()), max=float(ms.max()), segments=float(np.mean(segs)))


def kernel_split(size):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--child", size]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return ["rocprofv3 run failed (exit %d): %s" % (r.returncode, r.stderr[-300:])]
        rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    out = []
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        m = re.search(r"(k_det_\w+|\w*radix\w*|\w*scan\w*|\w*sort\w*|__amd_rocclr_\w+)", r["Name"])
        out.append("  %-40s calls %6s  avg %9.1f us  total %8.2f ms  %5.1f %%" % ((m.group(1) if m else r["Name"])[:40], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                                float(r["TotalDurationNs"]) / 1e6, 100.0 * float(r["TotalDurationNs"]) / total))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_times.txt"))
    a = ap.parse_args()
    from line3d_amd import capi
    if a.child:
        ctx = capi.Context(0)
        for img in scenes(a.child, 4) * 2:
            ctx.detect_segments(img)
        ctx.close()
        return
    ctx = capi.Context(0)
    lines = ["line segment detector, l3d_detect_segments: ms per image (upload, all kernels, download), warm-up %d, %d timed images per size" % (a.warmup, a.images)]
    for size in SIZES:
        r = time_size(ctx, size, a.warmup, a.images)
        lines.append("%-10s median %7.2f ms   p10 %7.2f  p90 %7.2f   min %7.2f  max %7.2f   (%.0f segments per image)"
                     % (r["size"], r["median"], r["p10"], r["p90"], r["min"], r["max"], r["segments"]))
    ctx.close()
    ref = os.path.join(ROOT, "tests", "golden", "detect_ref.npz")
    if os.path.exists(ref):
        lines.append("reference detector (lsd.cpp) on the CPU of the machine that made the golden, one 1920x1080 scene of this kind: %.3f s"
                     % float(np.load(ref)["ref_cpu_seconds_1080p"]))
    if not a.no_trace:
        for size in SIZES:
            lines.append("per kernel, %s, 8 images, a separate rocprofv3 --kernel-trace --stats run:" % size)
            lines += kernel_split(size)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
