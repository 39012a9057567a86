#!/usr/bin/env python3
"""What a batch buys: per-image milliseconds of the detector for single calls and for batches of 1, 4, 16 and 64, from pixels and from JPEG files, at
640x480 and 1920x1080.  Writes profiles/batch_times.txt.

    python scripts/time_batch.py --parent /path/to/the/parent/commit's/libline3d_amd.so [--out F]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_batch.py --trace-batch B      # a run of its own: kernel launches per image
    python scripts/time_batch.py --append-trace DIR_B1 DIR_B16 [--out F]                          # ... read back from the two traces

Scenes and settings of scripts/time_jpeg.py / time_undistort.py: the seeded scenes (four per size, cycled), JPEG quality 90 with 4:2:0 (encoded here
with Pillow), warm-up 5, the variants alternating call by call so that all see the same machine, each call ending with the segments on the host.
A library is measured in a process of its own (L3D_LIBRARY): (a) single calls with the parent commit's build, run twice -- before and after --,
(b) single calls with this build, by the same procedure as (a): pixels and JPEG alternate, nothing else runs in between (single calls timed between
batches of 64 start on cold host caches and came out 0.1 ms slower at 1920x1080 from JPEG than the same calls on their own), (c) batches with this
build.  Two things decide, and the last lines of the file say how they came out: (b) may not
be slower than (a) by more than the two runs of (a) differ, and the per-image time at a batch of 16 must be below (a)."""
import argparse
import csv
import glob
import io
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
BATCHES = (1, 4, 16, 64)


def inputs(size):
    """four seeded scenes of the size as pixels and as JPEG files"""
    from PIL import Image
    from time_undistort import scenes
    imgs = scenes(size, 4)
    files = []
    for img in imgs:
        buf = io.BytesIO()
        Image.fromarray(img[:, :, ::-1]).save(buf, "JPEG", quality=90, subsampling=2)
        files.append(buf.getvalue())
    return imgs, files


def worker(a):
    """this process's library: single calls, and with --batches the batched call; prints {size: {kind: {variant: [ms per image]}}}"""
    from line3d_amd import capi
    ctx = capi.Context(0)
    batched = a.batches
    out = {}
    for size in SIZES:
        imgs, files = inputs(size)
        kinds = (("pixels", imgs, ctx.detect_segments), ("jpeg", files, ctx.detect_segments_jpeg))
        variants = [("batch %d" % b, b) for b in BATCHES] if batched else [("single", 1)]
        out[size] = {kind: {name: [] for name, _ in variants} for kind, _, _ in kinds}
        for k in range(a.warmup + a.rounds):
            for name, b in variants:
                for kind, src, single in kinds:
                    batch = [src[(k + j) % len(src)] for j in range(b)]
                    t0 = time.perf_counter()
                    if name == "single":
                        single(batch[0])
                    else:
                        ctx.detect_segments_batch(batch)
                    if k >= a.warmup:
                        out[size][kind][name].append((time.perf_counter() - t0) * 1e3 / b)
    ctx.close()
    print("RESULT " + json.dumps(out))


def trace_batch(a):
    """for a kernel trace: three calls of a batch of B at 640x480 from pixels, nothing else on the device"""
    from line3d_amd import capi
    ctx = capi.Context(0)
    imgs, _ = inputs("640x480")
    for _ in range(3):
        ctx.detect_segments_batch([imgs[j % len(imgs)] for j in range(a.trace_batch)])
    ctx.close()


def launches(directory):
    total = 0
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                total += int(row.get("Calls") or row.get("calls") or 0)
    return total


def stats(ms):
    ms = np.array(ms)
    return "median %7.3f ms   p10 %7.3f  p90 %7.3f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))


def run_worker(a, library, batches):
    env = dict(os.environ)
    if library:
        env["L3D_LIBRARY"] = library
    else:
        env.pop("L3D_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(a.warmup), "--rounds", str(a.rounds)] + (["--batches"] if batches else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's build of the library (kept outside the repository's history)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--batches", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=400)
    ap.add_argument("--trace-batch", type=int, default=0)
    ap.add_argument("--append-trace", nargs=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.trace_batch:
        return trace_batch(a)
    if a.append_trace:
        n1, n16 = launches(a.append_trace[0]), launches(a.append_trace[1])
        text = ("kernel trace with stats, 640x480 from pixels, three calls each, in runs of their own: a batch of 1 takes %d kernel launches (%.1f per image), "
                "a batch of 16 takes %d (%.1f per image)\n" % (n1, n1 / 3.0, n16, n16 / 48.0))
        print(text, end="")
        with open(a.out, "a") as f:
            f.write(text)
        return
    if not a.parent:
        ap.error("--parent is needed")
    runs = [("parent, run 1", run_worker(a, os.path.abspath(a.parent), False)), ("this build", run_worker(a, None, False)),
            ("parent, run 2", run_worker(a, os.path.abspath(a.parent), False)), ("this build", run_worker(a, None, True))]
    lines = ["the detector over batches, ms per image, warm-up %d, %d timed rounds per variant, variants alternating; a library per process" % (a.warmup, a.rounds)]
    ok_single, ok_batch = True, True
    for size in SIZES:
        for kind in ("pixels", "jpeg"):
            lines.append("%s, %s" % (size, kind))
            med = {}
            for name, res in runs:
                for variant, ms in res[size][kind].items():
                    med[(name, variant)] = float(np.median(ms))
                    lines.append("  %-14s %-9s %s" % (name, variant, stats(ms)))
            a1, a2, b = med[("parent, run 1", "single")], med[("parent, run 2", "single")], med[("this build", "single")]
            spread = abs(a1 - a2)
            single_fine, batch_fine = b - min(a1, a2) <= spread, med[("this build", "batch 16")] < min(a1, a2)
            ok_single, ok_batch = ok_single and single_fine, ok_batch and batch_fine
            lines.append("  single calls: parent %.3f / %.3f (spread %.3f), this build %.3f: %s" % (a1, a2, spread, b, "not slower" if single_fine else "SLOWER than the spread allows"))
            lines.append("  batch of 16: %.3f ms per image, %.2f x the parent's single call: %s" % (med[("this build", "batch 16")], med[("this build", "batch 16")] / min(a1, a2),
                                                                                               "faster" if batch_fine else "NOT faster"))
    lines.append("single calls not slower than the parent's at every size and kind: %s" % ("yes" if ok_single else "NO"))
    lines.append("a batch of 16 faster per image than the parent's single call at every size and kind: %s" % ("yes" if ok_batch else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
