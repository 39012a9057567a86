#!/usr/bin/env python3
"""What it costs to bring an image into the detector: per-image milliseconds of Context.detect_segments_batch (the detector run of add_images) at
640x480 and 1920x1080 for batches of 1, 16 and 64, from host pixels (uploaded) and from images that are in device memory already -- a uint8
H x W x C tensor and a float32 C x H x W tensor in [0, 1] (gathered by k_det_ingest).  Writes profiles/device_images_times.txt.

    python scripts/time_device_images.py --parent /path/to/the/parent/commit's/libline3d_amd.so [--out F]

The procedure of scripts/time_batch.py: the seeded scenes of scripts/time_undistort.py (four per size, cycled), warm-up 5, the variants alternating
call by call so that all see the same machine, medians with p10 and p90, the profiler off, each call ending with the segments on the host.  A
library is measured in a process of its own (L3D_LIBRARY): host pixels with the parent commit's build, run twice -- before and after --, and
host pixels and the two device variants with this build.  The host-pixel lines of the parent and of this build show whether the existing path
moved; the device lines show what the upload was.  The tensors are on the device before the clock starts and the float tensor holds x / 255,
which ingests to the uint8 image's bytes: all variants detect the same segments (checked once per size)."""
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
BATCHES = (1, 16, 64)


def worker(a):
    """this process's library; prints {size: {variant: {batch: [ms per image]}}}"""
    from line3d_amd import capi
    from time_undistort import scenes
    ctx = capi.Context(0)
    out = {}
    for size in SIZES:
        imgs = scenes(size, 4)
        sources = {"host pixels": imgs}
        if a.device_images:
            import torch
            u8 = [torch.from_numpy(img).cuda() for img in imgs]
            f32 = [capi.device_image(torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)).cuda(), layout="CHW") for img in imgs]
            torch.cuda.synchronize()
            sources["device u8 HxWxC"], sources["device f32 CxHxW"] = u8, f32
            want = ctx.detect_segments(imgs[0]).tobytes()
            assert ctx.detect_segments(u8[0]).tobytes() == want and ctx.detect_segments(f32[0]).tobytes() == want
        out[size] = {name: {str(b): [] for b in BATCHES} for name in sources}
        for k in range(a.warmup + a.rounds):
            for b in BATCHES:
                for name, src in sources.items():
                    batch = [src[(k + j) % len(src)] for j in range(b)]
                    t0 = time.perf_counter()
                    ctx.detect_segments_batch(batch)
                    if k >= a.warmup:
                        out[size][name][str(b)].append((time.perf_counter() - t0) * 1e3 / b)
    ctx.close()
    print("RESULT " + json.dumps(out))


def stats(ms):
    ms = np.array(ms)
    return "median %7.3f ms   p10 %7.3f  p90 %7.3f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))


def run_worker(a, library, device_images):
    env = dict(os.environ)
    if library:
        env["L3D_LIBRARY"] = library
    else:
        env.pop("L3D_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--warmup", str(a.warmup), "--rounds", str(a.rounds)] + (["--device-images"] if device_images else [])
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
    ap.add_argument("--device-images", action="store_true")
    ap.add_argument("--worker-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_images_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent:
        ap.error("--parent is needed")
    runs = [("parent, run 1", run_worker(a, os.path.abspath(a.parent), False)), ("this build", run_worker(a, None, True)),
            ("parent, run 2", run_worker(a, os.path.abspath(a.parent), False))]
    lines = ["images from host and from device memory through detect_segments_batch, ms per image, warm-up %d, %d timed rounds per variant, variants alternating; "
             "a library per process" % (a.warmup, a.rounds)]
    for size in SIZES:
        for b in BATCHES:
            lines.append("%s, batch of %d" % (size, b))
            med = {}
            for name, res in runs:
                for variant, per_batch in res[size].items():
                    med[(name, variant)] = float(np.median(per_batch[str(b)]))
                    lines.append("  %-14s %-18s %s" % (name, variant, stats(per_batch[str(b)])))
            p1, p2, host = med[("parent, run 1", "host pixels")], med[("parent, run 2", "host pixels")], med[("this build", "host pixels")]
            lines.append("  host pixels: parent %.3f / %.3f (spread %.3f), this build %.3f (%+.3f against the nearer run)"
                         % (p1, p2, abs(p1 - p2), host, host - min((p1, p2), key=lambda v: abs(host - v))))
            for variant in ("device u8 HxWxC", "device f32 CxHxW"):
                d = med[("this build", variant)]
                lines.append("  %s: %.3f ms per image, %+.3f ms (%+.1f %%) against this build's host pixels" % (variant, d, d - host, 100.0 * (d - host) / host))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
