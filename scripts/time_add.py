#!/usr/bin/env python3
"""The add path itself, timed: per-image milliseconds of Line3D.add_image_pixels / add_image_jpeg (single calls) and Line3D.add_images (batches of 16)
at 640x480 and 1920x1080, Python marshalling included, for two checkouts of the project alternating, twice each (a checkout per process):

    python scripts/time_add.py --parent /path/to/a/built/checkout/of/the/parent/commit [--out profiles/add_entry_times.txt]   (appends)

Scenes and JPEG files of scripts/time_batch.py; no segment cache (loadAndStoreSegments off), every view a new id, reset() between rounds.  A median of
this checkout must lie within the parent's two medians widened by their spread on either side."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ("640x480", "1920x1080")
VARIANTS = (("pixels", "single", 1), ("jpeg", "single", 1), ("pixels", "batch 16", 16), ("jpeg", "batch 16", 16))


def worker(a):
    sys.path.insert(0, a.tree)
    import line3d_amd.pipeline as pipeline          # (the checkout under test, before this one's scripts put their own root in front)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import numpy as np
    import time_batch as tb
    K, R, t, wps = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]]), np.eye(3), np.zeros(3), list(range(10))
    out = {"package": os.path.dirname(pipeline.__file__)}
    with tempfile.TemporaryDirectory() as d:
        l3d = pipeline.Line3D(d + os.sep, matchingNeighbors=6)
        for size in SIZES:
            imgs, files = tb.inputs(size)
            src = {"pixels": imgs, "jpeg": files}
            out[size] = {"%s %s" % (kind, name): [] for kind, name, _ in VARIANTS}
            for k in range(a.warmup + a.rounds):
                l3d.reset()
                next_id = 0
                for kind, name, b in VARIANTS:
                    batch = [src[kind][(k + j) % 4] for j in range(b)]
                    ids = list(range(next_id, next_id + b))
                    next_id += b
                    t0 = time.perf_counter()
                    if name == "single":
                        ok = (l3d.add_image_pixels if kind == "pixels" else l3d.add_image_jpeg)(ids[0], batch[0], K, R, t, wps, loadAndStoreSegments=False)
                    else:
                        key = "img" if kind == "pixels" else "data"
                        ok = not any(l3d.add_images([{"imageID": i, key: x, "K": K, "R": R, "t": t, "worldpointIDs": wps} for i, x in zip(ids, batch)],
                                                    loadAndStoreSegments=False))
                    dt = (time.perf_counter() - t0) * 1e3 / b
                    assert ok and l3d.numCameras() == next_id
                    if k >= a.warmup:
                        out[size]["%s %s" % (kind, name)].append(dt)
        l3d.close()
    print("RESULT " + json.dumps(out))


def run_worker(a, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    env = {k: v for k, v in os.environ.items() if k != "L3D_LIBRARY"}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert os.path.samefile(res.pop("package"), os.path.join(tree, "line3d_amd"))
    return res


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--worker-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add_entry_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent:
        ap.error("--parent is needed")
    runs = [("%s, run %d" % (name, rep), run_worker(a, tree)) for rep in (1, 2) for name, tree in (("parent", os.path.abspath(a.parent)), ("this build", ROOT))]
    lines = ["", "the add path itself (scripts/time_add.py): Line3D.add_image_pixels / add_image_jpeg / add_images through Python, ms per image, warm-up %d, %d timed "
             "rounds, no segment cache; a checkout per process, order: parent, this build, parent, this build" % (a.warmup, a.rounds)]
    ok = True
    for size in SIZES:
        for kind, name, _ in VARIANTS:
            v = "%s %s" % (kind, name)
            med = {run: float(np.median(res[size][v])) for run, res in runs}
            for run, res in runs:
                ms = np.array(res[size][v])
                lines.append("  %-10s %-16s %-18s median %7.3f ms   p10 %7.3f  p90 %7.3f" % (size, v, run, np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90)))
            p1, p2 = med["parent, run 1"], med["parent, run 2"]
            spread = abs(p1 - p2)
            lo, hi = min(p1, p2) - spread, max(p1, p2) + spread
            for r in (1, 2):
                x = med["this build, run %d" % r]
                ok = ok and x <= hi
                lines.append("    parent %.3f / %.3f (spread %.3f, interval %.3f .. %.3f), this build run %d %.3f: %s"
                             % (p1, p2, spread, lo, hi, r, x, "within" if lo <= x <= hi else "below the interval" if x < lo else "ABOVE the interval"))
    lines.append("no median of this build above the parent's interval: %s" % ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
