#!/usr/bin/env python3
"""What projection and overlays cost (include/line3d_amd.h, "PROJECTION AND OVERLAYS").  Writes profiles/overlay_times.txt.

    python scripts/time_overlay.py [--rounds N] [--out F]

Three workloads: (1) l3d_project_lines of 10^5 3-D segments into 64 cameras of 1920 x 1080; (2) l3d_draw_segments_device of 10^4 projected segments
(camera 0's, repeated to that number) over a 1920 x 1080 x 3 image in device memory, stroke 2 pixels; (3) Line3D.overlay of one view of the smoke scene
make_scene(8, 120, 6, seed=3) over a grey host image.  Per workload: warm-up rounds, then the whole call by the host's clock (it ends in a stream
synchronise) with the profile brackets off -- median, 10th and 90th percentile --, then, in rounds of their own, device time per kernel by event brackets
(profile_get: launches and summed milliseconds).  Beside (1) and (2), as information: the host entry points (the same functions on the host: the projection
on 16 threads, four cameras each; the drawing on one).  Results are compared with the host entry points once, before
anything is timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
N3D, NCAM, NDRAW = 100000, 64, 10000
PROJ = ("proj_count", "proj_scan", "proj_write")
DRAW = ("draw_pieces", "draw_scan", "draw_cover", "draw_resolve")


def stats(ms):
    ms = np.array(ms)
    return "median %8.3f ms   p10 %8.3f  p90 %8.3f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))


def inputs():
    rng = np.random.default_rng(31)
    P = rng.uniform([-6.0, -4.0, 4.0], [6.0, 4.0, 14.0], (N3D, 3))
    Q = P + rng.uniform(-0.8, 0.8, (N3D, 3))
    K = np.array([[1500.0, 0.0, W / 2.0], [0.0, 1500.0, H / 2.0], [0.0, 0.0, 1.0]])
    cams = []
    for k in range(NCAM):
        a = (k - NCAM / 2) * 0.01
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        cams.append((K, R, np.array([0.05 * k - 1.6, 0.0, 0.0]), W, H))
    return np.concatenate([P, Q], 1), cams


def timed(fn, warmup, rounds):
    out = []
    for k in range(warmup + rounds):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            out.append(dt)
    return out


def kernels(ctx, fn, names, rounds):
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(rounds):
        fn()
    got = {k: ctx.profile_get(k) for k in names}
    ctx.profile_enable(False)
    return "   ".join("%s %.4f ms (%d launches)" % (k, got[k][1] / max(1, got[k][0]), got[k][0] // rounds) for k in names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_times.txt"))
    a = ap.parse_args()
    import torch
    from line3d_amd import capi
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    seg3d, cams = inputs()
    carr = capi.cameras(cams)
    ctx = capi.Context(0)
    lines = []
    # (1) projection
    got = ctx.project_lines(seg3d, carr, 1e-6, 0.0)
    want = capi.project_lines_host(seg3d, carr, 1e-6, 0.0)
    from concurrent.futures import ThreadPoolExecutor
    parts = [capi.cameras(cams[k:k + NCAM // 16]) for k in range(0, NCAM, NCAM // 16)]          # (the calls leave the interpreter lock: 16 threads run at once)
    with ThreadPoolExecutor(16) as pool:
        t0 = time.perf_counter()
        list(pool.map(lambda c: capi.project_lines_host(seg3d, c, 1e-6, 0.0), parts))
        host_proj = (time.perf_counter() - t0) * 1e3
    if not all(np.array_equal(x, y) for x, y in zip((got[0].view(np.uint32),) + got[1:], (want[0].view(np.uint32),) + want[1:])):
        raise SystemExit("projection: the device call differs from the host entry point")
    call = timed(lambda: ctx.project_lines(seg3d, carr, 1e-6, 0.0), a.warmup, a.rounds)
    lines += ["l3d_project_lines: %d 3-D segments into %d cameras of %d x %d (%.1f million pairs, %d kept); warm-up %d, %d timed rounds" % (N3D, NCAM, W, H, N3D * NCAM / 1e6, len(got[1]), a.warmup, a.rounds),
              "  the whole call (host clock; upload of 4.8 MB, one chunk, download of the kept segments):  " + stats(call),
              "  device time per kernel (event brackets, mean):  " + kernels(ctx, lambda: ctx.project_lines(seg3d, carr, 1e-6, 0.0), PROJ, a.rounds),
              "  the host entry point on 16 threads of the host (4 cameras each), once: %.1f ms" % host_proj]
    # (2) drawing
    first = got[0][got[3][0]:got[3][1]]
    segs = np.ascontiguousarray(np.resize(first, (NDRAW, 4)), np.float32)
    pal = capi.default_palette()
    rng = np.random.default_rng(32)
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    want = capi.draw_segments_host(base, segs, pal, None, 2.0, 255)
    host_draw = (time.perf_counter() - t0) * 1e3
    t = torch.from_numpy(base).to("cuda:0")
    ctx.draw_segments(t, segs, pal, None, 2.0, 255)
    if not np.array_equal(t.cpu().numpy(), want):
        raise SystemExit("drawing: the device call differs from the host entry point")
    torch.cuda.synchronize()
    call = timed(lambda: ctx.draw_segments(t, segs, pal, None, 2.0, 255), a.warmup, a.rounds)
    lines += ["l3d_draw_segments_device: %d segments (camera 0's %d projected segments, repeated) over %d x %d x 3 in device memory, stroke 2 pixels" % (NDRAW, len(first), W, H),
              "  the whole call (host clock):  " + stats(call),
              "  device time per kernel (event brackets, mean):  " + kernels(ctx, lambda: ctx.draw_segments(t, segs, pal, None, 2.0, 255), DRAW, a.rounds),
              "  the host entry point, once, on one thread (the winner of a pixel is taken over all segments: the call is not split): %.1f ms" % host_draw]
    ctx.close()
    # (3) one view's overlay of the smoke scene
    scene = make_scene(8, 120, 6, seed=3)
    l3d = Line3D("", matchingNeighbors=6, device=0)
    load_scene(l3d, scene)
    l3d.compute3Dmodel(False)
    grey = np.full((H, W, 3), 128, np.uint8)
    vid = scene.views[0]["id"]
    call = timed(lambda: l3d.overlay(vid, grey), a.warmup, a.rounds)
    c2 = l3d.context()
    lines += ["Line3D.overlay: view %d of make_scene(8, 120, 6, seed=3) (%d lines), members and observed model, over a grey %d x %d x 3 host image" % (vid, len(l3d.getResult()), W, H),
              "  the whole call (host clock; the image is uploaded and copied back once per layer):  " + stats(call),
              "  device time per kernel (event brackets, mean; two draws and one projection per overlay):  " + kernels(c2, lambda: l3d.overlay(vid, grey), PROJ + DRAW, a.rounds)]
    l3d.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
