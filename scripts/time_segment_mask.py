#!/usr/bin/env python3
"""What a segment mask costs (include/line3d_amd.h, "A SEGMENT MASK"): l3d_mask_segments on 3000 segments against 1920 x 1080 masks, with and without a
lens, the mask in host and in device memory.  Writes profiles/segment_mask_times.txt.

    python scripts/time_segment_mask.py [--rounds N] [--out F]

Per variant: the whole call by the host's clock (it ends in a stream synchronise), with the profile brackets off; then, in rounds of their own, the three
kernels by event brackets (profile_get: launches and summed milliseconds).  Warm-up rounds first, the variants alternating round by round.  The segments are
20 to 300 pixels long and lie anywhere in the image; the mask is made of 64-pixel cells of which about a quarter are invalid, so about a third of the
segments are cut; mode SPLIT, max_gap 2, min_length 10.  The result of every variant is compared with the host entry point's once, before anything is
timed (the lens is BROWN: no atan)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, NSEG = 1920, 1080, 3000
KERNELS = ("segmask_count", "segmask_scan", "segmask_write")


def inputs():
    rng = np.random.default_rng(20)
    cell = 64
    g = rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell)) < 0.75
    mask = (np.kron(g, np.ones((cell, cell))) * 255).astype(np.uint8)[:H, :W].copy()
    a = np.stack([rng.uniform(0, W, NSEG), rng.uniform(0, H, NSEG)], 1)
    ang, ln = rng.uniform(0, 2 * np.pi, NSEG), rng.uniform(20.0, 300.0, NSEG)
    b = a + np.stack([np.cos(ang), np.sin(ang)], 1) * ln[:, None]
    return mask, np.concatenate([a, b], 1).astype(np.float32)


def stats(ms):
    ms = np.array(ms)
    return "median %7.3f ms   p10 %7.3f  p90 %7.3f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_mask_times.txt"))
    a = ap.parse_args()
    import torch
    from line3d_amd import capi
    mask, segs = inputs()
    ctx = capi.Context(0)
    dmask = torch.from_numpy(mask).to("cuda:0")
    torch.cuda.synchronize()
    cam = (1500.0, 1500.0, 960.0, 540.0)
    lens = capi.lens("brown", [-0.12, 0.03, 0.0006, -0.0004, 0.002], camera=(1480.0, 1490.0, 955.0, 545.0))
    kw = dict(mode="split", max_gap=2, min_length=10.0)
    variants = {
        "no lens, host mask  ": capi.segment_mask(mask, **kw),
        "no lens, device mask": capi.segment_mask(dmask, **kw),
        "lens,    host mask  ": capi.segment_mask(mask, lens=lens, camera=cam, **kw),
        "lens,    device mask": capi.segment_mask(dmask, lens=lens, camera=cam, **kw),
    }
    counts = {}
    for name, m in variants.items():
        got = ctx.mask_segments(segs, m)
        hm = capi.segment_mask(mask, lens=lens if name.startswith("lens") else None, camera=cam, **kw)
        want = capi.mask_segments_host(segs, hm)
        if not (np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])):
            raise SystemExit("%s: the device call differs from the host entry point" % name.strip())
        counts[name] = (len(got[1]), len(set(got[1].tolist())))
    call = {v: [] for v in variants}
    for k in range(a.warmup + a.rounds):
        for name, m in variants.items():
            t0 = time.perf_counter()
            ctx.mask_segments(segs, m)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                call[name].append(dt)
    kern = {}
    ctx.profile_enable(True)
    for name, m in variants.items():
        ctx.profile_reset()
        for k in range(a.rounds):
            ctx.mask_segments(segs, m)
        kern[name] = {k: ctx.profile_get(k) for k in KERNELS}
    ctx.profile_enable(False)
    ctx.close()
    lines = ["l3d_mask_segments: %d segments of 20 to 300 pixels, %d x %d mask of 64-pixel cells (a quarter invalid), SPLIT, max_gap 2, min_length 10" % (NSEG, W, H),
             "warm-up %d, %d timed rounds per variant, variants alternating; every variant equals the host entry point bit for bit" % (a.warmup, a.rounds),
             "the whole call (host clock around the call, which ends in a stream synchronise; a host mask is 2.07 MB uploaded per call):"]
    for name in variants:
        lines.append("  %s  %s   -> %d segments from %d of the %d" % (name, stats(call[name]), counts[name][0], counts[name][1], NSEG))
    lines.append("the kernels alone (event brackets, mean of %d launches each):" % a.rounds)
    for name in variants:
        lines.append("  %s  " % name + "   ".join("%s %.4f ms" % (k, kern[name][k][1] / max(1, kern[name][k][0])) for k in KERNELS))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
