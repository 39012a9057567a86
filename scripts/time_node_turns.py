#!/usr/bin/env python3
"""compute3Dmodel of three objects on one GPU, interleaved: node mode 2 with the turns handing the chain over (l3d_line3d_set_turn_handover), plain
mode 2, and the one-device object (profiles/node_turns_handover.txt):

    python3 scripts/time_node_turns.py VIEWS SEGMENTS NEIGHBOURS out.json [--worlds 2 4 8] [--passes 2]

Per W: seconds per pass of each object (a fresh object's first pass, then passes after reset; scene generation and loading not timed), the chain
views every turn computed and its visits, the records per turn, the number of lines, and the device's sampled peak HBM (hipMemGetInfo every 20 ms,
whole device).  Every run's lines are compared with the one-device object's (tolerance 0)."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
hip = C.CDLL("libamdhip64.so")


def hbm_used_gb():
    free, total = C.c_size_t(0), C.c_size_t(0)
    hip.hipMemGetInfo(C.byref(free), C.byref(total))
    return (total.value - free.value) / 2**30


def timed(l, scene, passes, load):
    """seconds of compute3Dmodel per pass and the sampled peak over all of them"""
    peak, stop = [0.0], threading.Event()

    def sampler():
        while not stop.is_set():
            peak[0] = max(peak[0], hbm_used_gb())
            time.sleep(0.02)
    th = threading.Thread(target=sampler)
    th.start()
    secs = []
    try:
        for p in range(passes):
            if p:
                l.reset()
            load(l, scene)
            t0 = time.perf_counter()
            l.compute3Dmodel(False)
            secs.append(round(time.perf_counter() - t0, 3))
    finally:
        stop.set()
        th.join()
    return secs, round(peak[0], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("views", type=int); ap.add_argument("segments", type=int); ap.add_argument("neighbors", type=int); ap.add_argument("out")
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    from helpers import assert_lines_equal
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    V, S, N = a.views, a.segments, a.neighbors
    scene = make_scene(V, S, N, seed=20260)
    out = dict(shape=[V, S, N], passes=a.passes, worlds={})
    ref_lines = None
    for W in a.worlds:
        row = {}
        for name in ("handover", "mode2", "one_device"):
            l = Line3D("", matchingNeighbors=N, device=0) if name == "one_device" else Line3D("", matchingNeighbors=N, devices=[0] * W)
            try:
                if name != "one_device":
                    l.set_node_mode(2)
                    l.set_turn_handover(name == "handover")
                secs, peak = timed(l, scene, a.passes, load_scene)
                lines = l.getResult()
                if ref_lines is None and name == "one_device":
                    ref_lines = lines
                e = dict(seconds=secs, peak_gb=peak, lines=len(lines), kept=int(l.chain_summary()["n_kept"].astype("int64").sum()))
                if name != "one_device":
                    e["turn_views"] = [l.node_turn_views(r) for r in range(W)]
                    e["turn_records"] = [l.node_turn_records(r) for r in range(W)]
                    e["views_computed"] = sum(v for v, _ in e["turn_views"])
                    e["deferred_turns"] = sum(1 for _, k in e["turn_views"] if k > 1)
                row[name] = e
                row.setdefault("_lines", {})[name] = lines
            finally:
                l.close()
            print(W, name, {k: v for k, v in row[name].items() if k != "turn_records"}, flush=True)
        lines = row.pop("_lines")
        ref_lines = ref_lines or lines["one_device"]
        for name in ("handover", "mode2", "one_device"):
            assert_lines_equal(lines[name], ref_lines, 0.0)
        row["lines_equal_one_device"] = True
        out["worlds"][str(W)] = row
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: {n: (e["seconds"], e.get("views_computed")) for n, e in v.items() if isinstance(e, dict)} for k, v in out["worlds"].items()}))


if __name__ == "__main__":
    main()
