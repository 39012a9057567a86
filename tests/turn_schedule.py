"""Shared by tests/test_node_handover_cpu.py and tests/test_gpu_node_handover.py: the static schedule of matchViews built by hand (as _schedule of
tests/test_gpu_node_turns.py builds it), l3d_turn_handover_plan called on it, and the rule a turn is deferred by, written down independently of the
library: a turn is deferred exactly when one of the early-return or alias inputs of its rows is produced by a later turn's piece."""
import ctypes as C

import numpy as np


class ChainView(C.Structure):          # include/line3d_amd.h: l3d_chain_view (tests/test_partition_keep_cpu.py checks this layout against the header)
    _fields_ = [("view_id", C.c_uint32), ("src_segs", C.c_void_p), ("S_src", C.c_int32), ("RtKinv_src", C.c_void_p), ("C_src", C.c_void_p),
                ("tgt_segs", C.c_void_p), ("n_tgt", C.c_int32), ("offsets", C.c_void_p), ("N", C.c_int32),
                ("F", C.c_void_p), ("RtKinv", C.c_void_p), ("centers", C.c_void_p), ("P", C.c_void_p),
                ("to_be_matched", C.c_void_p), ("n_tbm", C.c_int32), ("local2global", C.c_void_p),
                ("source_cam", C.c_void_p), ("source_index", C.c_void_p), ("n_sources", C.c_int32),
                ("sigma_p", C.c_float), ("sigma_a", C.c_float), ("spatial_k", C.c_float)]


def schedule(ids, neighbours):
    """The static schedule of matchViews (line3D.cc:620-648, 698-730) in chain order = ascending ids: a view still has to match the neighbours
    that were not processed before it; an already processed neighbour that matched it is a source."""
    order = sorted(ids)
    pos = {v: k for k, v in enumerate(order)}
    views = []
    for k, v in enumerate(order):
        nb = neighbours[v]
        tbm = [q for q, n in enumerate(nb) if pos[n] > k]
        src = [(q, pos[n]) for q, n in enumerate(nb) if pos[n] < k and v in neighbours[n]]
        views.append(dict(id=v, l2g=np.array(nb, np.uint32), n_tbm=len(tbm), src_cam=np.array([q for q, _ in src], np.int32), src_idx=np.array([p for _, p in src], np.int32)))
    return views


def scene_schedule(scene):
    """the schedule of a synthetic scene: its neighbourhoods are its similarity lists"""
    return schedule([v["id"] for v in scene.views], {v["id"]: sorted(v["sims"]) for v in scene.views})


def reach_of(views):
    pos = {v["id"]: k for k, v in enumerate(views)}
    window = max([1] + [k - int(s) for k, v in enumerate(views) for s in v["src_idx"]])
    return max([window] + [abs(pos[int(n)] - k) for k, v in enumerate(views) for n in v["l2g"] if int(n) in pos]), window


def plan(lib, views, W):
    """l3d_turn_handover_plan: (list of dict(pre0, run0, run1, row0, row1, own0, own1, deferred), dict(reach, check, tail, supported))"""
    arr = (ChainView * len(views))()
    for k, v in enumerate(views):
        arr[k].view_id = v["id"]; arr[k].N = len(v["l2g"]); arr[k].n_tbm = v["n_tbm"]
        arr[k].local2global = v["l2g"].ctypes.data; arr[k].n_sources = len(v["src_cam"])
        arr[k].source_cam = v["src_cam"].ctypes.data; arr[k].source_index = v["src_idx"].ctypes.data
    out = np.zeros(8 * W, np.int32)
    info = np.zeros(4, np.int32)
    rc = lib.l3d_turn_handover_plan(arr, C.c_int(len(views)), C.c_int(W), out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    assert rc == 0
    keys = ("pre0", "run0", "run1", "row0", "row1", "own0", "own1", "deferred")
    return [dict(zip(keys, (int(x) for x in out[8 * r:8 * r + 8]))) for r in range(W)], dict(zip(("reach", "check", "tail", "supported"), (int(x) for x in info)))


def expected_deferred(views, turns):
    """Per turn: does a LATER turn's block produce an input of its rows?  The inputs the early-return quirk creates (cudawrapper.cu:877-878,
    line3D.cc:861-865): an early-return view e (nothing left to match, but sources) is rebuilt from the records of its sources that point at it, and its
    entries are filed in the rows of the views its sources' LOCAL camera numbers name (read as view ids) and in its own rows, where they name those views'
    segments.  So a turn whose rows hold such a named view, or that holds e, needs the records of every source of e; a turn whose rows hold e needs
    the best matches of every (verified) view e's local camera numbers name.  What the turn holds itself is no input; the producer of anything else is
    the turn that owns the view."""
    n, W = len(views), len(turns)
    pos = {v["id"]: k for k, v in enumerate(views)}
    owner = lambda k: max(r for r in range(W) if (n * r) // W <= k)
    out = []
    for r, t in enumerate(turns):
        held = lambda k: t["pre0"] <= k < t["run1"]
        rows = lambda k: t["row0"] <= k < t["row1"]
        producers = []
        for e, v in enumerate(views):
            if v["n_tbm"] != 0 or len(v["src_idx"]) == 0:
                continue
            sources = [(int(q), int(s)) for q, s in zip(v["src_cam"], v["src_idx"]) if s < e and views[s]["n_tbm"] > 0]
            named_rows = [pos[q] for q, _ in sources if q in pos]
            named_best = [pos[int(q)] for q in v["src_cam"] if int(q) in pos and views[pos[int(q)]]["n_tbm"] > 0]
            if not (held(e) or any(rows(b) for b in named_rows)):
                continue
            producers += [owner(s) for _, s in sources if not held(s)]
            if rows(e):
                producers += [owner(b) for b in named_best if not held(b)]
        out.append(1 if any(p > r for p in producers) else 0)
    return out
