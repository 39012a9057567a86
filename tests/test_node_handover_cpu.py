"""Node mode 2 with a warm hand-over between the turns (l3d_line3d_set_turn_handover) on a machine without a GPU: the header declares and the library
exports the new calls, a null handle is refused, the C++ facade's setTurnHandover compiles and links, scripts/memory_plan.py --mode turns --handover
runs, and the static plan of the turns (l3d_turn_handover_plan: host logic, no context) on hand-built schedules -- the helix with ids 0..V-1, the same
with ids offset by 1000, a scattered non-mutual one: every turn's preload lies in what its predecessor holds, the chains' ranges cover the chain, and a
turn is deferred exactly when a later turn's block produces an early-return or alias input of its rows (tests/turn_schedule.py: expected_deferred)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from turn_schedule import expected_deferred, plan, reach_of, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["l3d_line3d_set_turn_handover", "l3d_line3d_node_turn_views", "l3d_turn_handover_plan"]

FACADE_SRC = r'''
#include "line3D_amd.hpp"
int main() {
    std::vector<int> devices{ 0, 0 };
    L3D::Line3D line3D("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false, devices);
    const bool mode = line3D.setNodeMode(2);
    const bool on = line3D.setTurnHandover(true);
    const bool off = line3D.setTurnHandover(false);
    // (without a GPU there is no object: every call reports and returns false)
    return line3D.valid() ? ((mode && on && off) ? 0 : 1) : ((!mode && !on && !off) ? 0 : 1);
}
'''


def _lib():
    return C.CDLL(os.path.join(ROOT, "line3d_amd", "libline3d_amd.so"))


def test_header_declares_and_library_exports_the_new_calls():
    header = open(os.path.join(ROOT, "include", "line3d_amd.h")).read()
    lib = _lib()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in header, name
        assert getattr(lib, name) is not None
    assert "bool setTurnHandover(const bool on)" in open(os.path.join(ROOT, "include", "line3D_amd.hpp")).read()


def test_null_handles_are_refused():
    lib = _lib()
    n, v = C.c_int64(7), C.c_int(7)
    assert lib.l3d_line3d_set_turn_handover(None, C.c_int(1)) == 1
    assert lib.l3d_line3d_node_turn_views(None, C.c_int(0), C.byref(n), C.byref(v)) == 1
    assert lib.l3d_turn_handover_plan(None, C.c_int(0), C.c_int(2), None, None) == 1


def test_facade_set_turn_handover_compiles_and_links():
    import torch
    lib = os.path.join(ROOT, "line3d_amd")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
        open(src, "w").write(FACADE_SRC)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
        if not torch.cuda.is_available():
            assert subprocess.run([exe], stderr=subprocess.DEVNULL, timeout=120).returncode == 0


def test_memory_plan_turns_with_handover():
    args = ["--mode", "turns", "--views", "512", "--segments", "2000", "--neighbors", "12", "--world", "8", "--kept", "0.1", "--json"]
    run = lambda extra: json.loads(subprocess.check_output([sys.executable, os.path.join(ROOT, "scripts", "memory_plan.py")] + args + extra, timeout=120).decode())
    plain, hand = run([]), run(["--handover"])
    assert hand["handover"] is True and hand["across_turns_gb"]["handover_packages"] > 0
    assert not any(r["what"].startswith("send + gathered slots") for r in hand["rows"]) and any(r["what"].startswith("send + gathered slots") for r in plain["rows"])
    # the same arena per turn (block + check + tail views = the keep set's count), the chain's scratch without the ring of slots
    assert hand["per_turn_gb"]["arena_of_the_keep_set"] == plain["per_turn_gb"]["arena_of_the_keep_set"]
    assert hand["per_turn_gb"]["chain_scratch"] < plain["per_turn_gb"]["chain_scratch"]


# ---- the builder of the schedules ------------------------------------------------------------------------------------------------------------------
def _helix(V, h, offset=0):
    """ids offset..offset+V-1, every view's neighbours the views within h positions: mutual neighbourhoods"""
    ids = [offset + k for k in range(V)]
    return ids, {offset + k: [offset + j for j in range(max(0, k - h), min(V, k + h + 1)) if j != k] for k in range(V)}


def _scattered(V, seed):
    """ids scattered over 0..5V, up to four neighbours among the views within six positions, NOT mutual: early returns in mid-chain"""
    rng = np.random.RandomState(seed)
    ids = sorted(int(x) for x in rng.choice(5 * V, V, replace=False))
    nb = {}
    for k, v in enumerate(ids):
        near = [ids[j] for j in range(max(0, k - 6), min(V, k + 7)) if j != k]
        nb[v] = sorted(int(x) for x in rng.choice(near, min(4, len(near)), replace=False))
    return ids, nb


def test_the_schedule_builder_on_a_chain_of_five_views():
    ids, nb = _helix(5, 1)
    views = schedule(ids, nb)
    assert [v["id"] for v in views] == [0, 1, 2, 3, 4]
    # view 0 matches view 1; views 1..3 match their successor and take their predecessor as a source; the last view has nothing left to match
    assert [v["n_tbm"] for v in views] == [1, 1, 1, 1, 0]
    assert [list(v["src_idx"]) for v in views] == [[], [0], [1], [2], [3]]
    assert [list(v["src_cam"]) for v in views] == [[], [0], [0], [0], [0]]        # (the source is the first entry of each neighbour list)
    assert reach_of(views) == (1, 1)
    # a neighbour that does not name the view back is no source
    views = schedule([0, 1, 2], {0: [1], 1: [2], 2: [0, 1]})
    assert [list(v["src_idx"]) for v in views] == [[], [], [1]] and [v["n_tbm"] for v in views] == [1, 1, 0]


def _check_plan(views, W):
    lib = _lib()
    n = len(views)
    turns, info = plan(lib, views, W)
    reach, window = reach_of(views)
    assert info["reach"] == reach and info["tail"] == 2 * reach and info["check"] == max(window, 2 * reach)
    covered = np.zeros(n, int)
    for r, t in enumerate(turns):
        assert (t["own0"], t["own1"]) == ((n * r) // W, (n * (r + 1)) // W)
        assert t["run1"] == min(n, t["own1"] + info["tail"]) and t["run0"] == (0 if r == 0 else t["own0"]) and t["pre0"] == (0 if r == 0 else max(0, t["own0"] - info["check"]))
        assert t["pre0"] <= t["row0"] <= t["row1"] <= t["run1"]
        covered[t["run0"]:t["run1"]] += 1
        if r > 0:   # the preload lies in what the predecessor holds: what it took over and what it computed
            p = turns[r - 1]
            assert p["pre0"] <= t["pre0"] and t["run0"] <= p["run1"], (r, p, t)
    assert covered.min() >= 1, "the chains' ranges do not cover the chain"
    assert [t["deferred"] for t in turns] == expected_deferred(views, turns)
    return turns, info


@pytest.mark.parametrize("V,h,W", [(64, 3, 4), (256, 6, 8), (24, 4, 8), (40, 2, 1)])
def test_plan_of_the_helix_defers_turn_0_alone(V, h, W):
    """ids 0..V-1, mutual neighbourhoods: the last view returns early, its local camera numbers 0..h-1 read as view ids name the first views -- rows of
    turn 0, whose inputs (the records of the last view's sources) the last turn produces"""
    turns, info = _check_plan(schedule(*_helix(V, h)), W)
    assert info["supported"] == 1
    if W > 1 and V // W >= 4 * h:       # (blocks longer than check + tail: the last view's sources are the last turn's alone)
        assert [t["deferred"] for t in turns] == [1] + [0] * (W - 1)
    assert turns[-1]["deferred"] == 0   # (nothing is later than the last turn)


def test_plan_of_the_helix_with_offset_ids_defers_nothing():
    """ids 1000..: the local camera numbers name no view, so no row far from the last view gets an entry of it"""
    for V, h, W in ((64, 3, 4), (256, 6, 8), (24, 4, 8)):
        turns, info = _check_plan(schedule(*_helix(V, h, offset=1000)), W)
        assert info["supported"] == 1 and [t["deferred"] for t in turns] == [0] * W


@pytest.mark.parametrize("seed", [3, 77, 2026])
def test_plan_of_scattered_non_mutual_neighbourhoods(seed):
    views = schedule(*_scattered(48, seed))
    assert sum(1 for v in views if v["n_tbm"] == 0 and len(v["src_idx"])) >= 2, "the scene should have early returns in mid-chain"
    for W in (2, 3, 6):
        turns, _ = _check_plan(views, W)
        assert turns[-1]["deferred"] == 0


def _alternating(n_early, offset=1000):
    """2 n views, ids from `offset`: every odd view has nothing left to match and takes the view before it as its source -- n early returns"""
    views = []
    for k in range(2 * n_early):
        odd = k % 2 == 1
        views.append(dict(id=offset + k, l2g=np.array([offset + k - 1] if odd else [offset + k + 1], np.uint32), n_tbm=0 if odd else 1,
                          src_cam=np.array([0] if odd else [], np.int32), src_idx=np.array([k - 1] if odd else [], np.int32)))
    return views


def test_plan_refuses_what_the_partition_refuses():
    """more than 64 early-return views (the control block of k_early_pack holds 64 ids): supported = 0 -- such a compute3Dmodel runs as plain mode 2;
    64 of them are taken"""
    lib = _lib()
    for n_early, supported in ((64, 1), (65, 0)):
        turns, info = plan(lib, _alternating(n_early), 4)
        assert info["supported"] == supported, (n_early, info)
        assert [t["deferred"] for t in turns] == [0] * 4       # (every source sits right in front of its early return: held by whoever holds that)
    # a view a turn would ingest BOTH as the sliver of a source and as a named view (l3d_chain_partition.hip: the alias-and-source case of the partition): 40 views
    # in 2 turns, view 12 returns early with view 7 as its source under the local camera number 7 -- which, read as a view id, names view 7 again.
    # Turn 1 holds the views from 10 on (check = 2 x reach = 10): it holds 12, not 7, and would need 7's sliver and 7's best matches in one list
    v = [dict(id=k, l2g=np.array([k + 1], np.uint32), n_tbm=1, src_cam=np.array([], np.int32), src_idx=np.array([], np.int32)) for k in range(40)]
    v[12].update(n_tbm=0, src_cam=np.array([7], np.int32), src_idx=np.array([7], np.int32))
    turns, info = plan(lib, v, 2)
    assert (info["reach"], info["check"]) == (5, 10) and 7 < turns[1]["pre0"] <= 12, (turns, info)
    assert info["supported"] == 0
    v[12]["src_cam"] = np.array([3], np.int32)         # (naming another view: two lists, taken)
    assert plan(lib, v, 2)[1]["supported"] == 1
