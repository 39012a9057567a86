"""Node mode 2 with a warm hand-over between the turns (l3d_line3d_set_turn_handover): turn r computes only its own piece of the chain, warm from
the tail turn r - 1 left, instead of the whole chain.  With virtual ranks on the one GPU of the test box:
  * lines, affinity list and per-view kept counts equal the one-device object's (three and eight turns, blocks shorter than the tail, the scattered
    non-mutual scene with early returns in mid-chain, the config-2 golden of the oracle);
  * the chain work is not W-fold: the views all turns computed stay within 2 (V + W 2 reach), nobody is visited more than twice, no turn's arena holds
    half of the records, and the same object with the hand-over off reports (V, 1) for every rank;
  * with the room for kept records capped between twice the largest turn's arena and the one chain's, the one-device object fails with
    L3D_ERR_NOMEM and the hand-over object returns the uncapped model;
  * the switch is refused where it has no meaning, and an injected exchange failure in the collective finish names the rank and reset recovers.
Reference behaviour: matchViews streams a view at a time and spills to disk (line3D.cc:620-648, view.cc:150-224) -- no bound by device memory."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_lines_equal
from turn_schedule import plan, reach_of, scene_schedule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_PER_RECORD = 32 + 4           # a kept record and its side word (l3d_chain.hip: ch_kept, ch_keptcam)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _outcome(l):
    A, n_nodes = l.affinity()
    return dict(lines=l.getResult(), A=_sha(A), n_A=len(A), n_nodes=n_nodes, kept=l.chain_summary()["n_kept"].copy(), cams=l.numCameras())


def _single(scene, N, diffusion, loader=None):
    from line3d_amd.pipeline import Line3D, load_scene
    l = Line3D("", matchingNeighbors=N, device=0)
    try:
        (loader or load_scene)(l, scene)
        l.compute3Dmodel(diffusion)
        return _outcome(l)
    finally:
        l.close()


def _node_object(N, devices, env=None):
    """a node object in mode 2 with the hand-over on; env: options every rank's context reads when it is created"""
    from line3d_amd.pipeline import Line3D
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update({k: str(v) for k, v in (env or {}).items()})
    try:
        l = Line3D("", matchingNeighbors=N, devices=devices)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert l.num_ranks() == len(devices)
    l.set_node_mode(2)
    l.set_turn_handover(True)
    return l


def _turn_figures(l, W):
    return dict(turn_records=[l.node_turn_records(r) for r in range(W)], turn_views=[l.node_turn_views(r) for r in range(W)])


def _handover(scene, N, devices, diffusion, loader=None, env=None):
    from line3d_amd.pipeline import load_scene
    l = _node_object(N, devices, env)
    try:
        (loader or load_scene)(l, scene)
        l.compute3Dmodel(diffusion)
        out = _outcome(l)
        out.update(_turn_figures(l, len(devices)))
        return out
    finally:
        l.close()


def _assert_same(got, ref):
    assert got["cams"] == ref["cams"]
    assert got["n_nodes"] == ref["n_nodes"] and got["n_A"] == ref["n_A"] and got["A"] == ref["A"], "affinity list differs from the single device's"
    assert np.array_equal(got["kept"], ref["kept"]), "per-view kept counts differ from the single device's"
    assert_lines_equal(got["lines"], ref["lines"], 0.0)


def _assert_handed_over(got, V):
    """the run really took the hand-over path: no turn computed the whole chain twice over, the first turn starts at view 0"""
    views = got["turn_views"]
    assert all(1 <= visits <= 2 for _, visits in views), views
    assert any(n < V for n, _ in views), views


# ---- 1. equal to one device -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diffusion", [False, True], ids=["plain", "diffusion"])
def test_three_turns_equal_one_device(diffusion):
    from line3d_amd.synth import make_scene
    N = 8
    scene = make_scene(48, 400, N, seed=11)
    ref = _single(scene, N, diffusion)
    assert len(ref["lines"]) > 50
    got = _handover(scene, N, [0] * 3, diffusion)
    _assert_same(got, ref)
    _assert_handed_over(got, 48)


def test_eight_turns_with_blocks_shorter_than_the_tail_equal_one_device():
    """24 views in 8 blocks of 3: a block is shorter than `check`, so a turn's tail spans several blocks and is made of views it took over itself"""
    from line3d_amd.synth import make_scene
    N = 8
    scene = make_scene(24, 300, N, seed=9)
    turns, info = plan(C.CDLL(os.path.join(ROOT, "line3d_amd", "libline3d_amd.so")), scene_schedule(scene), 8)
    assert info["check"] > 3 and info["supported"] == 1
    # (the case in which turns r > 0 are deferred too: a package that is kept serves a second visit)
    assert any(t["deferred"] for t in turns[1:]) and not turns[-1]["deferred"]
    ref = _single(scene, N, False)
    assert len(ref["lines"]) > 20
    got = _handover(scene, N, [0] * 8, False)
    print("24 views in 8 turns: (views, visits) per turn", got["turn_views"], "deferred by the plan:", [t["deferred"] for t in turns])
    _assert_same(got, ref)
    assert got["turn_views"] == [((t["run1"] - t["run0"]) * (1 + t["deferred"]), 1 + t["deferred"]) for t in turns]


def test_turns_equal_one_device_on_scattered_non_mutual_neighbourhoods():
    """early-return views in mid-chain (cudawrapper.cu:877-878) couple views across the blocks: the slices go through the node object's store (the
    neighbourhoods come from the world points inside the library, so the plan is not rebuilt here: the views per turn show that no turn fell back)"""
    from line3d_amd.pipeline import load_scene_worldpoints
    from line3d_amd.synth import make_scene_scattered
    N = 8
    scene = make_scene_scattered(36, 260, seed=77)
    ref = _single(scene, N, False, loader=load_scene_worldpoints)
    assert len(ref["lines"]) > 5
    got = _handover(scene, N, [0, 0, 0], False, loader=load_scene_worldpoints)
    print("scattered scene: (views, visits) per turn", got["turn_views"])
    _assert_same(got, ref)
    # no fallback to plain mode 2 (that reports (36, 1) for every rank): every turn ran its own piece, the later ones from a package
    assert all(1 <= visits <= 2 for _, visits in got["turn_views"])
    assert got["turn_views"][0][0] >= 12 and all(n < 36 * visits for n, visits in got["turn_views"][1:]), got["turn_views"]


# ---- 2. the oracle's golden ----------------------------------------------------------------------------------------------------------------------
def test_handover_reproduces_the_config2_golden():
    """devices = [0, 0] on BASELINE configs[1] / configs[3]: the lines the ORACLE alone produced (tests/golden/config2_full.npz)"""
    from line3d_amd.pipeline import load_scene
    from line3d_amd.synth import make_scene
    g = np.load(os.path.join(ROOT, "tests", "golden", "config2_full.npz"))
    V, S, N, seed = (int(x) for x in g["shape"])
    scene = make_scene(V, S, N, seed=seed)
    l = _node_object(N, [0, 0])
    try:
        load_scene(l, scene)
        l.compute3Dmodel(False)
        edges, n_nodes = l.affinity()
        assert len(edges) == int(g["affinity_n"]) and n_nodes == int(g["n_nodes"])
        assert _sha(edges) == str(g["affinity_sha256"]), "affinity list differs from the oracle's"
        assert int(np.sum(l.chain_summary()["n_kept"], dtype=np.int64)) == int(g["kept_n"].sum())
        ids, id_off, pts, pt_off = g["plain_ids"], g["plain_id_off"], g["plain_pts"], g["plain_pt_off"]
        exp = [([(int(c), int(s)) for c, s in ids[id_off[k]:id_off[k + 1]]], [(p[:3], p[3:]) for p in pts[pt_off[k]:pt_off[k + 1]]])
               for k in range(len(id_off) - 1)]
        assert len(exp) > 2000
        assert assert_lines_equal(l.getResult(), exp, tol=1e-4) <= 1e-4
        _assert_handed_over(_turn_figures(l, 2), V)
    finally:
        l.close()


# ---- 3. / 4. the larger helix: the work and the capability ----------------------------------------------------------------------------------------
V_BIG, S_BIG, N_BIG, W_BIG = 256, 1000, 12, 8
_big = {}


def _big_runs():
    """the scene, the one chain, the hand-over run and the same object's run with the hand-over off, computed once for the two tests below"""
    if not _big:
        from line3d_amd.pipeline import load_scene
        from line3d_amd.synth import make_scene
        scene = make_scene(V_BIG, S_BIG, N_BIG, seed=20260)
        _big["scene"] = scene
        _big["single"] = _single(scene, N_BIG, False)
        l = _node_object(N_BIG, [0] * W_BIG)
        try:
            load_scene(l, scene)
            l.compute3Dmodel(False)
            on = _outcome(l)
            on.update(_turn_figures(l, W_BIG))
            l.set_turn_handover(False)
            l.reset()
            load_scene(l, scene)
            l.compute3Dmodel(False)
            off = _outcome(l)
            off.update(_turn_figures(l, W_BIG))
        finally:
            l.close()
        _big["on"], _big["off"] = on, off
    return _big["scene"], _big["single"], _big["on"], _big["off"]


def test_the_chain_work_is_not_w_fold():
    scene, single, on, off = _big_runs()
    _assert_same(on, single)
    _assert_same(off, single)
    views = scene_schedule(scene)
    assert len(views) == V_BIG
    reach, _ = reach_of(views)
    turns, info = plan(C.CDLL(os.path.join(ROOT, "line3d_amd", "libline3d_amd.so")), views, W_BIG)
    assert info["reach"] == reach and info["supported"] == 1
    total_views = sum(n for n, _ in on["turn_views"])
    deferred = sum(t["deferred"] for t in turns)
    print("views computed by all turns: %d of a bound of %d (one chain: %d, reach %d); deferred turns: %d; (views, visits) per turn: %s" %
          (total_views, 2 * (V_BIG + W_BIG * 2 * reach), V_BIG, reach, deferred, on["turn_views"]))
    # every turn runs its block and 2 reach views past it; a deferred turn runs that twice.  Deferring every turn but the last is the floor of the
    # design (two passes): 2 (V + (W - 1) 2 reach) views at the most
    assert total_views <= 2 * (V_BIG + W_BIG * 2 * reach)
    assert max(visits for _, visits in on["turn_views"]) <= 2
    assert [visits for _, visits in on["turn_views"]] == [1 + t["deferred"] for t in turns]
    assert [n for n, _ in on["turn_views"]] == [(t["run1"] - t["run0"]) * (1 + t["deferred"]) for t in turns]
    kept = single["kept"].astype(np.int64)
    total = int(kept.sum())
    print("records per turn:", on["turn_records"], "one chain:", total)
    for r in range(W_BIG):
        own = int(kept[(V_BIG * r) // W_BIG:(V_BIG * (r + 1)) // W_BIG].sum())
        assert own <= on["turn_records"][r] < total // 2, (r, own, on["turn_records"][r], total)
    # the same object with the hand-over off: plain mode 2, every turn computes the whole chain once
    assert off["turn_views"] == [(V_BIG, 1)] * W_BIG


def test_a_scene_past_the_capped_arena_fails_on_one_device_and_completes_with_the_handover():
    from line3d_amd.capi import L3DError
    from line3d_amd.pipeline import Line3D, load_scene
    scene, single, on, _ = _big_runs()
    total = int(single["kept"].astype(np.int64).sum())
    single_bytes, turn_bytes = total * BYTES_PER_RECORD, max(on["turn_records"]) * BYTES_PER_RECORD
    free_mb = (single_bytes + 2 * turn_bytes) // 2 >> 20
    print("arena of the one chain %d MB, of the largest turn %d MB, cap %d MB" % (single_bytes >> 20, turn_bytes >> 20, free_mb))
    assert math.ceil(2 * turn_bytes / 2**20) < free_mb < (single_bytes >> 20), "no gap between twice the largest turn's arena and the one chain's"

    # one device: the arena overflows and no regrow fits the room (tests/test_gpu_arena_regrow.py)
    l = Line3D("", matchingNeighbors=N_BIG, device=0)
    try:
        load_scene(l, scene)
        c = l.context()
        c.set_option("regrow_free_mb", int(free_mb))
        l.prepare()
        c.set_chain_capacities(0, total // 4)
        with pytest.raises(L3DError) as e:
            l.match_views()
        assert "error 3" in str(e.value), str(e.value)
    finally:
        l.close()

    # the same cap on every rank of the hand-over object: the model is the uncapped one
    got = _handover(scene, N_BIG, [0] * W_BIG, False, env=dict(L3D_REGROW_FREE_MB=int(free_mb)))
    _assert_same(got, single)
    assert got["turn_records"] == on["turn_records"] and got["turn_views"] == on["turn_views"]

    # the cap binds on what a hand-over turn allocates (first guess, regrow, the slices behind the records): with room for half of the SMALLEST
    # turn's records the first turn ends with NOMEM, named by its rank
    small_mb = max(1, min(on["turn_records"]) * BYTES_PER_RECORD // 2 >> 20)
    with pytest.raises(L3DError) as e:
        _handover(scene, N_BIG, [0] * W_BIG, False, env=dict(L3D_REGROW_FREE_MB=int(small_mb)))
    assert "error 3" in str(e.value) and "rank 0 (device 0)" in str(e.value) and "room for" in str(e.value), str(e.value)
    # ... and with room for the largest turn's records but not for twice as many, where the first guess of a turn (0.4 % of its pairs + 2^20 records)
    # is clipped to the room, the model is still the uncapped one: the arena allocated is the room, the records fit
    tight_mb = math.ceil(max(on["turn_records"]) * BYTES_PER_RECORD * 1.25 / 2**20) + 1
    assert tight_mb < free_mb
    got = _handover(scene, N_BIG, [0] * W_BIG, False, env=dict(L3D_REGROW_FREE_MB=int(tight_mb)))
    _assert_same(got, single)
    assert got["turn_records"] == on["turn_records"]


# ---- 5. switch hygiene ------------------------------------------------------------------------------------------------------------------------------
def test_the_switch_is_refused_where_it_has_no_meaning():
    from line3d_amd.capi import L3DError
    from line3d_amd.pipeline import Line3D
    l = Line3D("", matchingNeighbors=8, device=0)
    try:
        with pytest.raises(L3DError) as e:
            l.set_turn_handover(True)
        assert "node object" in str(e.value), str(e.value)
    finally:
        l.close()
    l = Line3D("", matchingNeighbors=8, devices=[0, 0])
    try:
        l.set_node_mode(2)
        l.set_turn_handover(True)
        l.set_turn_handover(False)
        with pytest.raises(L3DError):
            l.set_turn_handover(2)
        with pytest.raises(L3DError):        # (no run in turns yet)
            l.node_turn_views(0)
        with pytest.raises(L3DError):
            l.set_node_mode(3)
    finally:
        l.close()


def test_toggling_the_handover_off_again_gives_mode_2s_records():
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    N = 8
    scene = make_scene(32, 300, N, seed=9)
    plain = Line3D("", matchingNeighbors=N, devices=[0, 0])
    try:
        plain.set_node_mode(2)
        load_scene(plain, scene)
        plain.compute3Dmodel(False)
        expected = [plain.node_turn_records(r) for r in range(2)]
        lines = plain.getResult()
    finally:
        plain.close()
    l = _node_object(N, [0, 0])
    try:
        load_scene(l, scene)
        l.compute3Dmodel(False)
        assert_lines_equal(l.getResult(), lines, 0.0)
        _assert_handed_over(_turn_figures(l, 2), 32)
        l.set_turn_handover(False)
        l.reset()
        load_scene(l, scene)
        l.compute3Dmodel(False)
        assert_lines_equal(l.getResult(), lines, 0.0)
        assert [l.node_turn_records(r) for r in range(2)] == expected
        assert [l.node_turn_views(r) for r in range(2)] == [(32, 1)] * 2
    finally:
        l.close()


# ---- 6. a failure in the finish ---------------------------------------------------------------------------------------------------------------------
FAILURE_SCRIPT = r'''
import sys
from helpers import assert_lines_equal
from line3d_amd.capi import L3DError
from line3d_amd.pipeline import Line3D, load_scene
from line3d_amd.synth import make_scene
N = 8
scene = make_scene(32, 300, N, seed=9)
ref = Line3D("", matchingNeighbors=N, device=0)
load_scene(ref, scene)
ref.compute3Dmodel(False)
l = Line3D("", matchingNeighbors=N, devices=[0, 0])
l.set_node_mode(2)
l.set_turn_handover(True)
load_scene(l, scene)
try:
    l.compute3Dmodel(False)
    sys.exit("the injected exchange failure did not fail compute3Dmodel")
except L3DError as e:
    msg = str(e)
assert "rank 1 (device 0)" in msg, msg
l.reset()
load_scene(l, scene)
l.compute3Dmodel(False)
assert_lines_equal(l.getResult(), ref.getResult(), 0.0)
assert l.node_turn_records(0) > 0 and l.node_turn_records(1) > 0
assert all(l.node_turn_views(r)[0] > 0 for r in range(2)) and l.node_turn_views(1)[0] < 32
print("node failure ok:", msg)
'''


def test_exchange_failure_in_the_collective_finish_names_the_rank_and_reset_recovers():
    """L3D_NODE_FAIL_AT=1 (test-only option, read from rank 1's context): rank 1's first exchange returns 1 on the host -- a failing call, no device
    fault.  The turns exchange nothing; the exchanges are the collective finish's.  compute3Dmodel must return an error that names rank 1; after
    reset the same object computes the scene as one device does."""
    env = dict(os.environ, L3D_NODE_FAIL_AT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", FAILURE_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "node failure ok" in r.stdout
