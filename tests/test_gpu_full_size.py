"""Parity at BASELINE.json's full per-view sizes (2000 segments, 12 neighbours): the oracle is too slow for whole views
there (~25 s per view), so full size is covered by (i) the oracle on a slice of source segments of real full-size views,
bit for bit, (ii) properties that do not need the oracle: the three matching paths agree byte for byte, a pass is
idempotent, sharding over virtual ranks reproduces the unsharded lists, the diffusion of the full-size affinity matrix
equals the oracle's (the C oracle handles ~10^6 entries in seconds)."""
import hashlib

import numpy as np
import pytest

import l3d_oracle_pipeline as op
from helpers import literal_rule_lib

pytestmark = pytest.mark.gpu

V, S, N = 16, 2000, 12


@pytest.fixture(scope="module")
def full_scene():
    from line3d_amd.synth import make_scene
    return make_scene(V, S, N, seed=20260)


@pytest.fixture(scope="module")
def chain_run(full_scene):
    from line3d_amd.pipeline import Line3D, load_scene
    l = Line3D("", matchingNeighbors=N)
    l.keep_view_matches(True)
    load_scene(l, full_scene)
    l.prepare()
    l.match_views()
    lists = {v["id"]: l.view_matches(v["id"]) for v in full_scene.views}
    yield l, lists
    l.close()


def _digest(lists):
    h = hashlib.sha256()
    for vid in sorted(lists):
        h.update(lists[vid][0].tobytes())
        h.update(np.float32(lists[vid][1]).tobytes())
    return h.hexdigest()


def test_full_size_paths_agree_and_are_idempotent(full_scene, chain_run):
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd import distributed as l3dist
    l, lists = chain_run
    ref = _digest(lists)
    assert sum(len(m) for m, _ in lists.values()) > 300000
    l.match_views()                                                   # idempotent
    assert _digest({v["id"]: l.view_matches(v["id"]) for v in full_scene.views}) == ref
    for mode in ("sync", "native"):
        l2 = Line3D("", matchingNeighbors=N)
        l2.keep_view_matches(True)
        l2.set_sync_matching(mode == "sync")
        load_scene(l2, full_scene)
        l2.prepare()
        if mode == "native":
            l3dist.match_views_chain_native(l2, 0, 1, None, commit=True, n_segments=S, n_neighbors=N)
        else:
            l2.match_views()
        assert _digest({v["id"]: l2.view_matches(v["id"]) for v in full_scene.views}) == ref, mode
        l2.close()


def test_full_size_two_virtual_ranks_equal_unsharded(full_scene, chain_run):
    """Both ranks of a world-2 job on one GPU (recorded, then replayed through the native loop): rank 0's committed lists
    are the unsharded ones."""
    import torch
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.distributed import default_slot_records
    _l, lists = chain_run
    W = 2
    slot = default_slot_records(S, N, W)
    dev = torch.device("cuda", 0)
    ls = []
    for r in range(W):
        l = Line3D("", matchingNeighbors=N)
        l.keep_view_matches(True)
        load_scene(l, full_scene)
        l.prepare()
        ls.append(l)
    n_views, slot_bytes = [l.shard_open(r, W, slot) for r, l in enumerate(ls)][0]
    gathered = torch.zeros(n_views * W * slot_bytes, dtype=torch.uint8, device=dev)
    send = [torch.zeros(n_views * slot_bytes, dtype=torch.uint8, device=dev) for _ in range(W)]
    torch.cuda.synchronize()
    for k in range(n_views):
        for r, l in enumerate(ls):
            l.shard_enqueue(k, send[r].data_ptr() + k * slot_bytes, gathered.data_ptr())
        torch.cuda.synchronize()
        if ls[0].shard_view_verified(k):
            for r in range(W):
                gathered[(k * W + r) * slot_bytes:(k * W + r + 1) * slot_bytes].copy_(send[r][k * slot_bytes:(k + 1) * slot_bytes])
        torch.cuda.synchronize()
        for l in ls:
            l.shard_mark(k)
    for l in ls:
        l.shard_close(False)
    ls[0].shard_run(0, W, slot, "replay", gathered.data_ptr(), commit=True)
    assert _digest({v["id"]: ls[0].view_matches(v["id"]) for v in full_scene.views}) == _digest(lists)
    for l in ls:
        l.close()


def test_full_size_view_slice_against_oracle(full_scene, chain_run):
    """The first 160 source segments of a mid-chain full-size view (with its real reverse matches from earlier views)
    against the oracle, bit for bit (~3 s of oracle time)."""
    _l, lists = chain_run
    o = op.OracleLine3D(matching_neighbors=N, use_collinearity=False)
    for v in full_scene.views:
        o.add_image_fixed_sim(v["id"], v["width"], v["height"], v["segments"], v["K"], v["R"], v["t"], v["sims"])
    o.computation = True
    o.matched, o.potential = {}, {}
    o.find_visual_neighbors()
    o.transform_geometry()
    vid = 7
    # state after views 0..6: reverse matches of view 7 = the GPU lists of its earlier neighbours (already pinned to be
    # path independent above); feed them to the oracle as the existing matches, localized like view.cc:200-224
    for n in o.visual_neighbors[vid]:
        o._fundamental(vid, n)
    for a in range(vid):                                              # line3D.cc:875-881 after views 0..6
        for nb in o.visual_neighbors[a]:
            o.matched.setdefault(a, {})[nb] = True
            if a in o.visual_neighbors.get(nb, []):
                o.matched.setdefault(nb, {})[a] = True
    mv = o.marshal_view(vid)
    assert 0 < len(mv["tbm"]) < len(mv["l2g"])
    ex = []
    for a in range(vid):
        m, _ = lists[a]
        sel = m[m["camID2"] == vid]
        if len(sel) and a in mv["g2l"]:
            r = np.zeros(len(sel), dtype=op.MATCH_DTYPE)
            r["segID1"], r["segID2"], r["camID2"] = sel["segID2"], sel["segID1"], mv["g2l"][a]
            r["depths"] = sel["depths"][:, [2, 3, 0, 1]]
            ex.append(r)
    existing = np.concatenate(ex) if ex else np.zeros(0, dtype=op.MATCH_DTYPE)
    s1 = 160
    exp, _med, _ = op.compute_pairwise_matches(
        o.lib, mv["src_segs"], mv["RtKinv_src"], mv["C_src"], mv["tgt_segs"], mv["offsets"], mv["F"], mv["RtKinv"],
        mv["centers"], mv["P"], mv["tbm"], existing, mv["l2g"], mv["k_upper"], mv["k_lower"], 3.5, 10.0, mv["spatial_k"],
        seg_range=(0, s1), want_stats=True)
    got = lists[vid][0]
    got = got[got["segID1"] < s1]
    assert len(exp) > 1000 and got.tobytes() == exp.tobytes()


def test_full_size_diffusion_equals_oracle(chain_run, oracle_lib):
    """Config 4: replicator-dynamics diffusion of the full-size affinity matrix (GPU) against the C oracle, bit for bit."""
    from line3d_amd import capi
    l, _ = chain_run
    l.finish(False)
    A, n_nodes = l.affinity()[:2]
    assert len(A) > 100000
    ctx = capi.Context(0)
    got = ctx.replicator_dynamics_diffusion(A, n_nodes)
    exp = op.rdd(oracle_lib, A, n_nodes)
    assert got.tobytes() == exp.tobytes()
    ctx.close()


def test_full_size_affinity_fill_device_equals_literal_host_rule(chain_run, full_scene, gpu_ctx, monkeypatch):
    """The affinity fill runs on the device (l3d_affinity_fill: per-target "expanded" bits instead of the reference's `used` maps),
    on tables that never left it.  Cross-check at full size: (i) the device path with 5-target passes (groups and flattened entries
    straddling passes), one launch per view (the schedule of scenes with one-way records), other thread counts of the host stages,
    and matchViews with host bookkeeping (host-built tables uploaded to the same fill) give the same list and the same lines;
    (ii) the candidate enumeration with the reference's `used` rule applied LITERALLY on one thread (tests/cpp/literal_used_rule.c)
    over the resident tables, weighted through the similarity seam call, gives the same edge list bit for bit."""
    import ctypes as C
    l, _ = chain_run
    out = {}
    variants = {"device": {}, "device, 5-target passes": {"L3D_AFF_CHUNK": 5}, "device, one launch per view": {"L3D_AFF_PER_VIEW": 1},
                "device, 5 host threads": {"L3D_HOST_THREADS": 5}}
    lctx = l.context()
    for name, env in variants.items():
        for k in ("L3D_AFF_CHUNK", "L3D_HOST_THREADS", "L3D_AFF_PER_VIEW"):
            lctx.set_option(k, 0)
        for k, v in env.items():
            lctx.set_option(k, v)
        for diffusion in (False, True):
            l.finish(diffusion)
            A, n_nodes = l.affinity()[:2]
            lines = l.getResult()
            sig = hashlib.sha256(np.ascontiguousarray(A).tobytes())
            for seg2, seg3 in lines:
                sig.update(np.asarray(seg2, dtype=np.int64).tobytes())
                sig.update(np.asarray([np.concatenate(p) for p in seg3], dtype=np.float64).tobytes())
            out[(name, diffusion)] = (len(A), n_nodes, len(lines), sig.hexdigest())
    for k in ("L3D_AFF_CHUNK", "L3D_HOST_THREADS", "L3D_AFF_PER_VIEW"):
        lctx.set_option(k, 0)
    for diffusion in (False, True):
        assert out[("device", diffusion)][0] > 100000 and out[("device", diffusion)][2] > 100
        for name in variants:
            assert out[(name, diffusion)] == out[("device", diffusion)], (name, diffusion)
    # host bookkeeping (per-view delivery, host lists, host-packed tables): the same list
    from line3d_amd.pipeline import Line3D, load_scene
    monkeypatch.setenv("L3D_HOST_BOOKKEEPING", "1")
    l2 = Line3D("", matchingNeighbors=N, crosschecks=True)          # (the switch only exists in the cross-check build)
    assert l2.context().get_option("crosschecks") == 1 and l.context().get_option("crosschecks") == 0
    load_scene(l2, full_scene)
    l2.compute3Dmodel(False)
    assert l2.resident_products() is None
    A2 = l2.affinity()[0]
    monkeypatch.delenv("L3D_HOST_BOOKKEEPING")
    l.finish(False)
    A, n_nodes = l.affinity()[:2]
    assert A2.tobytes() == A.tobytes()
    l2.close()

    # ---- the literal rule over the resident tables
    pr = l.resident_products()
    seg_base, nd = pr["seg_base"], int(pr["seg_base"][-1])
    has = pr["best"]["segID1"] != 0xffffffff
    best = np.where(has, np.cumsum(has) - 1, -1).astype(np.int32)                # hypotheses are numbered in dense order
    hyp_dense = np.nonzero(has)[0].astype(np.int32)
    nh = len(hyp_dense)
    assert nh == len(pr["hyp"]) > 10000
    coll = gpu_ctx.compute_collinearity_batch([v["segments"] for v in full_scene.views])     # (the call prepare() makes)
    ci, cj, cw = [], [], []
    for vi, (i, j, w) in enumerate(coll):
        b = int(seg_base[vi])
        ci += [b + i, b + j]; cj += [b + j, b + i]; cw += [w, w]
    ci, cj, cw = np.concatenate(ci), np.concatenate(cj), np.concatenate(cw)
    order = np.lexsort((cj, ci))
    ci, cj, cw = ci[order], cj[order].astype(np.int32), cw[order].astype(np.float32)
    coll_start = np.zeros(nd + 1, np.int64)
    np.add.at(coll_start, ci + 1, 1)
    coll_start = np.cumsum(coll_start)
    lib = literal_rule_lib()
    item_t = np.dtype([("a", "<i4"), ("b", "<i4"), ("kind", "<i4"), ("cw", "<f4")])
    pot_start, pot_tgt = np.ascontiguousarray(pr["pot_start"]), np.ascontiguousarray(pr["pot_tgt"])
    args = [C.c_int32(nd), C.c_int32(nh), hyp_dense.ctypes.data_as(C.c_void_p), best.ctypes.data_as(C.c_void_p), pot_start.ctypes.data_as(C.c_void_p),
            pot_tgt.ctypes.data_as(C.c_void_p), coll_start.ctypes.data_as(C.c_void_p), cj.ctypes.data_as(C.c_void_p), cw.ctypes.data_as(C.c_void_p)]
    n_items = lib.literal_used_rule(*args, None, C.c_int64(0))
    items = np.zeros(n_items, item_t)
    assert lib.literal_used_rule(*args, items.ctypes.data_as(C.c_void_p), C.c_int64(n_items)) == n_items > 100000
    pairs = np.stack([items["a"], items["b"]], 1).astype(np.int32)
    sim = gpu_ctx.similarity_coll3D_batch(pr["hyp"], pairs, 10.0)                 # line3D.cc:1600-1681 (seam call, pinned to the oracle elsewhere)
    sc = pr["score"].astype(np.float32)
    ssum = (sc[items["a"]] + sc[items["b"]]).astype(np.float32)
    half = np.float32(0.5)
    w01 = ((half * ssum).astype(np.float32) * sim).astype(np.float32)            # :1014, :1085
    w2 = (((items["cw"] * half).astype(np.float32) * ssum).astype(np.float32) * sim).astype(np.float32)   # :1163
    w = np.where(items["kind"] == 2, w2, w01)
    keep = w > np.where(items["kind"] == 0, np.float32(0.25), np.float32(0.01))
    ka, kb, kw = items["a"][keep], items["b"][keep], w[keep]
    touch = np.stack([ka, kb], 1).ravel()                                         # first-touch node numbering: source before target, in order
    _, first = np.unique(touch, return_index=True)
    node_of = np.full(nh, -1, np.int64)
    node_of[touch[np.sort(first)]] = np.arange(len(first))
    exp = np.zeros(2 * len(ka), dtype=A.dtype)
    exp["i"][0::2], exp["j"][0::2], exp["w"][0::2] = node_of[ka], node_of[kb], kw
    exp["i"][1::2], exp["j"][1::2], exp["w"][1::2] = node_of[kb], node_of[ka], kw
    assert len(first) == n_nodes
    assert exp.tobytes() == A.tobytes()


def test_near_maximum_segments_per_view():
    """12 000 segments per view (the bit rows hold at most 16 384 targets per camera): the resident chain and the per-view
    seam path agree byte for byte, and the first source segments of the first view equal the oracle."""
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    Vb, Sb, Nb = 6, 12000, 6
    sc = make_scene(Vb, Sb, Nb, seed=77)
    digests, first = [], None
    for sync in (False, True):
        l = Line3D("", matchingNeighbors=Nb, useCollinearity=False)
        l.keep_view_matches(True)
        l.set_sync_matching(sync)
        load_scene(l, sc)
        l.prepare()
        l.match_views()
        lists = {v["id"]: l.view_matches(v["id"]) for v in sc.views}
        digests.append(_digest(lists))
        if first is None:
            first = lists[0][0].copy()
        l.close()
    assert digests[0] == digests[1]
    assert len(first) > 10000
    o = op.OracleLine3D(matching_neighbors=Nb, use_collinearity=False)
    for v in sc.views:
        o.add_image_fixed_sim(v["id"], v["width"], v["height"], v["segments"], v["K"], v["R"], v["t"], v["sims"])
    o.computation = True
    o.matched, o.potential = {}, {}
    o.find_visual_neighbors()
    o.transform_geometry()
    for n in o.visual_neighbors[0]:
        o._fundamental(0, n)
    mv = o.marshal_view(0)
    assert len(mv["tbm"]) == len(mv["l2g"]) == 3
    s1 = 40
    exp, _med, _ = op.compute_pairwise_matches(
        o.lib, mv["src_segs"], mv["RtKinv_src"], mv["C_src"], mv["tgt_segs"], mv["offsets"], mv["F"], mv["RtKinv"],
        mv["centers"], mv["P"], mv["tbm"], np.zeros(0, dtype=op.MATCH_DTYPE), mv["l2g"], mv["k_upper"], mv["k_lower"], 3.5, 10.0,
        mv["spatial_k"], seg_range=(0, s1), want_stats=True)
    got = first[first["segID1"] < s1]
    assert len(exp) > 50 and got.tobytes() == exp.tobytes()
