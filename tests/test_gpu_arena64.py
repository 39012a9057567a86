"""The kept arena indexed with 64 bits (ChainResult.kept_base, DESIGN.md sections 3 and 10): one single-GPU resident chain keeps more than 2^32
matches, and the views whose slices lie past record 2^32 come out byte for byte as one rank of the partitioned job computes them
(l3d_shard_chain_partition, the rank's share below 2^32 records) -- both decompositions are exact, so each is the other's
reference.  The scene is BASELINE configs[4]'s generator (synth.make_scene with turn_period left at its default) at the view count whose
chain keeps 4.4-4.8e9 records.  Reference behaviour: line3D.cc:620-648 (matchViews), :834-884 (what performMatching leaves behind); the reference
streams its match store to disk (view.cc:150-224) and has no such limit."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, S, N = 448, 4000, 24              # 4.53e9 kept records (640 views: 5.2e9 by view 495), profiles/arena64_sizing.txt
ARENA = 4_600_000_000               # records of the single chain's arena, given up front: no regrow
BLOCK_KEYS = 1 << 28                # the products' blocks of transients at a fixed size (by default they grow with the free HBM): the peak is what the test needs
PEAK_GB = 257.0                     # peak HBM in use, sampled on an MI355X (profiles/arena64_sizing.txt); the test skips below this + 10 % free
R, W = 1, 2                         # the rank of the partitioned job whose share is compared (below 2^32 records; its block holds the views past 2^32)


def _free_hbm():
    hip = C.CDLL("libamdhip64.so")
    f, t = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value, t.value


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _product_digests(prod, views):
    """per view: sha256 of its rows of potential_correspondences_ (row lengths and targets) and of its best matches"""
    sb, ps, pt, best = prod["seg_base"], prod["pot_start"], prod["pot_tgt"], prod["best"]
    out = {}
    for v in views:
        d0, d1 = int(sb[v]), int(sb[v + 1])
        out[v] = (_digest(np.diff(ps[d0:d1 + 1]), pt[ps[d0]:ps[d1]]), _digest(best[d0:d1]))
    return out


def test_single_chain_arena_past_2_32_records_equals_the_partitioned_job():
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene

    free, total = _free_hbm()
    peak, stop = [total - free], threading.Event()

    def poll():                     # (the HBM in use, sampled: printed for the record)
        while not stop.wait(0.05):
            f, t = _free_hbm()
            peak[0] = max(peak[0], t - f)
    if free < PEAK_GB * 1.1 * 2**30:
        pytest.skip("needs %.0f GB of free HBM (measured peak %.0f GB + 10 %%), the card has %.1f of %.1f GB free" % (PEAK_GB * 1.1, PEAK_GB, free / 2**30, total / 2**30))
    scene = make_scene(V, S, N)
    assert scene.params["turn_period"] == 0
    poller = threading.Thread(target=poll, daemon=True)
    poller.start()

    try:
        # ---- the one chain, its arena given up front
        l = Line3D("", matchingNeighbors=N)
        try:
            load_scene(l, scene)
            l.context().set_option("reserve_hint", 0)       # (no finish here: nothing reserved for it)
            l.context().set_option("check_pot", 0)          # (the host construction of the whole table would need 2 x 150 GB of host memory: the partitioned job is the check)
            l.context().set_option("prod_block_keys", BLOCK_KEYS)
            l.prepare()
            l.context().set_chain_capacities(0, ARENA)
            l.match_views()
            assert l.match_path() == 0
            summ = l.chain_summary()
            assert len(summ) == V
            n_kept = summ["n_kept"].astype(np.int64)
            base = np.concatenate([[0], np.cumsum(n_kept)])
            # a scene too small for the point of this test must not pass it
            assert base[-1] > 2**32, "%d kept records: not past 2^32" % base[-1]
            assert int(l.stats()["kept"]) == base[-1]
            # the views whose slices begin at or cross record 2^32, in full; the others by a sample
            past = [k for k in range(V) if n_kept[k] > 0 and base[k + 1] > 2**32]
            assert past and base[past[0]] < 2**32 <= base[past[0] + 1]
            sample = sorted(set(range(V * R // W, past[0], 11)) | {past[0] - 1})
            views = sample + past
            ctx = l.context()
            ref_lists = {}
            for k in views:
                m = ctx.chain_kept_list(k)
                assert len(m) == n_kept[k]
                ref_lists[k] = _digest(m)
            prod = l.resident_products()
            ref_prod = _product_digests(prod, views)
            del prod
        finally:
            l.close()
        peak_single = peak[0]

        # ---- the same scene as a partitioned job: rank R of W alone at world 1 (l3d_shard_chain_partition through the virtual-rank options, as
        # scripts/run_rank_share.py runs one rank's share): the segment-sharded chain over all views, this rank's keep set retired into its arena,
        # its rows of the products.  Its block holds the views past record 2^32; its share stays below 2^32 records
        p = Line3D("", matchingNeighbors=N)
        try:
            load_scene(p, scene)
            c = p.context()
            c.set_option("reserve_hint", 0)
            c.set_option("check_pot", 0)
            c.set_option("prod_block_keys", BLOCK_KEYS)
            p.prepare()
            c.set_option("L3D_PART_VRANK", R); c.set_option("L3D_PART_VWORLD", W)
            b0, b1 = V * R // W, V * (R + 1) // W
            share = int(base[min(V, b1 + N + 2)] - base[max(0, b0 - N - 2)])        # (its block and 2 x reach either side)
            assert share < 2**32
            c.set_chain_capacities(int(summ["n_candidates"].max() * 1.1) + 65536, int(share * 1.01) + 1000000)
            p.shard_run(0, 1, int(n_kept.max() * 1.05) + 65536, "local", None, commit="partition")
            info = p.partition_info()
            assert info["own"][0] <= past[0] and info["own"][1] == V
            held = info["held"]
            assert base[held[1]] - base[held[0]] < 2**32, "the rank holds %d records" % (base[held[1]] - base[held[0]])
            views = [k for k in views if info["own"][0] <= k < info["own"][1]]
            assert len(views) > len(past)
            got_lists = {k: _digest(c.chain_kept_list(k)) for k in views}
            got_prod = _product_digests(p.resident_products(), views)
        finally:
            p.close()
    finally:
        stop.set()
        poller.join()
    print("arena64: %d kept records, %d views past record 2^32, peak HBM in use %.1f GB (single chain %.1f GB)" % (base[-1], len(past), peak[0] / 2**30, peak_single / 2**30))
    assert sorted(got_lists) == sorted(views)
    for k in views:
        assert got_lists[k] == ref_lists[k], "view %d (records %d..%d): kept list" % (k, base[k], base[k + 1])
        assert got_prod[k][0] == ref_prod[k][0], "view %d: rows of potential_correspondences_" % k
        assert got_prod[k][1] == ref_prod[k][1], "view %d: best matches" % k
