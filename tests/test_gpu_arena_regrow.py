"""The regrow of the single-GPU chain's kept arena near the top of HBM: the old arena stays allocated while its used part is
copied, so the new one must fit BESIDE it.  A test-only cap on the free HBM the regrow sees (option regrow_free_mb) stands in for a full card:
  * room for the whole run, but less than the regrow asks for: the arena is cut to what fits, every view gets through, and the kept lists and products
    equal an unconstrained run's byte for byte;
  * no room for the view that overflowed: the chain fails with L3D_ERR_NOMEM and the sizes (no blind doubling, no endless restarts).
Reference behaviour: line3D.cc:620-648 (matchViews) -- the arena is this port's own store, the reference spills to disk (view.cc:150-224)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, S, N = 64, 2000, 12
# what the regrow counts per arena record with resident products and without early transposes (prod_early = 0): the record, its side word, 8 B of
# the products' table; and the HBM it keeps back for the products' smallest transient blocks (2^28 key slots x 24 B) + 1 GB (l3d_chain.hip)
PER_REC, RESERVE_MB = 32 + 4 + 8, 6144 + 1024


def _run(scene, arena=0, free_mb=0):
    from line3d_amd.pipeline import Line3D, load_scene
    l = Line3D("", matchingNeighbors=N)
    try:
        load_scene(l, scene)
        c = l.context()
        c.set_option("prod_early", 0)
        if free_mb:
            c.set_option("regrow_free_mb", free_mb)
        l.prepare()
        if arena:
            c.set_chain_capacities(0, arena)
        l.match_views()
        assert l.match_path() == 0
        summ = l.chain_summary()
        lists = [c.chain_kept_list(k).tobytes() for k in range(len(summ))]
        prod = l.resident_products()
        return summ["n_kept"].astype(np.int64), lists, prod
    finally:
        l.close()


def test_regrow_cut_to_what_fits_and_nomem_when_the_view_does_not_fit():
    from line3d_amd.capi import L3DError
    from line3d_amd.synth import make_scene
    scene = make_scene(V, S, N, seed=20260)
    n_kept, lists, prod = _run(scene)
    total = int(n_kept.sum())
    assert total > 1_500_000

    # room for every record + 100 k beside the old arena: the regrow from 0.9 x total asks for more (the projection, x 1.15) and is cut to that room
    room = total + 100_000
    free_mb = RESERVE_MB + math.ceil(room * PER_REC / 2**20)
    got_kept, got_lists, got_prod = _run(scene, arena=int(total * 0.9), free_mb=free_mb)
    assert np.array_equal(got_kept, n_kept)
    assert got_lists == lists
    for key in ("pot_start", "pot_tgt", "best"):
        assert got_prod[key].tobytes() == prod[key].tobytes(), key

    # no room at all beside the old arena: the first overflow ends the chain with NOMEM and the sizes
    with pytest.raises(L3DError) as e:
        _run(scene, arena=total // 4, free_mb=RESERVE_MB - 1)
    msg = str(e.value)
    assert "error 3" in msg and "does not fit beside it" in msg and "records in use" in msg, msg
