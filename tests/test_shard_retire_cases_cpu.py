"""The retirement schedule of the segment-sharded run's ring of gathered blocks (RetireSchedule in line3d_amd/csrc/l3d_shard_rule.hpp)
through its host-only hook l3d_test_shard_retire: the ring's safety invariant stated on every view of every case, and the hook held to
tests/shard_rule_model.py step for step.  No device: tests/test_gpu_pipeline_parity.py (ring_of_gathered_slots) and tests/test_gpu_partition.py run the
schedule on whole scenes.

The invariant.  View k's exchange overwrites block k % ring, where view k - ring lived: that view must be retired AND the retirement waited for by the
chain's stream when the exchange is enqueued.  A view reads at most `window` views back, so views from k - window on must still be in the ring.  After
the final flush every view is retired and nothing is outstanding -- also in a partitioned ring that never wraps."""
import functools
import itertools

import shard_rule_model as sm

BATCH = sm.RETIRE_BATCH


@functools.lru_cache(maxsize=None)
def _grid():
    """(arguments, the hook's answer, the branches the case takes)"""
    from line3d_amd import capi
    out = []
    for window in (1, 2, 5):
        for n, apart, partition in itertools.product(range(1, window + 18 + 2 * BATCH + 3 + 1), (False, True), (False, True)):
            args = (n, window, 1, partition, apart)      # (slot_ring 1: a ring wherever the views outnumber it)
            got = capi.shard_retire(*args)
            tags = {"window %d" % window, "apart" if apart else "same stream", "partitioned" if partition else "whole scene"}
            if not got["ring_mode"]:
                tags.add("no ring")
            else:
                tags.add("ring wraps" if n > got["ring"] else "ring never wraps")
                in_loop = [b for b in got["batches"] if b[2] < n]
                tags.add("%s batches on the way" % ("no" if not in_loop else "one" if len(in_loop) == 1 else "two or more"))
                flush = [b for b in got["batches"] if b[2] == n]
                if flush and flush[-1][1] < BATCH:
                    tags.add("ragged flush")
                if len(flush) > 1:
                    tags.add("flush of several batches")
                if any(b[3] for b in got["batches"]):
                    tags.add("waited before a batch")
                if apart and any(w > (got["waited_at"][k - 1] if k else 0) and not any(b[2] == k for b in got["batches"]) for k, w in enumerate(got["waited_at"])):
                    tags.add("waited at the overwriting view")
            out.append((args, got, tags))
    return out


def test_the_grid_reaches_every_branch_of_the_schedule():
    seen = set().union(*(t for _, _, t in _grid()))
    assert seen >= {"window 1", "window 2", "window 5", "apart", "same stream", "partitioned", "whole scene", "no ring", "ring wraps", "ring never wraps",
                    "no batches on the way", "one batches on the way", "two or more batches on the way", "ragged flush", "flush of several batches", "waited before a batch",
                    "waited at the overwriting view"}, seen
    for (n, window, _, partition, _), got, tags in _grid():
        assert got["ring_mode"] == (partition or n > window + 18), (n, window, partition)
        assert got["ring"] == (min(window + 18, n) if got["ring_mode"] else n)
        if "no ring" in tags:
            assert got["batches"] == [] and got["retired"] == 0
        if "ring never wraps" in tags:      # (partitioned only: no block is ever overwritten, whatever is left is retired by the flush)
            assert partition and got["ring"] == n and got["retired"] == n and not got["outstanding"]


def test_the_ring_invariant_on_every_view():
    for (n, window, _, _, apart), got, tags in _grid():
        if not got["ring_mode"]:
            continue
        ring = got["ring"]
        for k in range(n):
            retired, waited = got["retired_at"][k], got["waited_at"][k]
            # 1. the block view k's exchange overwrites is retired, and that retirement has been waited for
            if k >= ring:
                assert retired > k - ring and waited > k - ring, (n, window, apart, k, retired, waited)
            # 2. nothing is retired that view k or a later one still reads
            assert retired <= max(0, k - window), (n, window, apart, k, retired)
            assert 0 <= waited <= retired and (apart or waited == retired)
            assert retired >= (got["retired_at"][k - 1] if k else 0) and waited >= (got["waited_at"][k - 1] if k else 0)
        # 3. batches are contiguous, at most 16 long, ascending -- and a batch is enqueued behind the exchanges of its views
        at = 0
        for i, (first, count, when, waited_before) in enumerate(got["batches"]):
            assert first == at and 1 <= count <= BATCH and (when == n or first + count <= when - window), (n, window, got["batches"])
            assert i == 0 or when >= got["batches"][i - 1][2]
            # (the chain waits for the batch before this one first, unless a view in between -- the first that overwrites a block of it -- has done so)
            if i:
                first_p, _, when_p, _ = got["batches"][i - 1]
                passed = min(when - 1, n - 1) >= max(when_p, first_p + ring)
            assert bool(waited_before) == bool(apart and i > 0 and not passed), (n, window, apart, got["batches"])
            at += count
        # 4. after the final flush
        assert at == n and got["retired"] == n and got["waited"] == n and not got["outstanding"], (n, window, apart, got)


def test_hook_equals_model_step_for_step():
    for args, got, _ in _grid():
        assert got == sm.retire_run(*args), args


def test_options_that_keep_every_block():
    from line3d_amd import capi
    assert not capi.shard_retire(60, 1, 0, False, True)["ring_mode"] and capi.shard_retire(60, 1, 0, True, True)["ring_mode"]
    # (the budget decides: 60 blocks of one byte are far below it)
    assert not capi.shard_retire(60, 1, -1, False, True)["ring_mode"]


def test_literal_schedule():
    """window 2, 60 views, side stream: ring 20; the first batch goes at view 18 (16 views in front of 18 - 2) and is waited for at view 20, which overwrites
    view 0's block; the second goes at view 34 and is waited for at 36, the third at 50 and 52; the flush retires [48, 60).  34 views: the flush takes two
    batches, and the chain waits for the first before the second"""
    from line3d_amd import capi
    got = capi.shard_retire(60, 2, 1, False, True)
    assert got["ring"] == 20 and got["batches"] == [(0, 16, 18, 0), (16, 16, 34, 0), (32, 16, 50, 0), (48, 12, 60, 0)]
    assert capi.shard_retire(34, 2, 1, False, True)["batches"] == [(0, 16, 18, 0), (16, 16, 34, 0), (32, 2, 34, 1)]
    assert got["retired_at"][17:21] == [0, 16, 16, 16] and got["waited_at"][17:21] == [0, 0, 0, 16]
    assert got["retired_at"][33:37] == [16, 32, 32, 32] and got["waited_at"][33:37] == [16, 16, 16, 32]
    same = capi.shard_retire(60, 2, 1, False, False)
    assert same["batches"] == [(0, 16, 18, 0), (16, 16, 34, 0), (32, 16, 50, 0), (48, 12, 60, 0)] and same["waited_at"] == same["retired_at"] == got["retired_at"]
