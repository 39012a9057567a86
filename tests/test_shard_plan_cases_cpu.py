"""The sizing rules of the segment-sharded run (l3d_shard_rule.hpp in line3d_amd/csrc) through their host-only hook
l3d_test_shard_plan, held to tests/shard_rule_model.py on grids that reach every branch of every rule at the smallest numbers that do, and to literal
values.  No device: the sharded-run tests of tests/test_gpu_pipeline_parity.py, test_gpu_partition.py and test_gpu_arena64.py run the rules on whole scenes."""
import functools
import itertools

import shard_rule_model as sm

GB8 = 8 << 30
CAMS_MIN = 64


def _capi():
    from line3d_amd import capi
    return capi


# ---- the layout of a slot
@functools.lru_cache(maxsize=None)
def _geometry_grid():
    out = []
    for world, maxS, records, maxN in itertools.product((1, 3), (1, 7, 8), (CAMS_MIN - 1, CAMS_MIN, 1), (2, 5)):
        args = (maxS, maxN, world, records, CAMS_MIN, 9)
        m = sm.slot_geometry(*args)
        tags = {"world %d" % world, "maxS %d" % maxS, "side array and run table" if m["cam_off"] else "no side array"}
        tags.add("range divides evenly" if maxS % world == 0 else "range rounds up")
        out.append((args, m, tags))
    return out


def test_geometry_grid_reaches_every_shape():
    seen = set().union(*(t for _, _, t in _geometry_grid()))
    # (a slot that carries side words always carries a run table: "side array only" is no shape slot_geometry produces)
    assert seen >= {"world 1", "world 3", "maxS 1", "maxS 7", "maxS 8", "no side array", "side array and run table", "range divides evenly", "range rounds up"}, seen
    for args, m, _ in _geometry_grid():
        # (the best positions follow the depth pairs directly: ints behind float2s, 8-aligned -- the layout the kernels have always read; every other array starts on 32)
        assert all(m[k] % 32 == 0 for k in ("best_off", "rec_off", "cam_off", "rt_off")) and m["bpos_off"] % 8 == 0 and m["slot_bytes"] % 256 == 0 and m["stage_bytes"] % 256 == 0, (args, m)
        assert m["best_off"] < m["bpos_off"] < m["rec_off"] and bool(m["cam_off"]) == bool(m["rt_off"]) == (args[3] >= CAMS_MIN)
        assert m["bpos_off"] - m["best_off"] == 8 * m["seg_cap"] and m["rec_off"] - m["bpos_off"] >= 4 * m["seg_cap"]
        if m["cam_off"]:
            assert m["rec_off"] + 32 * args[3] <= m["cam_off"] and m["cam_off"] + 4 * args[3] <= m["rt_off"] and m["rt_off"] + 4 * (args[1] + 1) * m["seg_cap"] <= m["slot_bytes"]
        else:
            assert m["rec_off"] + 32 * args[3] <= m["slot_bytes"]
        assert m["seg_cap"] * args[2] >= args[0] + args[2] - 1          # (every rank's range fits, one segment to spare)


def test_geometry_hook_equals_model_and_literals():
    capi = _capi()
    for args, m, _ in _geometry_grid():
        assert capi.shard_slot_geometry(*args) == m, args
    got = capi.shard_slot_geometry(7, 2, 1, 63, 64, 9)         # 8 segments: pairs 64 B, positions 32 B, 63 records
    assert got == dict(seg_cap=8, best_off=32, bpos_off=96, rec_off=128, cam_off=0, rt_off=0, slot_bytes=2304, stage_bytes=2304, ring=9, max_n=2)
    got = capi.shard_slot_geometry(7, 2, 1, 64, 64, 9)         # + 64 side words at 2176, a run table of 3 x 8 ints at 2432
    assert got == dict(seg_cap=8, best_off=32, bpos_off=96, rec_off=128, cam_off=2176, rt_off=2432, slot_bytes=2560, stage_bytes=2304, ring=9, max_n=2)
    got = capi.shard_slot_geometry(8, 2, 3, 64, 64, 0)         # three ranks: 4 segments each; positions end at 80, records start at 96
    assert got == dict(seg_cap=4, best_off=32, bpos_off=64, rec_off=96, cam_off=2144, rt_off=2400, slot_bytes=2560, stage_bytes=6400, ring=1, max_n=2)


# ---- ring or every block
@functools.lru_cache(maxsize=None)
def _ring_grid():
    out = []
    for window, n in itertools.chain(((1, n) for n in (0, 1, 19, 20, 21, 40)), ((3, n) for n in (21, 22, 23))):
        blocks = sorted({1, GB8 // max(1, n), GB8 // max(1, n) + 1})
        for block, slot_ring, partition, commit in itertools.product(blocks, (-1, 0, 1), (False, True), (False, True)):
            if partition and commit:
                continue                     # (refused by l3d_shard_chain_run before the plan is made)
            args = (n, window, block, slot_ring, partition, commit)
            m = sm.ring_plan(*args)
            wraps = n > window + 18
            if partition:
                tag = "partition, ring wraps" if wraps else "partition, ring never wraps"
            elif commit:
                tag = "commits on the host"
            elif slot_ring == 0:
                tag = "ring off by option"
            elif not wraps:
                tag = "no more views than the ring"
            elif slot_ring > 0:
                tag = "ring forced"
            else:
                tag = "over the budget" if n * block > GB8 else "within the budget"
            out.append((args, m, {tag, "window %d" % window}))
    return out


def test_ring_grid_reaches_every_branch():
    seen = set().union(*(t for _, _, t in _ring_grid()))
    assert seen >= {"partition, ring wraps", "partition, ring never wraps", "commits on the host", "ring off by option", "no more views than the ring", "ring forced",
                    "over the budget", "within the budget", "window 1", "window 3"}, seen
    for (n, window, block, slot_ring, partition, commit), m, tags in _ring_grid():
        ring_on = bool(tags & {"partition, ring wraps", "partition, ring never wraps", "ring forced", "over the budget"})
        assert m["ring_mode"] == ring_on, (n, window, block, slot_ring, partition, commit)
        if not ring_on:
            assert m["ring_views"] == max(1, n) and m["send_ring"] == n
        elif "partition, ring never wraps" in tags:
            assert m["ring_views"] == m["send_ring"] == max(1, n)
        else:
            assert m["ring_views"] == m["send_ring"] == window + 18 < n
    # either side of window + 18 at window 1, and of 8 GB at 21 views
    capi = _capi()
    assert [capi.shard_ring_plan(n, 1, 1, 1, False, False)["ring_mode"] for n in (19, 20, 21)] == [False, True, True]
    assert capi.shard_ring_plan(20, 1, 1, 1, False, False) == dict(ring_mode=True, ring_views=19, send_ring=19)
    assert [capi.shard_ring_plan(21, 1, b, -1, False, False)["ring_mode"] for b in (GB8 // 21, GB8 // 21 + 1)] == [False, True]
    assert capi.shard_ring_plan(5, 1, 1, 0, True, False) == dict(ring_mode=True, ring_views=5, send_ring=5)
    assert capi.shard_ring_plan(0, 1, 1, -1, False, False) == dict(ring_mode=False, ring_views=1, send_ring=0)


def test_ring_hook_equals_model():
    capi = _capi()
    for args, m, _ in _ring_grid():
        assert capi.shard_ring_plan(*args) == m, args


# ---- the first guess of the compact arena
PAIRS = 3.3e9               # (0.004 of it: 13.2 M records; with arena_guess 8: 26.4 M)
M1 = 1048576


@functools.lru_cache(maxsize=None)
def _guess_grid():
    out = []
    base = int(PAIRS * 0.004) + M1
    want8 = int(PAIRS * 0.001 * 8) + M1
    frees = (sm.FREE_UNKNOWN, int(20_000_000 * 40 / 0.35), 1 << 40)      # unknown | 35 % of it holds 20 M records: between base and want8 | plenty
    rooms = (0, 256, 1 << 20)                                             # none | 256 MB = 7.4 M records: binds | 1 TB: never binds
    for world in (1, 2):
        for test_cap, seen, guess, free, mb in itertools.product((0, 5_000_000), (0, 40_000_000 * world), (4, 8), frees, rooms):
            for partition, kept, part_seen in ((False, 0, 0), (True, 0, 0), (True, 3, 0), (True, 10, 0), (True, 3, 1 << 30)):
                args = (PAIRS, world, test_cap, seen, guess, free, mb, partition, kept, 10, part_seen)
                cap, room = sm.arena_first_guess(*args)
                tags = {"test cap" if test_cap else "no test cap", "partition" if partition else "whole scene"}
                if not test_cap:
                    tags.add("seen cap above" if seen > base * world else "seen cap below")
                    tags.add("part seen above" if partition and part_seen > cap else "part seen below" if partition else "no part")
                    if partition:
                        tags.add("kept %d of 10" % kept)
                    elif guess <= 4:
                        tags.add("arena_guess <= 4")
                    elif free == sm.FREE_UNKNOWN:
                        tags.add("free unknown")
                    else:
                        tags.add("35 % cut binds" if int(float(free) * 0.35 / 40.0) < int(PAIRS * world * 0.001 * 8) + M1 else "free memory is plenty")
                tags.add("no room limit" if not room else "room binds" if cap == room else "room does not bind")
                out.append((args, (cap, room), tags))
    assert base == 14_248_576 and want8 == 27_448_576
    return out


def test_guess_grid_reaches_every_branch():
    seen = set().union(*(t for _, _, t in _guess_grid()))
    assert seen >= {"test cap", "no test cap", "partition", "whole scene", "seen cap above", "seen cap below", "part seen above", "part seen below", "kept 0 of 10",
                    "kept 3 of 10", "kept 10 of 10", "arena_guess <= 4", "free unknown", "35 % cut binds", "free memory is plenty", "no room limit", "room binds",
                    "room does not bind"}, seen
    g = lambda **kw: sm.arena_first_guess(**dict(dict(pairs=PAIRS, world=1, test_cap=0, seen_cap=0, arena_guess=4, free_bytes=sm.FREE_UNKNOWN, regrow_free_mb=0,      # noqa: E731
                                                      partition=False, kept_views=0, n_views=10, part_seen=0), **kw))[0]
    assert g() == g(arena_guess=8) == 14_248_576                               # 0.004 of the pairs + 2^20; the free memory is not known
    assert g(arena_guess=8, free_bytes=1 << 40) == 27_448_576                  # 0.008 of the pairs + 2^20
    assert g(arena_guess=8, free_bytes=int(20_000_000 * 40 / 0.35)) in (19_999_999, 20_000_000)      # what 35 % of the free memory holds at 40 B a record
    assert g(arena_guess=8, free_bytes=1000) == 14_248_576                     # (the cut never goes below the plain guess)
    assert g(seen_cap=50_000_000) == 50_000_000 and g(test_cap=77, seen_cap=50_000_000, arena_guess=8, free_bytes=1 << 40) == 77
    assert g(regrow_free_mb=256) == (256 << 20) // 36 == 7_456_540 and g(test_cap=8_000_000, regrow_free_mb=256) == 7_456_540
    assert g(partition=True, kept_views=3) == 14_248_576 * 3 // 10 + M1 and g(partition=True, kept_views=0) == M1
    assert g(partition=True, kept_views=3, part_seen=9_000_000) == 9_000_000
    assert g(partition=True, kept_views=3, arena_guess=8, free_bytes=1 << 40) == g(partition=True, kept_views=3)       # (a share does not look at the free memory)
    assert g(partition=True, kept_views=3, test_cap=77) == 77 and g(partition=True, kept_views=10, regrow_free_mb=256) == 7_456_540


def test_guess_hook_equals_model():
    capi = _capi()
    for args, m, _ in _guess_grid():
        assert capi.shard_arena_first_guess(*args) == m, args
    for pairs in (0.0, 1.0, 123456789.0, 2.5e11, 7.77e12):      # (the double expressions, bit for bit)
        for world, guess in ((1, 5), (3, 8), (8, 24)):
            args = (pairs, world, 0, 0, guess, 191 << 30, 0, False, 0, 10, 0)
            assert capi.shard_arena_first_guess(*args) == sm.arena_first_guess(*args), args


# ---- verdict and retry
def test_verdict_all_sixteen_combinations():
    capi = _capi()
    for bits in range(16):
        got = capi.shard_verdict(bits, 111, 222, 333)
        assert got == sm.verdict(bits, 111, 222, 333), bits
        assert (got[0] == 0 and got[1] == "") if bits == 0 else (got[0] == sm.NOMEM and got[1].startswith("l3d_shard_chain_run:") and got[1].endswith(";"))
    assert capi.shard_verdict(1, 111, 222, 333)[1] == "l3d_shard_chain_run: candidate capacity exceeded on a rank (111 candidates in one view's range; l3d_set_chain_capacities);"
    assert capi.shard_verdict(2, 111, 222, 333)[1] == "l3d_shard_chain_run: slot_records too small (222 kept matches in one view's range);"
    assert capi.shard_verdict(4, 111, 222, 333)[1] == "l3d_shard_chain_run: a rank gave up;"
    assert capi.shard_verdict(8, 111, 222, 5_000_000_000)[1] == "l3d_shard_chain_run: the compact kept arena of the slot ring is too small (5000000000 kept matches);"
    # the order of the parts: candidates, slot, arena, gave up
    t = capi.shard_verdict(15, 1, 2, 3)[1]
    assert t.index("candidate capacity") < t.index("slot_records") < t.index("compact kept arena") < t.index("gave up")


@functools.lru_cache(maxsize=None)
def _retry_grid():
    out = []
    for bits in range(16):
        for max_cand, max_kept, need, room, replay in itertools.product((100, 10_000_000), (10, 100_000), (1_000_000,), (0, 999_999, 1_000_000), (False, True)):
            args = (bits, 1_000_000, max_cand, 4096, max_kept, need, room, replay)
            m = sm.retry(*args)
            tags = set()
            if not bits & 11:
                tags.add("gave up alone" if bits == 4 else "no capacity bit")
            elif m["refuse_for_room"]:
                tags.add("room exceeded")
            elif bits & 2 and replay:
                tags.add("slot bit under replay")
            else:
                tags.add("retry")
                if bits & 4:
                    tags.add("retry although a rank gave up")
                if bits & 1:
                    tags.add("candidates: doubled" if m["cand_cap_next"] == 2_000_000 else "candidates: from the count")
                if bits & 2:
                    tags.add("slot: doubled" if m["slot_records_next"] == 8192 else "slot: from the count")
                if bits & 8:
                    tags.add("arena: room suffices" if room else "arena: no room limit")
            out.append((args, m, tags))
    return out


def test_retry_grid_reaches_every_branch():
    seen = set().union(*(t for _, _, t in _retry_grid()))
    assert seen >= {"gave up alone", "no capacity bit", "room exceeded", "slot bit under replay", "retry", "retry although a rank gave up", "candidates: doubled",
                    "candidates: from the count", "slot: doubled", "slot: from the count", "arena: room suffices", "arena: no room limit"}, seen
    for args, m, tags in _retry_grid():
        assert m["retry"] == ("retry" in tags), args
        if not m["retry"]:
            assert (m["cand_cap_next"], m["slot_records_next"], m["arena_cap_next"]) == (0, 0, 0), args
    capi = _capi()
    assert capi.shard_retry(4, 1000, 5, 64, 5, 0, 0, False) == dict(retry=False, cand_cap_next=0, slot_records_next=0, arena_cap_next=0, refuse_for_room=False)
    assert capi.shard_retry(1, 1000, 5, 64, 5, 0, 0, False)["cand_cap_next"] == 5 + 1 + 65536         # 1.25 x the count + 65536 beats the doubling
    assert capi.shard_retry(1, 1_000_000, 5, 64, 5, 0, 0, False)["cand_cap_next"] == 2_000_000
    assert capi.shard_retry(2, 1000, 5, 64, 5, 0, 0, False)["slot_records_next"] == 5 + 1 + 1024 and capi.shard_retry(2, 1000, 5, 4096, 5, 0, 0, False)["slot_records_next"] == 8192
    assert capi.shard_retry(8, 1000, 5, 64, 5, 1_000_000, 0, False) == dict(retry=True, cand_cap_next=0, slot_records_next=0, arena_cap_next=1_315_536, refuse_for_room=False)
    assert capi.shard_retry(8, 1000, 5, 64, 5, 1_000_000, 999_999, False) == dict(retry=False, cand_cap_next=0, slot_records_next=0, arena_cap_next=0, refuse_for_room=True)
    assert capi.shard_retry(2, 1000, 5, 64, 5, 0, 0, True)["retry"] is False and capi.shard_retry(1, 1000, 5, 64, 5, 0, 0, True)["retry"] is True


def test_retry_hook_equals_model():
    capi = _capi()
    for args, m, _ in _retry_grid():
        assert capi.shard_retry(*args) == m, args
