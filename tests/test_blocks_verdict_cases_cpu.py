"""The rules of matchViews sharded by blocks of views (l3d_blocks_rule.hpp in line3d_amd/csrc) through their host-only hook
l3d_test_blocks_verdict, held to tests/blocks_verdict_model.py on a grid that reaches every branch at the smallest shapes that do -- 7 views on 3 ranks
(blocks begin at 0, 2, 4) and 10 views on 4 ranks (0, 2, 5, 7), check 0..3, tail 0..4 -- and to a few literal cases.  No device: the GPU tests of
tests/test_gpu_partition.py and tests/test_gpu_pipeline_parity.py run the rule on whole scenes."""
import functools

import blocks_verdict_model as bm

SHAPES = ((7, 3), (10, 4))
KEYS = ("miss", "first_diff", "n_miss", "hopeless", "failed_rank", "t_rec", "t_seg", "t_first", "max_rec", "max_seg")


def _hook(n, W, check, tail, partition, table, comp_from, verified, S_src, **kw):
    from line3d_amd import capi
    return capi.blocks_verdict(n, W, check, tail, partition, [[e[0] for e in row] for row in table], [[e[1] for e in row] for row in table], comp_from, verified, S_src, **kw)


def _model(n, W, check, tail, partition, table, comp_from, verified, S_src):
    out = bm.verdict(table, n, W, check, tail, partition, comp_from)
    out.update(bm.handover_plan(table, n, W, check, out["miss"], verified, S_src))
    out["failed_rank"] = bm.failed_rank(table)
    return out


def _equal_table(n, W):
    return [[(1000 + k, 10 + k) for k in range(n)] for _ in range(W)]


def _scenarios(n, W, check, tail, partition):
    """(table, comp_from, tags the geometry of the change alone decides, the rank that was changed or None) of one configuration"""
    base = _equal_table(n, W)
    yield base, [0] * W, {"all equal"}, None
    for r in range(1, W):
        b, nxt = bm.begin(r, n, W), bm.begin(r + 1, n, W)
        lo = max(0, b - check)
        e = min(n, b + tail, nxt) if partition else b
        geo = set()
        if b - check < 0:
            geo.add("lo clamped at 0")
        if partition and b + tail > nxt and r + 1 < W:
            geo.add("e clamped by the next block")
        if partition and b + tail > n and r + 1 == W:
            geo.add("e clamped by n_views")
        where = {"at lo - 1": lo - 1, "at lo": lo, "at b - 1": b - 1, "at b": b, "at e - 1": e - 1, "at e": e}
        for name, k in where.items():
            if not 0 <= k < n:
                continue
            for what in ("hash", "n_kept"):
                t = [list(row) for row in base]
                t[r][k] = (t[r][k][0] + 1, t[r][k][1]) if what == "hash" else (t[r][k][0], t[r][k][1] + 3)
                yield t, [0] * W, geo | {"%s differs %s" % (what, name)}, r
        for name, first in (("comp_from == lo", lo), ("comp_from > lo", lo + 1)):
            cf = [0] * W
            cf[r] = first
            yield base, cf, geo | {name}, r
        if r + 1 < W and check >= 1:
            t = [list(row) for row in base]
            for q in (r, r + 1):
                k = bm.begin(q, n, W) - 1
                t[q][k] = (t[q][k][0] + 7, t[q][k][1] + 2)
            yield t, [0] * W, {"two adjacent ranks changed"}, r
    for name, r in (("mark on rank 0", 0), ("mark on the last rank", W - 1)):
        t = [list(row) for row in base]
        t[r][0] = bm.FAILURE_MARK
        yield t, [0] * W, {name}, None


@functools.lru_cache(maxsize=None)
def _grid():
    """(arguments, model's answer, the branches the case takes, the rank whose table or first view was changed) for every case"""
    out = []
    for n, W in SHAPES:
        S_src = [20 + 3 * k for k in range(n)]
        for partition in (False, True):
            for check in range(4):
                for tail in (range(5) if partition else (0, 3)):      # (replicas: the tail is not looked at)
                    for table, comp_from, tags, changed in _scenarios(n, W, check, tail, partition):
                        for vname, verified in (("all verified", [1] * n), ("every other view verified", [k % 2 for k in range(n)]), ("none verified", [0] * n)):
                            args = (n, W, check, tail, partition, table, comp_from, verified, S_src)
                            m = _model(*args)
                            tags = set(tags) | {"partitioned" if partition else "replicas", vname}
                            tags.add("miss" if m["n_miss"] else "no miss")
                            if m["hopeless"]:
                                tags.add("hopeless")
                                twin = _model(n, W, check, tail, True, table, comp_from, verified, S_src)
                                assert not twin["hopeless"]
                                tags.add("the same geometry partitioned is not hopeless")
                                if table == _equal_table(n, W):
                                    tags.add("hopeless with equal tables")
                            for r in range(1, W):
                                if m["miss"][r]:
                                    if m["t_first"][r - 1] == -1:
                                        assert m["t_seg"][r - 1] == 0
                                        tags.add("sender without a verified view")
                                    b = bm.begin(r, n, W)
                                    if sum(e[1] for e in table[r][max(0, b - check):b]) != m["t_rec"][r - 1]:
                                        tags.add("t_rec from the sender's row")
                                    if r + 1 < W and m["miss"][r + 1]:
                                        tags.add("two adjacent ranks missed")
                            tags.add("failure mark" if m["failed_rank"] >= 0 else "no failure mark")
                            out.append((args, m, tags, changed))
    return out


def _cases_with(*tags):
    """(arguments, model's answer, what the model says of the changed rank: its miss flag and first differing view)"""
    return [(a, m, (m["miss"][r], m["first_diff"][r]) if r is not None else None) for a, m, t, r in _grid() if set(tags) <= t]


def test_the_grid_reaches_every_branch_of_the_rule():
    seen = set().union(*(tags for _, _, tags, _ in _grid()))
    assert seen >= {"all equal", "replicas", "partitioned", "miss", "no miss", "hash differs at lo", "hash differs at b - 1", "hash differs at lo - 1", "n_kept differs at lo",
                    "n_kept differs at b - 1", "comp_from > lo", "comp_from == lo", "lo clamped at 0", "hopeless", "hopeless with equal tables",
                    "the same geometry partitioned is not hopeless", "hash differs at b", "hash differs at e - 1", "hash differs at e", "e clamped by the next block",
                    "e clamped by n_views", "sender without a verified view", "two adjacent ranks missed", "t_rec from the sender's row", "mark on rank 0",
                    "mark on the last rank", "failure mark", "no failure mark"}, seen
    # what each branch decides for the rank that was changed, on the model (the hook is held to it below); a[2], a[3]: check, tail
    assert all(m["n_miss"] == 0 for _, m, _ in _cases_with("all equal", "partitioned"))
    assert all(m["n_miss"] == 0 or m["hopeless"] for _, m, _ in _cases_with("all equal", "replicas"))
    for what in ("hash", "n_kept"):       # (n_kept alone, with the hash equal, is a difference)
        assert all(own == (0, -1) for _, m, own in _cases_with(what + " differs at lo - 1", "partitioned"))
        assert any(own == (0, -1) for _, m, own in _cases_with(what + " differs at lo - 1", "replicas"))
        for name in ("at lo", "at b - 1"):
            hit = [(a, own) for a, m, own in _cases_with("%s differs %s" % (what, name), "partitioned") if a[2] >= 1]      # (check 0: nothing in front of the block is compared)
            assert hit and all(own[0] == 1 and own[1] >= 0 for _, own in hit)
            assert all(own[0] == 1 for a, m, own in _cases_with("%s differs %s" % (what, name), "replicas") if a[2] >= 1)
        for name in ("at b", "at e - 1"):
            hit = [(a, own) for a, m, own in _cases_with("%s differs %s" % (what, name), "partitioned") if a[3] >= 1]
            assert hit and all(own[0] == 1 and own[1] >= 0 for _, own in hit)
        for clamp in ("e clamped by the next block", "e clamped by n_views"):
            assert any(own[0] == 1 for _, _, own in _cases_with(what + " differs at e - 1", clamp))
        hit = _cases_with(what + " differs at e", "e clamped by the next block")
        assert hit and all(own == (0, -1) for _, _, own in hit)
        assert all(own == (0, -1) for _, _, own in _cases_with(what + " differs at e", "partitioned"))
    assert all(own == (1, -1) and m["n_miss"] == 1 for _, m, own in _cases_with("comp_from > lo", "partitioned"))
    assert all(m["n_miss"] == 0 for _, m, _ in _cases_with("comp_from == lo", "partitioned"))
    assert any(m["n_miss"] == 0 for _, m, _ in _cases_with("comp_from == lo", "replicas"))
    assert all(m["n_miss"] >= 1 and m["first_diff"] == [-1] * a[1] for a, m, _ in _cases_with("hopeless with equal tables"))
    assert any(own[0] == 1 and own[1] == 0 for _, _, own in _cases_with("lo clamped at 0", "hash differs at lo", "partitioned"))
    assert all(m["failed_rank"] == 0 for _, m, _ in _cases_with("mark on rank 0")) and all(m["failed_rank"] == a[1] - 1 for a, m, _ in _cases_with("mark on the last rank"))
    assert all(m["failed_rank"] == -1 for _, m, _ in _cases_with("all equal"))


def test_hook_equals_model_on_the_grid():
    for args, m, _, _ in _grid():
        got = _hook(*args)
        assert {k: got[k] for k in KEYS} == m, (args, got, m)


def test_world_of_one_never_misses():
    for n in (1, 7):
        got = _hook(n, 1, 3, 4, True, _equal_table(n, 1), [0], [1] * n, [5] * n)
        assert got["miss"] == [0] and got["n_miss"] == 0 and not got["hopeless"] and got["begin"] == [0, n] and got["owner"] == [0] * n and got["max_rec"] == 0


def test_blocks_and_reach():
    for n, W in SHAPES + ((48, 3), (5, 8), (1, 3)):
        got = _hook(n, W, 0, 0, False, _equal_table(n, W), [0] * W, [1] * n, [1] * n)
        assert got["begin"] == [bm.begin(r, n, W) for r in range(W + 1)] and got["owner"] == [bm.owner(k, n, W) for k in range(n)], (n, W)
    assert _hook(7, 3, 0, 0, False, _equal_table(7, 3), [0] * 3, [1] * 7, [1] * 7)["begin"] == [0, 2, 4, 7]
    assert _hook(10, 4, 0, 0, False, _equal_table(10, 4), [0] * 4, [1] * 10, [1] * 10)["begin"] == [0, 2, 5, 7, 10]
    for window, nr in ((3, 0), (3, 3), (3, 5), (0, 0), (1, 2)):
        for partition in (False, True):
            got = _hook(7, 3, 0, 0, partition, _equal_table(7, 3), [0] * 3, [1] * 7, [1] * 7, window=window, neighbour_reach=nr)
            assert got["reach"] == bm.reach(window, nr, partition), (window, nr, partition)
    assert bm.reach(3, 5, True) == (5, 10, 10) and bm.reach(3, 5, False) == (5, 0, 3) and bm.reach(6, 2, True) == (6, 12, 12)


def test_literal_cases():
    n, W, S_src = 10, 4, [100] * 10
    t = _equal_table(n, W)                          # n_kept of view k: 10 + k
    t[2][4] = (t[2][4][0], 99)                      # rank 2 (block from 5) kept another number at view 4; rank 3 (block from 7) another list at view 6
    t[3][6] = (5, t[3][6][1])
    got = _hook(n, W, 2, 0, False, t, [0] * W, [1, 1, 1, 0, 1, 1, 0, 0, 1, 1], S_src)
    assert got["miss"] == [0, 0, 1, 1] and got["first_diff"] == [-1, -1, 4, 6] and got["n_miss"] == 2 and not got["hopeless"]
    # rank 1 hands over views 3, 4 (13 + 14 records by ITS row; view 3 is not verified), rank 2 views 5, 6 (15 + 16; view 6 is not verified)
    assert got["t_rec"] == [0, 27, 31, 0] and got["t_seg"] == [0, 100, 100, 0] and got["t_first"] == [-1, 4, 5, -1] and (got["max_rec"], got["max_seg"]) == (31, 100)
    # a check of 3 reaches past the blocks in front of ranks 1 and 3 (2 - 3 < 0, 7 - 3 < 5; rank 2: 5 - 3 = 2 does not): replicas cannot recover
    got = _hook(n, W, 3, 0, False, _equal_table(n, W), [0] * W, [1] * n, S_src)
    assert got["hopeless"] and got["miss"] == [0, 1, 0, 1] and got["first_diff"] == [-1] * 4
    got = _hook(n, W, 3, 0, True, _equal_table(n, W), [0] * W, [1] * n, S_src)
    assert not got["hopeless"] and got["n_miss"] == 0
    # the partitioned tail: rank 1's block is [2, 5); with a tail of 4 rank 0's views 2..4 are compared, view 5 is rank 2's business
    for k, want in ((2, 1), (4, 1), (5, 0)):
        t = _equal_table(n, W)
        t[1][k] = (1, t[1][k][1])
        assert _hook(n, W, 1, 4, True, t, [0] * W, [1] * n, S_src)["miss"][1] == want, k
