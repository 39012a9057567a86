"""The regrow rule of the single-GPU chain's kept arena (chain_arena_regrow in line3d_amd/csrc/l3d_chain_common.hpp) through its
host-only hook l3d_test_arena_regrow, held to tests/regrow_model.py on a grid that reaches every branch of the rule at the smallest numbers that do,
and to a few literal values where no rounding decides.  No device: tests/test_gpu_arena_regrow.py drives two of the branches on a card."""
import functools
import itertools

import regrow_model as rm

UNKNOWN = rm.MEM_UNKNOWN
CAP, SPAN = 10_000_000, 16
KEYS = ("ok", "new_cap", "need", "fits", "per_rec", "reserve")


def _hook(*args):
    from line3d_amd import capi
    return capi.arena_regrow(*args)


@functools.lru_cache(maxsize=None)
def _grid():
    """(arguments, model's answer, the branches the case takes) for every case"""
    out = []
    bases = itertools.product((0, 3, 4, 8, 12),                # views done: no projection | first half (2 * done < span) | past the middle
                              (1_000_000, 4_000_000, 8_000_000),   # records in use: the projection below the doubling / the eighth on top | above
                              (0, 100_000_000),                # the view's own count: need below | above the projection
                              (False, True), (False, True))
    for done, kept_base, n_want, early, products in bases:
        free0 = rm.arena_regrow(CAP, kept_base, n_want, done, SPAN, UNKNOWN, 0, early, products)
        rooms = sorted({free0["new_cap"], free0["new_cap"] - 1, free0["need"], free0["need"] - 1, CAP, CAP + 1, (free0["need"] + free0["new_cap"]) // 2})
        frees = [UNKNOWN, 0, free0["reserve"] - 1, free0["reserve"], free0["reserve"] + free0["per_rec"] - 1]
        frees += [free0["reserve"] + f * free0["per_rec"] + free0["per_rec"] - 1 for f in rooms]      # (the division rounds down)
        cases = [(fr, 0) for fr in frees] + [(fr, room) for room in rooms for fr in (0, UNKNOWN)]       # (a turn's room: the free memory is not looked at)
        for free, turn_room in cases:
            args = (CAP, kept_base, n_want, done, SPAN, free, turn_room, early, products)
            m = rm.arena_regrow(*args)
            tags = {"done %d" % done, "need above" if m["need"] == free0["new_cap"] else "need below"}      # (above the projection and the doubling)
            if free == UNKNOWN:
                tags.add("unknown")
            elif not m["ok"]:
                tags.add("nomem: the view does not fit" if m["fits"] < m["need"] else "nomem: no larger than the old arena")
                if m["fits"] == 0 and not turn_room:
                    tags.add("nothing free beyond the reserve")
            else:
                tags.add("cut" if m["new_cap"] == m["fits"] and m["new_cap"] < free0["new_cap"] else "fits")
            if turn_room and free != UNKNOWN:
                assert m["reserve"] == 0 and m["fits"] == turn_room
                tags.add("turn room")
            out.append((args, m, tags))
    return out


def test_the_grid_reaches_every_branch_of_the_rule():
    seen = set().union(*(tags for _, _, tags in _grid()))
    assert seen >= {"done 0", "done 3", "done 4", "done 8", "done 12", "need above", "need below", "unknown", "cut", "fits",
                    "nomem: the view does not fit", "nomem: no larger than the old arena", "nothing free beyond the reserve", "turn room"}, seen
    # the two NOMEM conditions apart, and the cut, on one case each (44 B per record, 7168 MB kept back)
    R = rm.RESERVE_PRODUCTS
    m = rm.arena_regrow(CAP, 8_000_000, 5_000_000, 4, SPAN, R + 12_000_000 * 44, 0, False, True)
    assert not m["ok"] and CAP < m["fits"] == 12_000_000 < m["need"] == 13_065_536
    m = rm.arena_regrow(CAP, 8_000_000, 0, 4, SPAN, R + 9_000_000 * 44, 0, False, True)
    assert not m["ok"] and m["need"] == 8_065_536 <= m["fits"] == 9_000_000 <= CAP
    m = rm.arena_regrow(CAP, 8_000_000, 0, 4, SPAN, R + 20_000_000 * 44, 0, False, True)
    assert m["ok"] and m["need"] <= m["fits"] == m["new_cap"] == 20_000_000 > CAP


def test_hook_equals_model_on_the_grid():
    for args, m, _ in _grid():
        got = _hook(*args)
        assert got == m, (args, got, m)


def test_early_transposes_count_below_their_31_bit_limit_only():
    """per_rec is taken from the size asked for, before the cut: 2 x arena_cap on either side of 0x7ffffff0, with and without products"""
    below, at = (rm.EARLY_LIMIT - 2) // 2, rm.EARLY_LIMIT // 2
    for products in (False, True):
        base = 36 + (8 if products else 0)
        for cap, early, want in ((below, True, base + 4), (at, True, base), (below, False, base), (at, False, base)):
            for free in (UNKNOWN, (rm.RESERVE_PRODUCTS if products else rm.RESERVE_PLAIN) + 0x50000000 * want):      # (the second: cut below the limit)
                args = (cap, 1000, 0, 0, SPAN, free, 0, early, products)
                got = _hook(*args)
                assert got == rm.arena_regrow(*args), args
                assert got["ok"] and got["per_rec"] == want and got["new_cap"] == (2 * cap if free == UNKNOWN else 0x50000000), (args, got)


def test_literal_values():
    assert _hook(1000, 900, 200, 3, 10, UNKNOWN, 0, False, False)["new_cap"] == 66636            # need = 900 + 200 + 65536 beats the doubling
    assert _hook(10_000_000, 8_000_000, 0, 4, 16, UNKNOWN, 0, False, False)["new_cap"] == 49_048_576     # 8e6 / 4 * 16 * 1.5 + 2^20
    got = _hook(10_000_000, 8_000_000, 0, 4, 16, 1 << 40, 0, False, True)
    # products without early transposes: what tests/test_gpu_arena_regrow.py restates as PER_REC and RESERVE_MB
    assert got["per_rec"] == 44 and got["reserve"] == 7168 << 20 and got["ok"] and got["new_cap"] == 49_048_576
    got = _hook(10_000_000, 8_000_000, 0, 4, 16, 1 << 40, 0, False, False)
    assert got["per_rec"] == 36 and got["reserve"] == 512 << 20
    assert _hook(10_000_000, 8_000_000, -5, 0, 16, UNKNOWN, 0, False, False)["need"] == 8_065_536     # (a negative count counts as 0)
