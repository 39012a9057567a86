"""The rule by which the single-GPU chain sizes its kept arena after an overflow (chain_arena_regrow, line3d_amd/csrc/l3d_chain_common.hpp; DESIGN.md
section 3), written from its statement: the same integer steps and the same double expression in the same order, so the projection agrees with the
library's bit for bit.  Pure arithmetic -- no device."""

MEM_UNKNOWN = 2 ** 64 - 1             # free_bytes: the card's free memory could not be read (no cut, no NOMEM)
EARLY_LIMIT = 0x7ffffff0              # early transposes index their entries with 31 bits
RECORD, SIDE_WORD, EARLY_ENTRY, TABLE_ENTRY = 32, 4, 4, 8
RESERVE_PRODUCTS = (1 << 28) * 24 + (1 << 30)       # the products' smallest transient blocks + 1 GB
RESERVE_PLAIN = 512 << 20


def arena_regrow(arena_cap, kept_base, n_want, done, span, free_bytes, turn_room, early, products):
    """-> dict(ok, new_cap, need, fits, per_rec, reserve); records except per_rec (bytes per record) and reserve (bytes)"""
    new_cap = 2 * arena_cap
    if done >= 4:
        first_half = 2 * done < span
        proj = int(float(kept_base) / done * span * (1.5 if first_half else 1.15)) + 1048576
        new_cap = max(new_cap, proj) if first_half else max(proj, arena_cap + arena_cap // 8)
    need = kept_base + max(0, n_want) + 65536
    new_cap = max(new_cap, need)
    per_rec = RECORD + SIDE_WORD + (EARLY_ENTRY if early and new_cap < EARLY_LIMIT else 0) + (TABLE_ENTRY if products else 0)
    reserve = 0 if turn_room else RESERVE_PRODUCTS if products else RESERVE_PLAIN
    known = free_bytes != MEM_UNKNOWN
    fits = turn_room if turn_room else (free_bytes - reserve) // per_rec if known and free_bytes > reserve else 0
    ok = True
    if known and new_cap > fits:
        if fits < need or fits <= arena_cap:
            ok = False
        else:
            new_cap = fits
    return dict(ok=ok, new_cap=new_cap, need=need, fits=fits, per_rec=per_rec, reserve=reserve)
