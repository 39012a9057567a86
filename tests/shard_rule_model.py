"""The sizing rules of the segment-sharded run (l3d_shard_rule.hpp, line3d_amd/csrc; DESIGN.md section 6 i, iv), written from their statements: the same
integer steps and the same double expressions in the same order, so the first guess of the compact arena agrees with the library's bit for bit.
Pure arithmetic -- no device."""

RECORD, SLOT_HEADER, SIDE_WORD = 32, 32, 4
RETIRE_BATCH = 16
GATHERED_BUDGET = 8 << 30
FREE_UNKNOWN = -1
NOMEM = 3
BIT_CANDIDATES, BIT_SLOT, BIT_GAVE_UP, BIT_ARENA = 1, 2, 4, 8


def align(x, a):
    return (x + a - 1) // a * a


def slot_geometry(maxS, maxN, world, slot_records, slot_cams_min, n_views):
    """a slot: header | best depth pairs | best positions | records | side words (dense slots) | run table (with the side words)"""
    seg_cap = (maxS + world - 1) // world + 1
    best_off = SLOT_HEADER
    bpos_off = best_off + 8 * seg_cap
    rec_off = align(bpos_off + 4 * seg_cap, 32)
    end = rec_off + RECORD * slot_records
    cam_off = rt_off = 0
    if slot_records >= slot_cams_min:
        cam_off = align(end, 32)
        rt_off = align(cam_off + SIDE_WORD * slot_records, 32)
        end = rt_off + 4 * (maxN + 1) * seg_cap
    return dict(seg_cap=seg_cap, best_off=best_off, bpos_off=bpos_off, rec_off=rec_off, cam_off=cam_off, rt_off=rt_off, slot_bytes=align(end, 256),
                stage_bytes=align(world * (8 * seg_cap + RECORD * slot_records), 256), ring=max(1, n_views), max_n=maxN)


def ring_plan(n_views, window, block_bytes, slot_ring, partition, host_commit):
    """-> dict(ring_mode, ring_views, send_ring)"""
    ring = min(window + RETIRE_BATCH + 2, max(1, n_views))
    if partition:
        mode = True
    elif host_commit or slot_ring == 0 or ring >= n_views:
        mode = False
    else:
        mode = slot_ring > 0 or n_views * block_bytes > GATHERED_BUDGET
    return dict(ring_mode=mode, ring_views=ring if mode else max(1, n_views), send_ring=ring if mode else n_views)


def room_records(regrow_free_mb):
    return (regrow_free_mb << 20) // (RECORD + SIDE_WORD) if regrow_free_mb > 0 else 0


def arena_first_guess(pairs, world, test_cap, seen_cap, arena_guess, free_bytes, regrow_free_mb, partition, kept_views, n_views, part_seen):
    """-> (records of the first guess, room in records); free_bytes FREE_UNKNOWN: not known"""
    room = room_records(regrow_free_mb)
    if test_cap:
        cap = test_cap
    else:
        cap = max(int(float(pairs) * world * 0.004) + 1048576, seen_cap)
        if not partition and arena_guess > 4 and free_bytes != FREE_UNKNOWN:
            want = int(float(pairs) * world * 0.001 * arena_guess) + 1048576
            fits = int(float(free_bytes) * 0.35 / 40.0)
            cap = max(cap, min(want, fits))
        if partition:
            cap = max(part_seen, cap * kept_views // max(1, n_views) + 1048576)
    if room > 0:
        cap = min(cap, room)
    return cap, room


def verdict(bits, max_cand, max_kept, arena_total):
    """-> (return code, text)"""
    if not bits:
        return 0, ""
    text = "l3d_shard_chain_run:"
    if bits & BIT_CANDIDATES:
        text += " candidate capacity exceeded on a rank (%d candidates in one view's range; l3d_set_chain_capacities);" % max_cand
    if bits & BIT_SLOT:
        text += " slot_records too small (%d kept matches in one view's range);" % max_kept
    if bits & BIT_ARENA:
        text += " the compact kept arena of the slot ring is too small (%d kept matches);" % arena_total
    if bits & BIT_GAVE_UP:
        text += " a rank gave up;"
    return NOMEM, text


def retry(bits, cand_cap, max_cand, slot_records, max_kept, arena_needed, room, replay):
    """-> dict(retry, cand_cap_next, slot_records_next, arena_cap_next, refuse_for_room); 0: as it was"""
    out = dict(retry=False, cand_cap_next=0, slot_records_next=0, arena_cap_next=0, refuse_for_room=False)
    if not bits & (BIT_CANDIDATES | BIT_SLOT | BIT_ARENA):
        return out
    if bits & BIT_ARENA and room > 0 and arena_needed > room:
        out["refuse_for_room"] = True
        return out
    if bits & BIT_SLOT and replay:
        return out
    out["retry"] = True
    if bits & BIT_ARENA:
        out["arena_cap_next"] = arena_needed + arena_needed // 4 + 65536
    if bits & BIT_CANDIDATES:
        out["cand_cap_next"] = max(2 * cand_cap, max_cand + max_cand // 4 + 65536)
    if bits & BIT_SLOT:
        out["slot_records_next"] = max(2 * slot_records, max_kept + max_kept // 4 + 1024)
    return out


def retire_run(n_views, window, slot_ring, partition, apart):
    """The retirement of a ring-mode run, view by view: before view k is enqueued a batch of 16 goes once 16 views in front of k - window are not retired
    yet; on a side stream (apart) the chain waits for a batch when the next one is enqueued, or at the first view whose exchange overwrites a block
    of it (the batch's first view + ring).  After the last view everything left is retired in batches and waited for.
    -> dict(ring_mode, ring, retired_at, waited_at, batches [(first, count, at, waited before)], retired, waited, outstanding)"""
    plan = ring_plan(n_views, window, 1, slot_ring, partition, False)
    out = dict(ring_mode=plan["ring_mode"], ring=plan["ring_views"], retired_at=[0] * n_views, waited_at=[0] * n_views, batches=[], retired=0, waited=0, outstanding=False)
    if not plan["ring_mode"]:
        return out
    ring, apart = plan["ring_views"], bool(apart)
    retired = waited = 0

    def retire_to(upto, at):
        nonlocal retired, waited
        while retired < upto:
            n = min(RETIRE_BATCH, upto - retired)
            before = apart and waited < retired
            if before:
                waited = retired                    # (the batch before this one)
            out["batches"].append((retired, n, at, int(before)))
            retired += n
            if not apart:
                waited = retired                    # (same stream: ordered)

    for k in range(n_views):
        if k - window - retired >= RETIRE_BATCH:
            retire_to(k - window, k)
        if waited < retired and k >= waited + ring:         # (waited = the outstanding batch's first view)
            waited = retired
        out["retired_at"][k], out["waited_at"][k] = retired, waited
    retire_to(n_views, n_views)
    waited = retired
    out.update(retired=retired, waited=waited, outstanding=False)
    return out
