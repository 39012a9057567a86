"""Plain model of the slot kernels of the segment-sharded chain (l3d_chain_sharded.hip): the bytes of a slot, what k_slot_write leaves in one, what
k_exist_count_slots + the range scan + k_place_slots collect out of gathered slots, and what k_pack_view, k_shard_totals, k_check_slots,
k_shard_pack_all and k_shard_retire make of them.  Python loops over numpy arrays; the offsets come from capi.shard_slot_geometry (host only), nothing
is taken from device output.  Floats are only ever copied: everything is held byte for byte.

A geometry is a dict: the inputs (maxS, maxN, world, slot_records, slot_cams_min, n_views), the layout (seg_cap, best_off, bpos_off, rec_off, cam_off,
rt_off, slot_bytes, stage_bytes, max_n) and ring, the view blocks of the gathered buffer."""
import struct

import numpy as np

import keptwrite_model as km
from line3d_amd import capi

MATCH_DTYPE = km.MATCH_DTYPE
BESTPOS_CANARY = km.BESTPOS_CANARY
HEADER_KEYS = ("n_kept", "R", "overflow", "s0", "s1", "pad0", "pad1", "pad2")
INT_MAX = 0x7fffffff


def geometry(maxS, maxN, world, slot_records, slot_cams_min, n_views, ring=0):
    g = dict(maxS=maxS, maxN=maxN, world=world, slot_records=slot_records, slot_cams_min=slot_cams_min, n_views=n_views)
    g.update(capi.shard_slot_geometry(maxS, maxN, world, slot_records, slot_cams_min, n_views))
    if ring:
        g["ring"] = ring
    return g


def rank_range(S, r, world):
    """the source-segment range of rank r (chain_plan_views)"""
    return S * r // world, S * (r + 1) // world


def header(n_kept=0, R=0, overflow=0, s0=0, s1=0, pad0=0, pad1=0, pad2=0):
    return np.array([n_kept, R, overflow, s0, s1, pad0, pad1, pad2], np.int32)


# ---- the bytes of a slot
def build_slot(geom, hdr, best, bpos, records, side=None, rt=None):
    """-> slot_bytes uint8.  best (ns, 2) float32, bpos (ns,) int32, records MATCH_DTYPE, side (n,) uint32 and rt (rows, ns) int32 where the geometry
    has them (rows seg_cap apart).  What no part covers is 0xff (0x7f in the best positions)."""
    out = np.full(geom["slot_bytes"], 0xff, np.uint8)
    cap = geom["seg_cap"]
    out[geom["bpos_off"]:geom["bpos_off"] + 4 * cap] = 0x7f

    def put(off, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert off + len(b) <= len(out)
        out[off:off + len(b)] = b

    put(0, np.asarray(hdr, np.int32))
    best, bpos = np.asarray(best, np.float32).reshape(-1, 2), np.asarray(bpos, np.int32)
    assert len(best) <= cap and len(bpos) <= cap and len(records) <= geom["slot_records"]
    put(geom["best_off"], best)
    put(geom["bpos_off"], bpos)
    put(geom["rec_off"], np.asarray(records, MATCH_DTYPE))
    if side is not None and len(side):
        assert geom["cam_off"] and len(side) <= geom["slot_records"]
        put(geom["cam_off"], np.asarray(side, np.uint32))
    if rt is not None and np.size(rt):
        rt = np.asarray(rt, np.int32)
        assert geom["rt_off"] and rt.shape[0] <= geom["max_n"] + 1 and rt.shape[1] <= cap
        for q in range(rt.shape[0]):
            put(geom["rt_off"] + 4 * q * cap, rt[q])
    return out


def parse_slot(geom, b):
    """the parts of a slot at their full capacities: header (8 ints), best (seg_cap, 2), bpos (seg_cap), records (slot_records), side (slot_records)
    and rt (max_n + 1, seg_cap), the last two None where the geometry has none"""
    b = np.ascontiguousarray(b, np.uint8)
    assert len(b) == geom["slot_bytes"]
    cap, n = geom["seg_cap"], geom["slot_records"]
    part = lambda off, count, dt: b[off:off + count * np.dtype(dt).itemsize].view(dt)
    return dict(header=part(0, 8, np.int32), best=part(geom["best_off"], 2 * cap, np.float32).reshape(cap, 2), bpos=part(geom["bpos_off"], cap, np.int32),
                records=part(geom["rec_off"], n, MATCH_DTYPE), side=part(geom["cam_off"], n, np.uint32) if geom["cam_off"] else None,
                rt=part(geom["rt_off"], (geom["max_n"] + 1) * cap, np.int32).reshape(geom["max_n"] + 1, cap) if geom["rt_off"] else None)


def slot_of(geom, gathered, block, r):
    o = (block * geom["world"] + r) * geom["slot_bytes"]
    return gathered[o:o + geom["slot_bytes"]]


# ---- k_slot_write
def sub_case(case, s0, s1):
    """the view's candidates restricted to the segments [s0, s1), positions from 0"""
    N, rs = case["N"], case["row_start"]
    a, b = int(rs[s0 * N]), int(rs[s1 * N])
    return dict(S=s1 - s0, N=N, row_start=(rs[s0 * N:s1 * N + 1] - a).astype(np.int32), meta=case["meta"][a:b], depths=case["depths"][a:b], conf=case["conf"][a:b],
                l2g=case["l2g"])


def best_pairs(case):
    """(S, 2) floats, every one its own bit pattern: what the verification would leave as the best hypothesis' depths"""
    return (0x40000000 + 7 * np.arange(2 * case["S"], dtype=np.uint32)).view(np.float32).reshape(-1, 2)


def slot_parts(case, s0, s1, geom, cand_cap=None):
    """-> (header, best, bpos, records, side, rt) of the rank's slot"""
    S, N = case["S"], case["N"]
    R = int(case["row_start"][S * N])
    cand_cap = R if cand_cap is None else cand_cap
    sub = sub_case(case, s0, s1)
    total = int(km.kept_counts(sub).sum())
    overflow = 1 if R > cand_cap else 0
    n_kept = 0 if overflow else total
    if n_kept > geom["slot_records"]:
        overflow |= 2
        n_kept = 0
    hdr = header(n_kept, R, overflow, s0, s1, total)
    best = best_pairs(case)[s0:s1]
    if overflow:
        return hdr, best, np.full(s1 - s0, -1, np.int32), np.zeros(0, MATCH_DTYPE), None, None
    w = km.writer(sub, arena_cap=total)
    recs = w["records"].copy()
    recs["segID1"] += s0
    has = bool(geom["cam_off"])
    return hdr, best, w["best_pos"], recs, (w["side"] if has else None), (w["rt"] if has else None)


def slot_write(case, s0, s1, geom, cand_cap=None):
    """-> the slot's bytes after k_slot_write over a slot of 0xff bytes (0x7f in the best positions)"""
    return build_slot(geom, *slot_parts(case, s0, s1, geom, cand_cap))


def tables_of(records, l2g, s0, s1):
    """side words and run table (N + 1, s1 - s0) of a rank's records (global camera ids, segments in [s0, s1)), as the writer leaves them"""
    local = records.copy()
    local["segID1"] -= s0
    qt, rt, err = km.rebuild(local, s1 - s0, np.asarray(l2g, np.uint32))
    assert err == 0
    return qt, rt


def first_positions(records, s0, s1):
    """a best position per segment of the range that a writer could have left: the segment's first record, -1 without one"""
    bpos = np.full(s1 - s0, -1, np.int32)
    for i in range(len(records) - 1, -1, -1):
        bpos[int(records["segID1"][i]) - s0] = i
    return bpos


def slot_from_list(geom, l2g, records, s0, s1, R=0, best=None):
    """the slot of a rank that kept `records` (its part of the view's list, in order)"""
    n = len(records)
    assert n <= geom["slot_records"]
    side, rt = tables_of(records, l2g, s0, s1) if geom["cam_off"] else (None, None)
    best = np.zeros((s1 - s0, 2), np.float32) if best is None else best
    return build_slot(geom, header(n, R, 0, s0, s1, n), best, first_positions(records, s0, s1), records, side, rt)


def view_blocks(geom, view, bests=None):
    """the world slots of a view (dict S, l2g, kept) whose list is split over the ranks' ranges, back to back"""
    out = []
    for r in range(geom["world"]):
        s0, s1 = rank_range(view["S"], r, geom["world"])
        k = view["kept"]
        mine = k[(k["segID1"] >= s0) & (k["segID1"] < s1)]
        out.append(slot_from_list(geom, view["l2g"], mine, s0, s1, R=len(mine) * 3 + r, best=None if bests is None else bests[s0:s1]))
    return np.concatenate(out)


# ---- k_exist_count_slots, the range scan, k_place_slots, the ordering of the runs
def source_slot(views, k, q):
    """the local number view k has in the neighbour list of its q-th source; -1: not listed (chain_source_slot)"""
    w = views[int(views[k]["source_index"][q])]
    l = np.asarray(w["l2g"]).tolist()
    return l.index(views[k]["id"]) if views[k]["id"] in l else -1


def collect(views, k, gathered, geom, s0, s1, rowA, metaA, depthsA, rowcnt, tags=None):
    """-> dict(row_start, meta (R, 2), depths (R, 4) uint32 bits, cursor, rev_rows, R, seg_sizes): reverse matches out of the RECORDS of every slot
    that is not overflowed, of every source that lists the view, whose target lies in [s0, s1), in ascending target order; stage-1 rows of the
    range's segments; row starts of the range's rows only, 0xffffffff elsewhere"""
    v = views[k]
    S, N = v["S"], len(v["l2g"])
    tags = set() if tags is None else tags
    rows = {}
    for q, (cam, si) in enumerate(zip(v["source_cam"], v["source_index"])):
        if source_slot(views, k, q) < 0:
            tags.add("source that does not list the view")
            continue
        for r in range(geom["world"]):
            p = parse_slot(geom, slot_of(geom, gathered, int(si) % geom["ring"], r))
            h = dict(zip(HEADER_KEYS, p["header"].tolist()))
            if h["overflow"]:
                tags.add("source slot with overflow bit %d" % h["overflow"])
                continue
            if h["n_kept"] == 0:
                tags.add("source slot without records")
            if h["n_kept"] > 4096:
                tags.add("record scan wraps its grid stride")
            for rec in p["records"][:h["n_kept"]]:
                u = int(rec["segID2"])
                if int(rec["camID2"]) == v["id"]:
                    for edge, what in ((s0 - 1, "s0 - 1"), (s0, "s0"), (s1 - 1, "s1 - 1"), (s1, "s1")):
                        if u == edge and s1 > s0:
                            tags.add("target at " + what)
                    if s0 <= u < s1:
                        d = rec["depths"].view(np.uint32)
                        rows.setdefault(u * N + int(cam), []).append((int(rec["segID1"]), (int(d[2]), int(d[3]), int(d[0]), int(d[1]))))
    for row in rows:
        rows[row].sort(key=lambda e: e[0])
    counts = np.zeros(S * N, np.int64)
    counts[s0 * N:s1 * N] = rowcnt[s0 * N:s1 * N]
    cursor = np.full(S * N, -1, np.int32)
    cursor[s0 * N:s1 * N] = 0
    for row, lst in rows.items():
        counts[row] += len(lst)
        cursor[row] = len(lst)
    excl = np.concatenate([[0], np.cumsum(counts[s0 * N:s1 * N])]).astype(np.int32)
    R = int(excl[-1])
    row_start = np.full(S * N + 1, -1, np.int32)
    row_start[s0 * N:s1 * N + 1] = excl
    row_start[S * N] = R
    meta, depths = np.zeros((R, 2), np.uint32), np.zeros((R, 4), np.uint32)
    dA = np.asarray(depthsA, np.float32).view(np.uint32).reshape(-1, 4)
    for cam in v["tbm"]:
        for y in range(s0, s1):
            row = y * N + int(cam)
            a, n, b = int(rowA[row]), int(rowcnt[row]), int(row_start[row])
            meta[b:b + n], depths[b:b + n] = metaA[a:a + n], dA[a:a + n]
    for row, lst in rows.items():
        b = int(row_start[row])
        for i, (tgt, d) in enumerate(lst):
            meta[b + i] = (tgt, row % N)
            depths[b + i] = d
    sizes = np.array([int(counts[y * N:(y + 1) * N].sum()) for y in range(s0, s1)], np.int64)
    if s1 == s0:
        tags.add("empty range")
    if s1 - s0 == 1:
        tags.add("range of one segment")
    return dict(row_start=row_start, meta=meta, depths=depths, cursor=cursor, rev_rows=sorted(rows), R=R, seg_sizes=sizes)


def seg_order_ok(order, s0, s1, seg_sizes):
    """the first s1 - s0 entries: the range's segments, bins 63 - min(63, m >> 5) never decreasing (the order inside a bin is the atomics'); behind them
    nothing was written"""
    order = np.asarray(order)
    n = s1 - s0
    if not (order[n:] == -1).all() or sorted(order[:n].tolist()) != list(range(s0, s1)):
        return False
    bins = 63 - np.minimum(63, np.asarray(seg_sizes)[order[:n].astype(np.int64) - s0] >> 5)
    return bool(np.all(np.diff(bins) >= 0))


# ---- the consumers of the gathered blocks
def headers_in_front(geom, gathered):
    """(n_views, world, 8) int32: the headers in front of the slots of a buffer that holds every view's block"""
    nv, W = geom["n_views"], geom["world"]
    return np.array([[parse_slot(geom, slot_of(geom, gathered, k, r))["header"] for r in range(W)] for k in range(nv)], np.int32).reshape(nv, W, 8)


def _n(h):
    return 0 if h[2] else int(h[0])


def totals(hdrs, verified):
    """k_shard_totals -> (n_views, 2): kept records and candidates per verified view, the candidates clamped at 2^31 - 1"""
    out = np.zeros((len(hdrs), 2), np.int32)
    for k in range(len(hdrs)):
        if verified[k]:
            out[k] = (sum(_n(h) for h in hdrs[k]), min(sum(int(h[1]) for h in hdrs[k]), INT_MAX))
    return out


def check(hdrs, verified):
    """k_check_slots -> (OR of the overflow bits, largest R, largest pad[0]) over the verified views' headers"""
    bits = mr = mk = 0
    for k in range(len(hdrs)):
        if verified[k]:
            for h in hdrs[k]:
                bits, mr, mk = bits | (int(h[2]) & 7), max(mr, int(h[1])), max(mk, int(h[5]))
    return np.array([bits, mr, mk], np.int32)


def pack_view(geom, gathered, k):
    """k_pack_view -> (stage bytes, the 32 bytes of the PackHeader): the ranks' depth pairs seg_cap apart, then their records back to back; a rank with an
    overflow bit or an impossible count makes the whole view `bad`: no record, n_kept 0"""
    W, cap = geom["world"], geom["seg_cap"]
    out = np.full(geom["stage_bytes"], 0xff, np.uint8)
    parts = [parse_slot(geom, slot_of(geom, gathered, k, r)) for r in range(W)]
    ok = [not p["header"][2] and 0 <= p["header"][0] <= geom["slot_records"] for p in parts]
    bad = not all(ok)
    base = 0
    for r, p in enumerate(parts):
        h = p["header"]
        nb = int(h[4] - h[3])
        out[r * cap * 8:r * cap * 8 + nb * 8] = p["best"][:nb].view(np.uint8).reshape(-1)
        if not bad:
            n = int(h[0])
            o = W * cap * 8 + base * 32
            out[o:o + n * 32] = p["records"][:n].view(np.uint8).reshape(-1)
        base += int(h[0]) if ok[r] else 0
    R = sum(int(p["header"][1]) for p in parts)
    return out, np.frombuffer(struct.pack("<qii4i", R, 0 if bad else base, 1 if bad else 0, 0, 0, 0, 0), np.uint8)


def _canaries(arena_cap, best_cap):
    return (km.canary_records(arena_cap), np.full((best_cap, 2), 0xffffffff, np.uint32), np.full(best_cap, BESTPOS_CANARY, np.int32))


def _file_best(p, o, n, in_front, best, bestpos):
    h = p["header"]
    for i in range(int(h[4] - h[3])):
        best[o + int(h[3]) + i] = p["best"][i].view(np.uint32)
        bp = int(p["bpos"][i])
        bestpos[o + int(h[3]) + i] = -1 if bp < 0 or n == 0 else in_front + bp


def pack_all(geom, gathered, verified, best_off, pack_cap, best_cap):
    """k_shard_pack_all -> dict(arena, best (uint32 bits), bestpos): the verified views back to back, each the ranks' records in rank order"""
    arena, best, bestpos = _canaries(pack_cap, best_cap)
    base_k = 0
    for k in range(geom["n_views"]):
        if not verified[k]:
            continue
        in_front = 0
        for r in range(geom["world"]):
            p = parse_slot(geom, slot_of(geom, gathered, k, r))
            n = _n(p["header"])
            arena[base_k + in_front:base_k + in_front + n] = p["records"][:n]
            _file_best(p, int(best_off[k]), n, in_front, best, bestpos)
            in_front += n
        base_k += in_front
    return dict(arena=arena, best=best, bestpos=bestpos, total=base_k)


def retire(geom, gathered, verified, keep, best_off, view_sn, rt_off, batches, arena_cap, best_cap, rt_cap, tables):
    """k_shard_retire in the batches (first, count, enqueued at) over a ring filled as the exchanges fill it -> dict(arena, best, bestpos, base_dev, hdr_all,
    overflow, qt, rt_all)"""
    nv, W, ring, cap = geom["n_views"], geom["world"], geom["ring"], geom["seg_cap"]
    block = W * geom["slot_bytes"]
    ringbuf = np.full(ring * block, 0xff, np.uint8)
    arena, best, bestpos = _canaries(arena_cap, best_cap)
    base_dev = np.zeros(nv + 2, np.int64)
    hdr_all = np.full((nv, W, 8), -1, np.int32)
    qt, rt_all = np.full(arena_cap, 0xffffffff, np.uint32), np.full(rt_cap, -1, np.int32)
    overflow, exchanged = 0, 0
    here = lambda q: bool(verified[q]) and (keep is None or bool(keep[q]))
    for first, count, at in batches:
        for j in range(exchanged, at):
            ringbuf[(j % ring) * block:(j % ring + 1) * block] = gathered[j * block:(j + 1) * block] if verified[j] else 0
        exchanged = max(exchanged, at)
        base = int(base_dev[first])
        for k in range(first, first + count):
            parts = [parse_slot(geom, slot_of(geom, ringbuf, k % ring, r)) for r in range(W)]
            ns = [_n(p["header"]) for p in parts]
            all_k = sum(ns) if here(k) else 0
            base_dev[k] = base
            if k == first + count - 1:
                base_dev[k + 1] = base + all_k
            if not verified[k]:
                hdr_all[k] = 0
                continue
            hdr_all[k] = [p["header"] for p in parts]
            if here(k):
                if base + all_k > arena_cap:
                    overflow = 1
                else:
                    S, N = int(view_sn[k][0]), int(view_sn[k][1])
                    in_front = 0
                    for r, p in enumerate(parts):
                        n, h = ns[r], p["header"]
                        arena[base + in_front:base + in_front + n] = p["records"][:n]
                        _file_best(p, int(best_off[k]), n, in_front, best, bestpos)
                        if tables:
                            qt[base + in_front:base + in_front + n] = p["side"][:n]
                            for q in range(N + 1):
                                for j in range(int(h[4] - h[3])):
                                    rt_all[int(rt_off[k]) + q * S + int(h[3]) + j] = in_front + (int(p["rt"][q, j]) if n > 0 else 0)
                        in_front += n
            base += all_k
    return dict(arena=arena, best=best, bestpos=bestpos, base_dev=base_dev, hdr_all=hdr_all, overflow=overflow, qt=qt, rt_all=rt_all)


# ---- what a case reaches (tests/test_shardslot_cases_cpu.py and tests/test_gpu_shard_slots.py hold the union to one fixed list)
def writer_tags(case, s0, s1, geom, cand_cap=None):
    hdr = slot_parts(case, s0, s1, geom, cand_cap)[0]
    n, ovf, total = int(hdr[0]), int(hdr[2]), int(hdr[5])
    N, rs = case["N"], case["row_start"]
    tags = {"writer: side words and run table" if geom["cam_off"] else "writer: records only"}
    if s1 == s0:
        tags.add("writer: empty range, header only")
    if s1 - s0 == 1:
        tags.add("writer: range of one segment")
    for bit in (1, 2):
        if ovf == bit:
            tags.add("writer: overflow bit %d" % bit)
    if ovf:
        return tags
    if n and n == geom["slot_records"]:
        tags.add("writer: exact fit")
    if s0 > 0 and n and geom["cam_off"]:
        tags.add("writer: run table of a rank other than 0")
    if s1 - s0 > 256 and n:
        tags.add("writer: more than 256 segments in the range")
    if n and any(int(rs[(y + 1) * N] - rs[y * N]) > 2048 for y in range(s0, s1)):
        tags.add("writer: segment of several rounds")
    if N > 64 and n and geom["cam_off"]:
        tags.add("writer: run-table prefix over two camera chunks")
    if N < geom["max_n"] and n and geom["cam_off"]:
        tags.add("writer: fewer neighbours than the geometry's most")
    if N == 1:
        tags.add("writer: one neighbour")
    with np.errstate(invalid="ignore"):
        c = case["conf"][int(rs[s0 * N]):int(rs[s1 * N])]
        if np.isnan(c).any() and (c == np.float32(1.0)).any():
            tags.add("writer: NaN and 1.0 are not kept")
    return tags


def pack_tags(inp):
    geom, ver, keep, batches = inp["geom"], inp["verified"], inp["keep"], inp["batches"]
    nv = geom["n_views"]
    hdrs = headers_in_front(geom, inp["gathered"])
    tags = {"pack: world %d" % geom["world"], "pack: retire tables " + ("on" if inp["tables"] else "off"),
            "pack: keep " + ("absent" if keep is None else "all" if keep.all() else "some")}
    if not ver.all():
        tags.add("pack: unverified view")
    for k in range(nv):
        if ver[k] and all(_n(h) == 0 and not h[2] for h in hdrs[k]):
            tags.add("pack: view without records")
        if ver[k] and any(h[2] for h in hdrs[k]) and any(_n(h) for h in hdrs[k]):
            tags.add("pack: overflowed slot among good ones")
        if ver[k] and sum(int(h[1]) for h in hdrs[k]) > INT_MAX:
            tags.add("pack: candidates clamped at 2^31 - 1")
    last_at = max([b[2] for b in batches] + [0])
    tags.add("pack: ring of all views" if geom["ring"] >= nv and keep is None else "pack: partitioned ring that never wraps" if geom["ring"] >= nv else
             "pack: ring that wraps" if last_at > geom["ring"] else "pack: ring")
    for i, (first, count, at) in enumerate(batches):
        tags.add("pack: batch of 1" if count == 1 else "pack: batch of 16" if count == 16 else "pack: ragged batch")
    here = ver.astype(bool) & (np.ones(nv, bool) if keep is None else keep.astype(bool))
    kept_total = int(totals(hdrs, ver)[:, 0][here].sum())
    if kept_total and inp["arena_cap"] == kept_total:
        tags.add("pack: arena fits exactly")
    if inp["arena_cap"] == kept_total - 1:
        tags.add("pack: arena one record short")
    return tags
