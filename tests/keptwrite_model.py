"""Plain model of the chains' kept writer (k_kept_write_chain / write_kept_segment_wg, l3d_kept.hpp) and of the rebuild of side words and run tables
from records (k_qt_from_records / k_qt_order_seams / k_rt_from_qt, l3d_chain_common.hip): Python loops over numpy arrays, nothing taken from device
output.  Floats are only ever compared (confidence > 1) or halved (exact); everything is held byte for byte."""
import numpy as np

MATCH_DTYPE = np.dtype([("segID1", "<u4"), ("camID2", "<u4"), ("segID2", "<u4"), ("depths", "<f4", (4,)), ("confidence", "<f4")])
BESTPOS_CANARY = 0x7f7f7f7f


def canary_records(n):
    return np.frombuffer(b"\xff" * (n * MATCH_DTYPE.itemsize), dtype=MATCH_DTYPE).copy()


def kept_counts(case):
    """per segment: candidates with a confidence above 1 (float32 comparison; a NaN is not kept)"""
    S, N, rs = case["S"], case["N"], case["row_start"]
    with np.errstate(invalid="ignore"):
        k = case["conf"] > np.float32(1.0)
    return np.array([int(k[rs[y * N]:rs[(y + 1) * N]].sum()) for y in range(S)], np.int32)


def writer(case, prev=None, cand_cap=None, arena_cap=0):
    """-> dict(records, side, rt, best_pos, kept_base, n_kept, R, overflow, n_want): the whole arena of arena_cap records with its canaries"""
    S, N, rs = case["S"], case["N"], case["row_start"]
    R = int(rs[S * N])
    cand_cap = R if cand_cap is None else cand_cap
    cnt = kept_counts(case)
    total = int(cnt.sum())
    overflow = 1 if R > cand_cap else 0
    n_kept = 0 if overflow else total
    base = prev[0] + prev[1] if prev is not None else 0
    n_want = 0
    if base + n_kept > arena_cap:
        overflow |= 2
        n_want, n_kept = n_kept, 0
    out = dict(records=canary_records(arena_cap), side=np.full(arena_cap, 0xffffffff, np.uint32), rt=np.full((N + 1, S), -1, np.int32),
               best_pos=np.full(S, BESTPOS_CANARY, np.int32), kept_base=base, n_kept=n_kept, R=R, overflow=overflow, n_want=n_want)
    if overflow:
        return out
    recs, side = out["records"], out["side"]
    pos = 0
    two = np.float32(2.0)
    for y in range(S):
        first = pos
        best, best_c = -1, None
        per_cam = np.zeros(N + 1, np.int64)
        for i in range(rs[y * N], rs[(y + 1) * N]):
            c = case["conf"][i]
            if not c > np.float32(1.0):
                continue
            tgt, cam = int(case["meta"][i, 0]), int(case["meta"][i, 1])
            p = base + pos
            recs["segID1"][p], recs["camID2"][p], recs["segID2"][p] = y, case["l2g"][cam], tgt
            recs["depths"][p] = case["depths"][i]
            recs["confidence"][p] = c / two
            side[base + pos] = (cam << 16) | tgt
            per_cam[cam] += 1
            if best_c is None or c > best_c:        # the first strict maximum in list order
                best, best_c = pos, c
            pos += 1
        out["best_pos"][y] = best
        run = first
        for q in range(N + 1):
            out["rt"][q, y] = run
            run += per_cam[q]
    assert pos == total
    # (depths are copied as bytes: assigning a float32 NaN keeps its payload in numpy, and the comparison is on bytes)
    return out


def rebuild(records, S, l2g):
    """-> (qt (n,), rt (N + 1, S), err): side words and run table of a list from its records alone, and the error count of the launch"""
    N, n = len(l2g), len(records)
    local = {int(g): q for q, g in enumerate(l2g)}
    qt = np.zeros(n, np.uint32)
    key = np.zeros(n, np.uint64)
    err = 0
    for i, r in enumerate(records):
        q = local.get(int(r["camID2"]))
        known = q is not None and int(r["segID1"]) < S and int(r["segID2"]) < 65536
        qt[i] = ((q if known else 0xffff) << 16) | (int(r["segID2"]) & 0xffff)
        key[i] = ((int(r["segID1"]) << 8) | q) & 0xffffffff if known else 0xffffffff
        err += 0 if known else 1
    for i in range(1, n):
        if key[i] != 0xffffffff and key[i - 1] != 0xffffffff and key[i - 1] > key[i]:
            err += 1
    rt = np.zeros((N + 1, S), np.int32)
    for q in range(N + 1):
        for s in range(S):
            want = (s << 8) | q if q < N else (s + 1) << 8
            rt[q, s] = int(np.searchsorted(key, want, side="left")) if err == 0 else _lower_bound(key, want)
    return qt, rt, err


def _lower_bound(key, want):
    """the kernel's binary search, step for step: on an unordered list its answer is whatever the probes say"""
    lo, hi = 0, len(key)
    while lo < hi:
        mid = (lo + hi) >> 1
        if key[mid] < want:
            lo = mid + 1
        else:
            hi = mid
    return lo
