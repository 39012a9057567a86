"""Plain model of the step of the resident chain that collects a view's candidates (l3d_chain.hip: k_exist_count / k_place, k_exist_count_rt +
k_exist_combine / k_place_rt, k_scan, k_exist_sort_runs): every record of a source's kept list that points at the view becomes a reverse match in the
row of (its target segment, the source's camera), stage-1 rows keep their given order, the row starts are the exclusive sum of the row counts.
Python loops over numpy arrays; depths are moved, never computed: everything is held byte for byte."""
import numpy as np

MATCH_DTYPE = np.dtype([("segID1", "<u4"), ("camID2", "<u4"), ("segID2", "<u4"), ("depths", "<f4", (4,)), ("confidence", "<f4")])
CHUNKS = 16                 # chunks a source's segments are cut into by the run-table count
LONG_LIST = 262144


def reverse_rows(case):
    """row -> [(target, depths (4,) uint32 bits)] in ascending target order"""
    views, k = case["views"], case["k"]
    v = views[k]
    S, N = v["S"], len(v["l2g"])
    rows = {}
    for cam, si in zip(v["source_cam"], v["source_index"]):
        w = views[si]
        if w["n_tbm"] == 0 or (case["overflowed"] is not None and case["overflowed"][si]):
            continue                    # never verified: no list; overflowed: its result record says 0 records
        mine = w["kept"][(w["kept"]["camID2"] == v["id"]) & (w["kept"]["segID2"] < S)]
        for r in mine:
            if True:
                d = r["depths"].view(np.uint32)
                rows.setdefault(int(r["segID2"]) * N + int(cam), []).append((int(r["segID1"]), (int(d[2]), int(d[3]), int(d[0]), int(d[1]))))
    for row in rows:
        rows[row].sort(key=lambda e: e[0])
    return rows


def model(case):
    """-> dict(row_start, meta (R, 2), depths (R, 4) uint32 bits, cursor, rev_rows (the rows that hold reverse matches), seg_sizes)"""
    v = case["views"][case["k"]]
    S, N = v["S"], len(v["l2g"])
    rev = reverse_rows(case)
    counts = case["rowcnt"].astype(np.int64).copy()
    cursor = np.zeros(S * N, np.int32)
    for row, lst in rev.items():
        counts[row] += len(lst)
        cursor[row] = len(lst)
    row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    R = int(row_start[-1])
    meta, depths = np.zeros((R, 2), np.uint32), np.zeros((R, 4), np.uint32)
    dA = case["depthsA"].view(np.uint32).reshape(-1, 4)
    for cam in v["tbm"]:
        for y in range(S):
            row = y * N + cam
            a, n, b = int(case["rowA"][row]), int(case["rowcnt"][row]), int(row_start[row])
            meta[b:b + n], depths[b:b + n] = case["metaA"][a:a + n], dA[a:a + n]
    for row, lst in rev.items():
        b = int(row_start[row])
        for i, (tgt, d) in enumerate(lst):
            meta[b + i] = (tgt, row % N)
            depths[b + i] = d
    return dict(row_start=row_start, meta=meta, depths=depths, cursor=cursor, rev_rows=sorted(rev), R=R,
                seg_sizes=(row_start[N::N] - row_start[:-1:N]) if S else np.zeros(0, np.int32))


def seg_order_ok(order, seg_sizes):
    """a permutation of the segments whose bins 63 - min(63, m >> 5) never decrease; the order inside a bin is not determined"""
    S = len(seg_sizes)
    if sorted(np.asarray(order).tolist()) != list(range(S)):
        return False
    bins = 63 - np.minimum(63, np.asarray(seg_sizes)[np.asarray(order, np.int64)] >> 5)
    return bool(np.all(np.diff(bins) >= 0))


# ---- mirrors of the chain's rules (l3d_chain_common.hpp: chain_collect_rule, rt_lanes_per_run)
def lanes_rule(opt, avg_run):
    if opt == 0:
        return 1
    g = 1
    if opt < 0:
        while g < 64 and g < avg_run:
            g <<= 1
        return g
    while g < 64 and 2 * g <= opt:
        g <<= 1
    return g


def rules(case, route, rt_g, avg_kept):
    """-> (g, workgroups per source of the route taken, blocks_move)"""
    views, k = case["views"], case["k"]
    v = views[k]
    S, N = v["S"], len(v["l2g"])
    maxS = max(w["S"] for w in views[:k + 1])
    g = lanes_rule(rt_g, avg_kept / max(1.0, float(S) * max(1, N)))
    bps = int(min(512.0, max(32.0, avg_kept / 4096.0)))
    rt_bps = max(1, min(512, (maxS * max(1, g) + 255) // 256))
    return g, (rt_bps if route == 1 else bps), (S * len(v["tbm"]) + 3) // 4
