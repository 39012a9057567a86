"""Crafted schedules and kept lists for the step of the resident chain that collects a view's candidates (l3d_chain.hip), one case per edge of its
kernels: the lengths of a (segment, camera) run of reverse matches around the 64 lanes of a wave, the 256 entries a wave orders in registers and the
512 of two staged passes; a source's segment count against the 16 chunks of the run-table count; the 16384 segments of the largest LDS histogram;
sources that must contribute nothing; list lengths against the 8192 records one pass of the scanning kernels covers at the fewest workgroups; the
neighbour counts; the 4096-int tiles of the row scan; stage-1 rows laid out with gaps.  Every case is made from those numbers, seeded, never from
device output.  tests/test_collect_cases_cpu.py holds each case to what its name claims, tests/test_gpu_collect_paths.py runs them.

A case: name, views (one dict per chain view: id, S, l2g, n_tbm, tbm, source_cam, source_index, kept), k (the view under test, always the last),
overflowed (None or a flag per view), rowA / metaA / depthsA / rowcnt (view k's stage-1 rows) and `about`."""
import numpy as np

from collect_model import MATCH_DTYPE

RUN_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000)
TILE = 4096
MIN_BPS_RECORDS = 32 * 256          # what one pass of the scanning kernels covers at the fewest workgroups per source
SPECIAL_DEPTH_BITS = (0x80000000, 0x00000001, 0x7fc00123)      # -0.0, a denormal, a NaN payload

_bits = [0]


def fresh_depths(n):
    """n x 4 floats, every one its own bit pattern (over the whole module)"""
    b = (0x3f000000 + 13 * (_bits[0] + np.arange(n * 4, dtype=np.uint64))).astype(np.uint32)
    _bits[0] += n * 4
    return b.view(np.float32).reshape(n, 4)


def view(vid, S, l2g, tbm=(), sources=(), kept=None):
    return dict(id=vid, S=S, l2g=np.asarray(l2g, np.uint32), n_tbm=len(tbm), tbm=np.asarray(tbm, np.int32),
                source_cam=np.asarray([c for c, _ in sources], np.int32), source_index=np.asarray([i for _, i in sources], np.int32),
                kept=np.zeros(0, MATCH_DTYPE) if kept is None else kept)


def kept_list(w, triples):
    """a kept list of view w from (segment, local camera, target segment) triples, put into (segment, camera, target) order"""
    t = sorted(set(triples))
    recs = np.zeros(len(t), MATCH_DTYPE)
    if t:
        a = np.array(t, np.int64)
        assert a[:, 0].max() < w["S"] and a[:, 1].max() < len(w["l2g"])
        recs["segID1"], recs["camID2"], recs["segID2"] = a[:, 0], w["l2g"][a[:, 1]], a[:, 2]
        recs["depths"] = fresh_depths(len(t))
        recs["confidence"] = 0.75
    return recs


def stage1(S, N, tbm, counts, gap, seed):
    """stage-1 rows of the cameras `tbm`: counts[(y, cam)] entries (default 0), row starts `gap` entries apart from the end of the row before"""
    rng = np.random.default_rng(seed)
    rowA, rowcnt = np.zeros(S * N, np.int32), np.zeros(S * N, np.int32)
    at = 0
    for y in range(S):
        for cam in tbm:
            n = counts(y, cam)
            rowA[y * N + cam], rowcnt[y * N + cam] = at, n
            at += n + gap
    metaA = np.full((at, 2), 0xdeadbeef, np.uint32)          # (what lies in the gaps must never be moved)
    depthsA = fresh_depths(at)
    for y in range(S):
        for cam in tbm:
            a, n = rowA[y * N + cam], rowcnt[y * N + cam]
            metaA[a:a + n, 0] = np.sort(rng.choice(5000, n, replace=False))
            metaA[a:a + n, 1] = cam
    return rowA, metaA, depthsA, rowcnt


def make(name, views, counts=lambda y, cam: 0, gap=0, overflowed=None, **about):
    k = len(views) - 1
    v = views[k]
    N = len(v["l2g"])
    rowA, metaA, depthsA, rowcnt = stage1(v["S"], N, v["tbm"].tolist(), counts, gap, len(name))
    case = dict(name=name, views=views, k=k, overflowed=overflowed, rowA=rowA, metaA=metaA, depthsA=depthsA, rowcnt=rowcnt, about=about)
    check_preconditions(case)
    return case


def check_preconditions(case):
    views, k = case["views"], case["k"]
    v = views[k]
    N = len(v["l2g"])
    assert v["n_tbm"] > 0 and not set(v["tbm"].tolist()) & set(v["source_cam"].tolist())         # sources and cameras to be matched are disjoint
    assert len(set(v["source_cam"].tolist())) == len(v["source_cam"]) and all(0 <= si < k for si in v["source_index"])    # sources come earlier in the chain
    for cam, si in zip(v["source_cam"], v["source_index"]):
        w = views[si]
        assert 0 <= cam < N
        r = w["kept"]
        key = r["segID1"].astype(np.int64) * 256 + np.array([w["l2g"].tolist().index(c) for c in r["camID2"]], np.int64)
        assert np.all(np.diff(key) >= 0)                                                            # a kept list is in (segment, camera) order
        mine = r[r["camID2"] == v["id"]]
        pair = mine["segID2"].astype(np.int64) * (1 << 20) + mine["segID1"]
        assert len(np.unique(pair)) == len(pair)                                                    # targets are distinct inside a run
    for w in views[:k]:
        assert w["n_tbm"] > 0 or len(w["kept"]) == 0


def fillers(rng, w, n, avoid_cam):
    """n records of view w towards cameras other than `avoid_cam` (None: any)"""
    cams = [q for q in range(len(w["l2g"])) if q != avoid_cam]
    return [(int(rng.integers(0, w["S"])), int(cams[rng.integers(0, len(cams))]), int(rng.integers(0, 300))) for _ in range(n)] if cams and w["S"] else []


CASES = {}


def _add(case):
    assert case["name"] not in CASES
    CASES[case["name"]] = case


# ---- run lengths: one source whose list holds runs of every length towards view 9 (its local camera 1), targets = distinct source segments
def _run_lengths():
    rng = np.random.default_rng(1)
    S = len(RUN_LENGTHS) + 1
    src = view(4, 1024, [70, 9, 80, 90], tbm=[0])
    t = []
    for y, n in enumerate(RUN_LENGTHS):
        t += [(int(s), 1, y) for s in rng.choice(1024, n, replace=False)]
    t += [(5, 1, S - 1), (900, 1, S + 3)]                     # one more run of 1, and a record aimed past the view's segments: dropped by count and place alike
    t += fillers(rng, src, 700, 1)
    src["kept"] = kept_list(src, t)
    for i, bits in zip(np.flatnonzero(src["kept"]["camID2"] == 9)[:3], SPECIAL_DEPTH_BITS):     # depths that must travel as bytes
        src["kept"]["depths"].view(np.uint32)[i, 1] = bits
    me = view(9, S, [4, 50, 51, 52], tbm=[1, 3], sources=[(0, 0)])
    sizes = {0: 0, 1: 1, 2: 64, 3: 65}
    return make("run_lengths", [src, me], counts=lambda y, cam: sizes.get(y, 3) if cam == 1 else (y * 5) % 7, gap=3, runs=list(RUN_LENGTHS) + [1])


_add(_run_lengths())


# ---- a source's segments against the 16 chunks of the run-table count; sources with more and with fewer segments than the view
def _source_sizes():
    rng = np.random.default_rng(2)
    sizes = (1, 5, 16, 17, 100)
    S = 40
    views = []
    for i, Sw in enumerate(sizes):
        w = view(10 + i, Sw, [200 + i, 99, 300 + i], tbm=[0])
        t = [(int(rng.integers(0, Sw)), 1, int(rng.integers(0, S))) for _ in range(60)] + [(Sw - 1, 1, 0), (0, 1, S - 1)] + fillers(rng, w, 40, 1)
        w["kept"] = kept_list(w, t)
        views.append(w)
    me = view(99, S, [10, 11, 12, 13, 14, 500, 501], tbm=[5, 6], sources=[(i, i) for i in range(5)])
    return make("source_segment_counts", views + [me], counts=lambda y, cam: (y + cam) % 3, source_S=list(sizes))


_add(_source_sizes())


# ---- the largest view: 16384 segments, the largest dynamic LDS request of the run-table count; records aimed at its first and last segment
def _largest_view():
    w = view(1, 50, [2, 3], tbm=[1])
    w["kept"] = kept_list(w, [(0, 0, 0), (3, 0, 16383), (7, 0, 16383), (7, 0, 0), (9, 1, 5), (49, 0, 8000)])
    me = view(2, 16384, [1, 3], tbm=[1], sources=[(0, 0)])
    return make("largest_view", [w, me], counts=lambda y, cam: 1 if y in (0, 4095, 4096, 16383) else 0, S=16384)


_add(_largest_view())


# ---- sources that must contribute nothing, beside one that does
def _odd_sources():
    rng = np.random.default_rng(4)
    S = 12
    empty = view(20, 30, [77, 21], tbm=[1])                                   # verified, keeps nothing
    unverified = view(21, 30, [77, 20])                                       # never verified: no list, no run table
    over = view(22, 30, [77, 20], tbm=[0])                                    # overflow set in its result record: its records stay unread
    over["kept"] = kept_list(over, [(int(rng.integers(0, 30)), 0, int(rng.integers(0, S))) for _ in range(50)])
    stranger = view(23, 30, [20, 21], tbm=[0])                                # does not list view 77: slot -1
    stranger["kept"] = kept_list(stranger, fillers(rng, stranger, 40, None))
    good = view(24, 30, [20, 77], tbm=[0])
    good["kept"] = kept_list(good, [(int(rng.integers(0, 30)), 1, int(rng.integers(0, S))) for _ in range(40)] + [(3, 1, S), (4, 1, 65535)] + fillers(rng, good, 30, 1))
    me = view(77, S, [20, 21, 22, 23, 24, 600], tbm=[5], sources=[(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)])
    return make("sources_that_give_nothing", [empty, unverified, over, stranger, good, me], counts=lambda y, cam: y % 4, overflowed=[0, 0, 1, 0, 0, 0])


_add(_odd_sources())


# ---- list lengths against the 8192 records of one pass at the fewest workgroups per source
def _list_lengths():
    rng = np.random.default_rng(5)
    S = 64
    views = []
    for i, n in enumerate((MIN_BPS_RECORDS - 1, MIN_BPS_RECORDS, MIN_BPS_RECORDS + 1)):
        w = view(30 + i, 300, [41, 42, 40], tbm=[0])
        last = (299, 2, S - 1)                                  # the last record of the list points at the view
        t = set()
        while len(t) < n - 1:
            need = n - 1 - len(t)
            t |= {(int(a), int(b), int(c)) for a, b, c in zip(rng.integers(0, 300, need), rng.integers(0, 3, need), rng.integers(0, S, need))} - {last}
        w["kept"] = kept_list(w, sorted(t) + [last])
        assert len(w["kept"]) == n
        views.append(w)
    me = view(40, S, [30, 31, 32, 700], tbm=[3], sources=[(0, 0), (1, 1), (2, 2)])
    return make("list_lengths", views + [me], counts=lambda y, cam: 2, lengths=[MIN_BPS_RECORDS - 1, MIN_BPS_RECORDS, MIN_BPS_RECORDS + 1])


_add(_list_lengths())


# ---- neighbour counts; the source's camera is the last one
def _neighbours(N):
    rng = np.random.default_rng(60 + N)
    S = 9
    if N == 1:
        return make("neighbours_1", [view(5, S, [6], tbm=[0])], counts=lambda y, cam: y % 3, N=1)
    w = view(1, 20, [2, 3], tbm=[1])
    w["kept"] = kept_list(w, [(int(rng.integers(0, 20)), 0, int(rng.integers(0, S))) for _ in range(30)] + fillers(rng, w, 10, 0))
    l2g = [1000 + q for q in range(N - 1)] + [1]
    return make("neighbours_%d" % N, [w, view(2, S, l2g, tbm=list(range(0, N - 1, max(1, N // 8))), sources=[(N - 1, 0)])], counts=lambda y, cam: (y + cam) % 2, N=N)


for _N in (1, 2, 24, 255):
    _add(_neighbours(_N))


# ---- S x N against the tiles of the row scan, with counts in front of every seam
def _tiles(S, N):
    rng = np.random.default_rng(S * N)
    if N == 1:
        return make("rows_%d" % (S * N), [view(5, S, [6], tbm=[0])], counts=lambda y, cam: 1 + y % 3, rows=S * N)
    w = view(1, 64, [2, 3], tbm=[1])
    tg = [0, S - 1, min(S - 1, TILE // N), min(S - 1, TILE // N + 1), min(S - 1, 2 * TILE // N)]
    w["kept"] = kept_list(w, [(int(rng.integers(0, 64)), 0, int(rng.integers(0, S))) for _ in range(400)] + [(int(s), 0, int(t)) for t in tg for s in range(3)])
    l2g = [1] + [2000 + q for q in range(N - 1)]
    return make("rows_%d" % (S * N), [w, view(2, S, l2g, tbm=[N - 1], sources=[(0, 0)])], counts=lambda y, cam: 1 + y % 3, rows=S * N)


for _S, _N in ((1, 1), (1365, 3), (2048, 2), (241, 17), (8191, 1), (2731, 3)):
    _add(_tiles(_S, _N))
