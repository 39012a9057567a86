"""Crafted verified candidates for the chains' kept writer (write_kept_segment_wg, l3d_kept.hpp; k_kept_write_chain, l3d_chain.hip) and crafted lists for
the rebuild of side words and run tables (l3d_chain_common.hip), one case per edge of the code: the writer's rounds of 2048 candidates and chunks of 64,
the 64-camera chunks of the run-table prefix, the 256-thread sum of the kept counts in front of a segment, the best position's tie rule, the two
overflow bits of the result record; the rebuild's order check inside a wave, across waves, across workgroups and across the grid stride.  Every case
is made from those numbers, seeded, never from device output.  tests/test_keptwrite_cases_cpu.py holds each case to what its name claims,
tests/test_gpu_kept_write.py runs them.

A writer case: name, S, N, row_start (S*N + 1), meta (R, 2: target, local camera), depths (R, 4), conf (R), l2g (N) and `about` (the numbers the CPU
test checks).  Inside a segment the candidates are in (camera, target) order, targets distinct inside a row -- what the verification hands the writer."""
import numpy as np

from keptwrite_model import MATCH_DTYPE

ROUND = 2048                # candidates per round of the writer
CHUNK = 64                  # candidates per ballot
ONE_UP = np.nextafter(np.float32(1.0), np.float32(2.0))
KEPT_VALUES = np.array([ONE_UP, 2.0, 1.5, np.nextafter(np.float32(2.0), np.float32(1.0))], np.float32)     # all below the 3.0 of a crafted maximum
DROPPED_VALUES = np.array([1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 0.0, -1.0, np.nan, 0.5], np.float32)
SPECIAL_DEPTH_BITS = (0x80000000, 0x00000001, 0x7fc00123, 0xffc00001, 0x7f800000)      # -0.0, the smallest denormal, two NaN payloads, +inf


def make(name, N, rows, keep, conf_at=None, **about):
    """rows: (S, N) candidates per row; keep: (R,) bool or a function of (segment, index in the segment, segment size)"""
    rows = np.asarray(rows, np.int64).reshape(-1, N)
    S = len(rows)
    row_start = np.concatenate([[0], np.cumsum(rows.reshape(-1))]).astype(np.int32)
    R = int(row_start[-1])
    meta = np.zeros((R, 2), np.uint32)
    seg_of, idx_in_seg = np.zeros(R, np.int64), np.zeros(R, np.int64)
    for y in range(S):
        a = row_start[y * N]
        for q in range(N):
            b, e = row_start[y * N + q], row_start[y * N + q + 1]
            meta[b:e, 0] = (np.arange(e - b) * 3 + (y + q) % 3) % 65536           # ascending, distinct inside the row
            meta[b:e, 1] = q
        e = row_start[(y + 1) * N]
        seg_of[a:e], idx_in_seg[a:e] = y, np.arange(e - a)
    if callable(keep):
        sizes = rows.sum(axis=1)
        keep = np.array([bool(keep(int(seg_of[i]), int(idx_in_seg[i]), int(sizes[seg_of[i]]))) for i in range(R)], bool)
    keep = np.asarray(keep, bool)
    assert keep.shape == (R,)
    conf = np.where(keep, KEPT_VALUES[np.arange(R) % len(KEPT_VALUES)], DROPPED_VALUES[np.arange(R) % len(DROPPED_VALUES)]).astype(np.float32)
    for i, v in (conf_at or {}).items():
        conf[i] = np.float32(v)
    bits = (0x3f800000 + 17 * np.arange(R * 4, dtype=np.uint64)).astype(np.uint32)      # distinct bit patterns, record by record
    for k, b in enumerate(SPECIAL_DEPTH_BITS):
        if R * 4 > 5 * k + 3:
            bits[5 * k + 3] = b
    assert len(np.unique(bits)) == len(bits)
    l2g = np.arange(N, dtype=np.uint32)[::-1] * 5 + 11                    # distinct ids, not in local order
    return dict(name=name, S=S, N=N, row_start=row_start, meta=meta, depths=bits.view(np.float32).reshape(R, 4), conf=conf, l2g=l2g.astype(np.uint32), about=about)


def split_rows(sizes, N, seed):
    """segment sizes -> (S, N) row counts that sum to them, unevenly, some rows empty"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((len(sizes), N), np.int64)
    for y, m in enumerate(sizes):
        cuts = np.sort(rng.integers(0, m + 1, N - 1)) if N > 1 else np.zeros(0, np.int64)
        rows[y] = np.diff(np.concatenate([[0], cuts, [m]]))
    return rows


SEGMENT_SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 4097]
CASES = {}


def _add(case):
    assert case["name"] not in CASES
    CASES[case["name"]] = case


_rows = split_rows(SEGMENT_SIZES, 3, 1)
_add(make("sizes_none_kept", 3, _rows, lambda y, i, m: False, sizes=SEGMENT_SIZES, kept=0))
_add(make("sizes_all_kept", 3, _rows, lambda y, i, m: True, sizes=SEGMENT_SIZES, kept=sum(SEGMENT_SIZES)))
_add(make("sizes_alternating", 3, _rows, lambda y, i, m: i % 2 == 1, sizes=SEGMENT_SIZES, kept=sum(m // 2 for m in SEGMENT_SIZES)))
_add(make("sizes_only_the_last", 3, _rows, lambda y, i, m: i == m - 1, sizes=SEGMENT_SIZES, kept=sum(1 for m in SEGMENT_SIZES if m)))
_add(make("sizes_first_of_the_second_round", 3, _rows, lambda y, i, m: i == ROUND, sizes=SEGMENT_SIZES, kept=sum(1 for m in SEGMENT_SIZES if m > ROUND)))

# confidences: exactly 1.0 is dropped, the next float is kept; the written confidence is half of it, bit for bit
_add(make("confidence_edges", 2, [[3, 3]], [False, True, True, False, True, False],
          conf_at={0: 1.0, 1: ONE_UP, 2: 2.0, 3: np.nan, 4: np.float32(1.0000002), 5: np.nextafter(np.float32(1.0), np.float32(0.0))}, kept=3))

# best position: the first of several equal maxima; a maximum in the second round behind a smaller one in the first; no kept match
_add(make("best_tie_first_wins", 2, [[40, 60], [0, 0], [5, 0]], lambda y, i, m: y == 0 and i % 7 == 3,
          conf_at={10: 3.0, 17: 3.0, 94: 3.0}, best=[1, -1, -1]))
_add(make("best_in_the_second_round", 1, [[3000]], lambda y, i, m: i % 100 == 7, conf_at={7: 2.5, 2507: 3.0, 2907: 3.0}, best=[25]))

# the run table's camera chunks of 64: N at and around them, every other camera without a kept match, a segment without candidates in the middle
for _N in (1, 63, 64, 65, 128, 255):
    _r = np.full((5, _N), 2, np.int64)
    _r[2] = 0
    _r[:, 1::3] = 0
    _add(make("run_table_N%d" % _N, _N, _r, lambda y, i, m: i % 4 < 2, cams=_N))

# the sum of the kept counts in front of a segment: 256 threads stride over the segments
for _S in (0, 1, 255, 256, 257, 600):
    _rng = np.random.default_rng(100 + _S)
    _add(make("segments_%d" % _S, 2, _rng.integers(0, 4, (_S, 2)), lambda y, i, m: (y * 7 + i * 3) % 5 < 3, segs=_S))


# ---- lists for the rebuild
def ordered_list(n, S, N, seed):
    """n records in (segment, local camera) order, cameras as GLOBAL ids of a neighbour list that is not in id order"""
    rng = np.random.default_rng(seed)
    l2g = (rng.permutation(N).astype(np.uint32) * 3 + 100)
    key = np.sort(rng.integers(0, S * N, n)) if n else np.zeros(0, np.int64)
    recs = np.zeros(n, MATCH_DTYPE)
    recs["segID1"], recs["camID2"] = key // N, l2g[key % N] if n else 0
    recs["segID2"] = rng.integers(0, 65536, n)
    recs["depths"] = rng.random((n, 4), dtype=np.float32)
    recs["confidence"] = 0.75
    return dict(records=recs, S=S, l2g=l2g)


def with_descent(lst, i):
    """one descent of the (segment, camera) order exactly between records i - 1 and i: record i - 1 moves to the last segment"""
    recs = lst["records"].copy()
    assert 0 < i < len(recs) and recs["segID1"][i] < lst["S"] - 1
    recs["segID1"][i - 1] = lst["S"] - 1
    return dict(lst, records=recs)


def with_stranger(lst, i):
    recs = lst["records"].copy()
    recs["camID2"][i] = 999999
    return dict(lst, records=recs)


GOOD_LISTS = [ordered_list(n, S, N, 40 + n) for n, S, N in ((0, 3, 2), (1, 1, 1), (64, 9, 4), (65, 300, 24), (1025, 40, 255))]
_base = ordered_list(1100, 400, 6, 7)          # two workgroups per job of the pass over the records: a stride of 512
_long = ordered_list(16500, 2000, 3, 8)        # the seam pass of one workgroup strides 256 x 64 = 16384 records
BAD_LISTS = {
    "camera_is_no_neighbour": with_stranger(_base, 500),
    "descent_inside_a_wave": with_descent(_base, 11),
    "descent_across_63_64": with_descent(_base, 64),
    "descent_across_255_256": with_descent(_base, 256),
    "descent_across_the_grid_stride": with_descent(_base, 512),
    "descent_across_the_seam_pass_stride": with_descent(_long, 16384),
}
