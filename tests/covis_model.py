"""Two references for the co-visibility counting, each -> (num_wps uint32 (V,), row_start int32 (V + 1,), col int32, count uint32): the non-zero
common_wps as a CSR over list indices, columns ascending.
  closed_form(lists)  the closed form, written from its statement: the incidence matrix of the tracks of three or more views
  replay(lists)       the literal bookkeeping: the oracle's restatement of Line3D::processWorldpointList, list after list in add order
reference(name) computes a case's reference once."""
import functools

import numpy as np

import covis_cases


def _csr(num, common):
    V = len(num)
    rows, cols = np.nonzero(common)                 # (row-major: columns ascend within a row)
    row_start = np.zeros(V + 1, np.int32)
    row_start[1:] = np.cumsum(np.bincount(rows, minlength=V))
    return num.astype(np.uint32), row_start, cols.astype(np.int32), common[rows, cols].astype(np.uint32)


def closed_form(lists):
    V = len(lists)
    points = np.unique(np.concatenate([np.asarray(l, np.uint32) for l in lists] + [np.zeros(0, np.uint32)]))
    M = np.zeros((len(points), V), np.int64)        # M[p, v] = 1: view v names point p
    for v, l in enumerate(lists):
        M[np.searchsorted(points, np.asarray(l, np.uint32)), v] = 1
    M = M[M.sum(axis=1) >= 3]                       # a track of fewer than three views counts nothing
    common = M.T @ M                                # ordered pairs (a, b) of a track's views ...
    np.fill_diagonal(common, 0)                     # ... with a != b
    return _csr(M.sum(axis=0), common)


def replay(lists):
    import l3d_oracle_pipeline as op
    o = object.__new__(op.OracleLine3D)             # (the bookkeeping alone: no library, no views)
    o.num_wps, o.common_wps, o.worldpoints2views = {}, {}, {}
    for v, l in enumerate(lists):
        o._process_worldpoints(v, [int(p) for p in l])
    V = len(lists)
    num = np.array([o.num_wps[v] for v in range(V)], np.int64).reshape(V)
    row_start, col, count = np.zeros(V + 1, np.int32), [], []
    for v in range(V):
        for n in sorted(o.common_wps.get(v, {})):
            col.append(n)
            count.append(o.common_wps[v][n])
        row_start[v + 1] = len(col)
    return num.astype(np.uint32), row_start, np.array(col, np.int32).reshape(-1), np.array(count, np.uint32).reshape(-1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case's expected result: the closed form where it holds, the replay where a list repeats an id"""
    case = covis_cases.CASES[name]
    out = replay(case["lists"]) if case["repeats"] else closed_form(case["lists"])
    for a in out:
        a.setflags(write=False)
    return out


def same(a, b):
    """the four arrays equal, element for element (integers: exactly)"""
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
