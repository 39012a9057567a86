"""The rules of matchViews sharded by blocks of views (l3d_blocks_rule.hpp, line3d_amd/csrc; DESIGN.md section 6, "The rule"), written from their
statement there: the blocks, how far a rank reaches and is checked, which ranks missed their speculation on a table of digests, whether the pass is
hopeless, the failure mark, and what every predecessor of a rank that missed hands over.  Pure arithmetic on lists -- no device.

A table is a list of W rows (one per rank) of n entries (hash, n_kept)."""

FAILURE_MARK = (2 ** 64 - 1, -1)


def begin(r, n, W):
    return n * r // W


def owner(k, n, W):
    return max(r for r in range(W) if begin(r, n, W) <= k)


def reach(window, neighbour_reach, partition):
    """-> (reach, tail, check)"""
    rch = max(window, neighbour_reach)
    return (rch, 2 * rch, max(window, 2 * rch)) if partition else (rch, 0, window)


def failed_rank(table):
    marked = [r for r, row in enumerate(table) if row[0] == FAILURE_MARK]
    return marked[0] if marked else -1


def verdict(table, n, W, check, tail, partition, comp_from):
    """-> dict(miss, first_diff, n_miss, hopeless)"""
    miss, first_diff, hopeless = [0] * W, [-1] * W, False
    for r in range(1, W):
        b = begin(r, n, W)
        lo = max(0, b - check)
        e = min(n, b + tail, begin(r + 1, n, W)) if partition else b
        never_computed = comp_from[r] > lo
        cannot_vouch = not partition and b - check < begin(r - 1, n, W)
        hopeless = hopeless or cannot_vouch
        if never_computed or cannot_vouch:
            miss[r] = 1
            continue
        differing = [k for k in range(lo, e) if table[r][k] != table[r - 1][k]]
        if differing:
            miss[r], first_diff[r] = 1, differing[0]
    return dict(miss=miss, first_diff=first_diff, n_miss=sum(miss), hopeless=hopeless)


def handover_plan(table, n, W, check, miss, verified, S_src):
    """-> dict(t_rec, t_seg, t_first, max_rec, max_seg), filed under the sender"""
    t_rec, t_seg, t_first = [0] * W, [0] * W, [-1] * W
    for r in range(1, W):
        if not miss[r]:
            continue
        s, b = r - 1, begin(r, n, W)
        handed = range(max(0, b - check), b)
        ver = [k for k in handed if verified[k]]
        t_rec[s] = sum(table[s][k][1] for k in handed)
        t_seg[s] = sum(S_src[k] for k in ver)
        t_first[s] = ver[0] if ver else -1
    return dict(t_rec=t_rec, t_seg=t_seg, t_first=t_first, max_rec=max(t_rec), max_seg=max(t_seg))
