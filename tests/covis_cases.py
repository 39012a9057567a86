"""Named sets of world point lists for the co-visibility counting (l3d_covisibility): the smallest shapes at which it can go wrong.
CASES[name] = dict(lists=[uint32 array per view, in add order], tile=L3D_COVIS_TILE for the device run (0: automatic), repeats=a list names an id
twice, claim=what the name promises, as a predicate on the lists).  Everything is built once, at import, from fixed seeds."""
import numpy as np

CASES = {}


def _tracks(lists):
    """{point id: sorted list of the distinct views naming it}"""
    t = {}
    for v, l in enumerate(lists):
        for p in np.unique(np.asarray(l, np.uint32)).tolist():
            t.setdefault(p, []).append(v)
    return t


def track_lengths(lists):
    return sorted(len(v) for v in _tracks(lists).values())


def _has_repeat(lists):
    return any(len(np.unique(l)) != len(l) for l in lists)


def _case(name, lists, claim, tile=0, repeats=False):
    lists = [np.ascontiguousarray(l, dtype=np.uint32).reshape(-1) for l in lists]
    assert name not in CASES
    CASES[name] = dict(lists=lists, tile=tile, repeats=repeats, claim=claim)


def _from_tracks(n_views, tracks):
    """tracks: iterable of (point id, views) -> one list per view, ids in the order given"""
    lists = [[] for _ in range(n_views)]
    for p, views in tracks:
        for v in views:
            lists[v].append(p)
    return lists


# ---- track lengths --------------------------------------------------------------------------------------------------------------------------
_case("track_lengths_1_2_3_4", _from_tracks(4, [(10, [0]), (11, [0, 1]), (12, [0, 1, 2]), (13, [0, 1, 2, 3]), (14, [3]), (15, [2, 3])]),
      lambda ls: track_lengths(ls) == [1, 1, 2, 2, 3, 4])
_case("one_point_in_all_70_views", _from_tracks(70, [(7, list(range(70)))] + [(100 + v, [v]) for v in range(70)]),
      lambda ls: len(ls) == 70 and track_lengths(ls)[-1] == 70 and track_lengths(ls)[:-1] == [1] * 70)
_case("tracks_of_63_64_65", _from_tracks(65, [(1, list(range(63))), (2, list(range(64))), (3, list(range(65)))]),
      lambda ls: track_lengths(ls) == [63, 64, 65])

# ---- views and their lists ------------------------------------------------------------------------------------------------------------------
_case("empty_list_view", _from_tracks(5, [(1, [0, 1, 3]), (2, [0, 3, 4]), (3, [1, 4])]),
      lambda ls: len(ls[2]) == 0 and all(len(l) for i, l in enumerate(ls) if i != 2))
_case("short_tracks_only_view", _from_tracks(5, [(1, [0, 1, 2]), (2, [0, 1, 2, 3]), (3, [4]), (4, [3, 4]), (5, [0, 4])]),
      lambda ls: len(ls[4]) == 3 and all(len(_tracks(ls)[int(p)]) < 3 for p in ls[4]))
_case("one_view", [[5, 6, 7]], lambda ls: len(ls) == 1)
_case("three_views", _from_tracks(3, [(1, [0, 1, 2]), (2, [0, 1, 2]), (3, [0, 2]), (4, [1])]), lambda ls: len(ls) == 3 and 3 in track_lengths(ls))
_case("four_views", _from_tracks(4, [(1, [0, 1, 2]), (2, [1, 2, 3]), (3, [0, 1, 2, 3]), (4, [0, 3])]), lambda ls: len(ls) == 4 and 4 in track_lengths(ls))


def _random_scene(seed, n_views, n_points, max_len, shuffle):
    rng = np.random.default_rng(seed)
    ids = rng.choice(1 << 20, n_points, replace=False).astype(np.uint32)
    lists = [[] for _ in range(n_views)]
    for p in ids.tolist():
        for v in rng.choice(n_views, int(rng.integers(1, max_len + 1)), replace=False).tolist():
            lists[v].append(p)
    lists = [np.asarray(l, np.uint32) for l in lists]
    return [l[rng.permutation(len(l))] for l in lists] if shuffle else lists


_case("arbitrary_order_within_a_view", _random_scene(11, 9, 400, 6, True),
      lambda ls: any(np.any(np.diff(l.astype(np.int64)) < 0) for l in ls) and any(np.any(np.diff(l.astype(np.int64)) > 0) for l in ls))


def _big_view():
    big = np.arange(200000, dtype=np.uint32)
    return [big, np.arange(0, 50000, 7, dtype=np.uint32), np.arange(0, 70000, 5, dtype=np.uint32), np.arange(0, 200000, 35, dtype=np.uint32)[::-1].copy(),
            np.array([3, 35, 199999], np.uint32)]


_case("one_view_of_200000_observations", _big_view(), lambda ls: len(ls[0]) == 200000 and max(len(l) for l in ls[1:]) < 20000)

# ---- point ids: all 32 bits count -----------------------------------------------------------------------------------------------------------
_case("point_ids_extremes_and_high_bits",
      _from_tracks(6, [(0, [0, 1, 2]), (1 << 31, [1, 2, 3]), ((1 << 32) - 1, [2, 3, 4, 5]), (0x00010001, [0, 2, 4]), (0x80010001, [1, 3, 5]), (0x40010001, [0, 5]),
                       (0xC0010001, [0, 3, 4, 5]), (1, [0, 1])]),
      lambda ls: {0, 1 << 31, (1 << 32) - 1, 0x00010001, 0x80010001} <= set(_tracks(ls)))

# ---- counter width --------------------------------------------------------------------------------------------------------------------------
_case("two_views_share_70000_points", [np.arange(70000, dtype=np.uint32)] * 3 + [np.array([1, 2], np.uint32)],
      lambda ls: len(np.intersect1d(ls[0], ls[1])) == 70000 and track_lengths(ls)[-1] == 4 and track_lengths(ls)[0] == 3)


# ---- tiling: rows that span tiles, a tile that is not full ------------------------------------------------------------------------------------
def _banded(seed, n_views, n_points, half_width):
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(n_views)]
    for p in range(n_points):
        c = int(rng.integers(0, n_views))
        for v in range(max(0, c - half_width), min(n_views, c + half_width + 1)):
            if v == c or rng.random() < 0.5:
                lists[v].append(1000 + p)
    for v in range(n_views):
        lists[v].append(5)                  # one point seen by every view: every row spans every tile
    return lists


_BANDED = _banded(23, 300, 2000, 40)
_case("tiling_300_views_tile_64", _BANDED, lambda ls: len(ls) == 300 and 300 % 64 != 0 and track_lengths(ls)[-1] == 300, tile=64)
_case("tiling_300_views_tile_100", _BANDED, lambda ls: len(ls) == 300 and track_lengths(ls)[-1] == 300, tile=100)

# ---- random scenes --------------------------------------------------------------------------------------------------------------------------
for _s in (101, 102, 103):
    _case("random_40_views_3000_points_seed_%d" % _s, _random_scene(_s, 40, 3000, 8, True), lambda ls: len(ls) == 40 and len(_tracks(ls)) == 3000)

# ---- repeated ids: the closed form does not hold, the function itself decides ------------------------------------------------------------------
# (before: the second view names the id twice -- its first mention takes the track to two views, its second finds `size() == 2`; after: the third view does)
_case("repeat_before_track_reaches_two_views", [[5, 9], [5, 9, 5], [5, 9, 11], [5, 11], [11, 9]],
      lambda ls: _has_repeat(ls[1:2]) and not _has_repeat(ls[:1]) and not _has_repeat(ls[2:]), repeats=True)
_case("repeat_after_track_reaches_two_views", [[5, 9], [5, 9], [9, 5, 11, 5], [5, 11], [11, 9]],
      lambda ls: _has_repeat(ls[2:3]) and not _has_repeat(ls[:2]) and not _has_repeat(ls[3:]), repeats=True)

NAMES = sorted(CASES)
