"""The case table of the co-visibility counting without a GPU: every case is what its name claims; the closed form (incidence matrix of the tracks of
three or more views) equals the literal replay of Line3D::processWorldpointList wherever no list repeats an id -- the derivation pinned against the
reference's restatement; and the library's host hook (l3d_test_covisibility_host: the product's own function on a scratch state) equals the replay on
every case, repeats included.  Integers, compared exactly.  The host code is clean under AddressSanitizer and UBSan as a stand-alone program
(tests/cpp/covis_asan.cpp), and the C++ facade's new members compile."""
import os
import subprocess

import numpy as np
import pytest

import covis_cases
import covis_model
from line3d_amd import capi


HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_REPLAY = {}


def _replay(name):
    if name not in _REPLAY:
        _REPLAY[name] = covis_model.replay(covis_cases.CASES[name]["lists"])
    return _REPLAY[name]


def test_table_covers_the_issue():
    names = " ".join(covis_cases.NAMES)
    for word in ("track_lengths_1_2_3_4", "all_70_views", "63_64_65", "empty_list", "short_tracks_only", "one_view", "three_views", "four_views", "arbitrary_order",
                 "200000", "high_bits", "70000", "tile_64", "tile_100", "seed_101", "seed_102", "seed_103", "repeat_before", "repeat_after"):
        assert word in names, word


@pytest.mark.parametrize("name", covis_cases.NAMES)
def test_case_is_what_its_name_claims(name):
    case = covis_cases.CASES[name]
    assert case["claim"](case["lists"])
    assert case["repeats"] == any(len(np.unique(l)) != len(l) for l in case["lists"])
    assert sum(len(l) for l in case["lists"]) < 2 ** 31


@pytest.mark.parametrize("name", [n for n in covis_cases.NAMES if not covis_cases.CASES[n]["repeats"]])
def test_closed_form_equals_replay(name):
    assert covis_model.same(covis_model.reference(name), _replay(name))


@pytest.mark.parametrize("name", [n for n in covis_cases.NAMES if covis_cases.CASES[n]["repeats"]])
def test_repeats_leave_the_closed_form(name):
    """what makes path 1 necessary: with a repeated id the function counts a view with itself, which the closed form never does"""
    num, row_start, col, count = _replay(name)
    rows = np.repeat(np.arange(len(num)), np.diff(row_start))
    assert np.any(rows == col)
    assert not covis_model.same(covis_model.closed_form(covis_cases.CASES[name]["lists"]), (num, row_start, col, count))


@pytest.mark.parametrize("name", covis_cases.NAMES)
def test_host_hook_equals_replay(name):
    got = capi.covisibility_host(covis_cases.CASES[name]["lists"])
    assert got[4] == 1, "the host hook always replays"
    assert covis_model.same(got, _replay(name))


def test_expected_values_of_the_small_cases():
    """a few counts by hand, so that the two references cannot agree on something wrong"""
    num, row_start, col, count = covis_model.reference("track_lengths_1_2_3_4")
    # tracks of three or more views: 12 in {0, 1, 2}, 13 in {0, 1, 2, 3}
    assert num.tolist() == [2, 2, 2, 1]
    dense = np.zeros((4, 4), np.int64)
    dense[np.repeat(np.arange(4), np.diff(row_start)), col] = count
    assert dense.tolist() == [[0, 2, 2, 1], [2, 0, 2, 1], [2, 2, 0, 1], [1, 1, 1, 0]]
    num, row_start, col, count = covis_model.reference("short_tracks_only_view")
    assert num[4] == 0 and row_start[4] == row_start[5]
    num, row_start, col, count = covis_model.reference("two_views_share_70000_points")
    assert count[0] == 70000 and num[0] == 70000
    num, row_start, col, count = covis_model.reference("one_view")
    assert num.tolist() == [0] and row_start.tolist() == [0, 0]


def test_host_hook_refusals():
    import ctypes as C
    lib = capi.load_library()
    out = [C.c_void_p() for _ in range(4)]
    path = C.c_int(0)
    ids = np.zeros(4, np.uint32)

    def call(ids_p, start, n_lists):
        s = np.ascontiguousarray(start, np.int64)
        return lib.l3d_test_covisibility_host(ids_p, capi._p(s), C.c_int(n_lists), *[C.byref(o) for o in out], C.byref(path))

    assert call(capi._p(ids), [0, 2 ** 31 - 1], 1) == 5     # L3D_ERR_UNSUPPORTED, too many observations: nothing is read
    assert call(capi._p(ids), [0, 3, 2], 2) != 0            # offsets descend
    assert call(capi._p(ids), [1, 3], 1) != 0               # do not start at 0
    assert call(None, [0, 3], 1) != 0                       # observations without ids
    assert lib.l3d_test_covisibility_host(capi._p(ids), None, C.c_int(1), *[C.byref(o) for o in out], C.byref(path)) != 0
    assert all(o.value is None for o in out)


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/covis_asan.cpp: l3d_covis.hpp -- Line3D::processWorldpointList on given tables and the replay of whole lists -- with a main of its own,
    built with AddressSanitizer and UBSan as a plain host program: random lists against a brute-force closed form, and lists with a repeated id"""
    exe = str(tmp_path / "covis_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "covis_asan.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 bad" in run.stdout, run.stdout + run.stderr


def test_facade_compiles(tmp_path):
    """Line3D::setDeviceCovisibility, getNeighbors and getViewSimilarities of include/line3D_amd.hpp"""
    src = tmp_path / "facade_covis.cpp"
    src.write_text('''#include "line3D_amd.hpp"
size_t use(L3D::Line3D& l)
{
    l.setDeviceCovisibility(true);
    l.compute3Dmodel(false);
    const std::vector<unsigned int> nb = l.getNeighbors(3);
    const std::map<unsigned int, float> sims = l.getViewSimilarities(3);
    return nb.size() + sims.size();
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
