"""The add family against its recorded table (tests/golden/add_table.json, taken by scripts/record_add_table.py on the commit named in the file,
before the add path became one route): every exported l3d_line3d_add_image* call, l3d_line3d_add_images with one and with three entries and
l3d_line3d_add_image_entry give the recorded code, message, number of cameras, data directory and statuses for every case of
tests/add_table_cases.py -- the refusals one by one, the cache rules, and pairs of causes that pin the order in which they are tested."""
import json
import os
import time

import pytest

import add_table_cases as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = [r for case in T.CASES for r in T.runs(case, with_entry=True)]
BY_NAME = {case["name"]: case for case in T.CASES}


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "add_table.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed(gpu_ctx, tmp_path_factory):
    """every run once, on one ordinary and one node object"""
    runner = T.Runner(os.path.join(HERE, "golden", "jpeg_ref.npz"), tmp_path_factory.mktemp("add_table"))
    t0 = time.time()
    try:
        got = {name + "/" + via: runner.run(BY_NAME[name], via) for name, via in RUNS}
    finally:
        runner.close()
    print("%d runs replayed in %.2f s" % (len(got), time.time() - t0))
    return got


def test_the_table_covers_every_entry_point_and_cause(table):
    assert len(table["commit"]) >= 7
    assert {T.entry_point_of(BY_NAME[name], via) for name, via in RUNS} == set(T.ENTRY_POINTS) and len(T.ENTRY_POINTS) == 13
    assert {c for case in T.CASES for c in case["causes"]} == set(T.CAUSES)
    recorded = {name + "/" + via for name, via in RUNS if via != "entry"}
    assert recorded == set(table["records"]), "the fixture and the case list differ"
    for name, via in RUNS:                                  # a tag is not enough: the recorded row has to show the cause
        if via != "entry":
            T.check_properties(BY_NAME[name], table["records"][name + "/" + via])


@pytest.mark.parametrize("name,via", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_add_table(table, replayed, name, via):
    want = T.expected_for_entry(BY_NAME[name], table["records"]) if via == "entry" else table["records"][name + "/" + via]
    got = replayed[name + "/" + via]
    print(got)
    assert got == want
