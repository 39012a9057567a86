"""The crafted cases of tests/keptwrite_cases.py against the numbers they are made for, and the two halves of tests/keptwrite_model.py against each
other -- no device.  Also the host rule that turns option rt_g into the lanes per run of the chain's run-table route (l3d_test_rt_lanes), held to a
table: the two kernels that take it (k_exist_count_rt, k_place_rt) cut their workgroups into 1024 / g and 256 / g groups and step their segment
loops by that number, so anything but a power of two up to 64 must never reach them."""
import numpy as np
import pytest

import keptwrite_cases as kc
import keptwrite_model as km


def test_writer_cases_are_well_formed():
    for name, c in kc.CASES.items():
        S, N, rs = c["S"], c["N"], c["row_start"]
        assert rs.shape == (S * N + 1,) and rs[0] == 0 and (np.diff(rs) >= 0).all(), name
        R = int(rs[-1])
        assert c["meta"].shape == (R, 2) and c["depths"].shape == (R, 4) and c["conf"].shape == (R,) and len(set(c["l2g"].tolist())) == N, name
        for row in range(S * N):
            m = c["meta"][rs[row]:rs[row + 1]]
            assert (m[:, 1] == row % N).all() and (np.diff(m[:, 0].astype(np.int64)) > 0).all() and (m[:, 0] < 65536).all(), (name, row)
        assert len(np.unique(c["depths"].view(np.uint32))) == R * 4, name          # every depth its own bit pattern
        assert c["l2g"].tolist() != sorted(c["l2g"].tolist()) or N == 1, name     # (the rebuild has to map ids back to local numbers)


def test_writer_cases_hold_the_numbers_they_are_for():
    C = kc.CASES
    sizes = lambda c: [int(c["row_start"][(y + 1) * c["N"]] - c["row_start"][y * c["N"]]) for y in range(c["S"])]
    for name in ("sizes_none_kept", "sizes_all_kept", "sizes_alternating", "sizes_only_the_last", "sizes_first_of_the_second_round"):
        assert sizes(C[name]) == [0, 1, 63, 64, 65, 2047, 2048, 2049, 4097] == C[name]["about"]["sizes"]
        assert int(km.kept_counts(C[name]).sum()) == C[name]["about"]["kept"], name
    assert kc.ROUND == 2048 and km.kept_counts(C["sizes_first_of_the_second_round"]).tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1]
    assert km.kept_counts(C["sizes_only_the_last"]).tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1]
    # depths: -0.0, a denormal, NaN payloads
    bits = set(C["sizes_all_kept"]["depths"].view(np.uint32).reshape(-1).tolist())
    assert set(kc.SPECIAL_DEPTH_BITS) <= bits
    # confidences around 1
    c = C["confidence_edges"]
    assert c["conf"][0] == 1.0 and c["conf"][1].view(np.uint32) == 0x3f800001 and c["conf"][2] == 2.0 and np.isnan(c["conf"][3])
    w = km.writer(c, arena_cap=3)
    assert w["n_kept"] == 3 and w["records"]["confidence"].view(np.uint32).tolist() == [0x3f000001, 0x3f800000, 0x3f000002]      # c / 2, bit for bit
    assert w["records"]["segID2"].tolist() == [c["meta"][i, 0] for i in (1, 2, 4)] and w["records"]["camID2"].tolist() == [c["l2g"][q] for q in (0, 0, 1)]
    # best positions
    for name in ("best_tie_first_wins", "best_in_the_second_round"):
        c = C[name]
        w = km.writer(c, arena_cap=int(km.kept_counts(c).sum()))
        assert w["best_pos"].tolist() == c["about"]["best"], name
        top = w["records"]["confidence"].max()
        assert (w["records"]["confidence"] == top).sum() >= 2 and w["records"]["confidence"][w["best_pos"][0]] == top      # a tie, and the first of it
    c = C["best_in_the_second_round"]
    assert np.flatnonzero(c["conf"] == 3.0)[0] >= kc.ROUND and np.nanmax(c["conf"][:kc.ROUND]) == 2.5
    # run tables: the camera chunks of 64, cameras and a segment without kept matches
    assert [C[n]["N"] for n in C if n.startswith("run_table_N")] == [1, 63, 64, 65, 128, 255]
    for n in C:
        if n.startswith("run_table_N"):
            c = C[n]
            w = km.writer(c, arena_cap=int(km.kept_counts(c).sum()))
            assert (w["rt"][:, 2] == w["rt"][0, 2]).all() and w["rt"][0, 2] == w["rt"][c["N"], 1]          # the segment without candidates: all rows equal
            if c["N"] > 1:
                assert (w["rt"][1] == w["rt"][2]).all() and (w["rt"][0] < w["rt"][1])[[0, 1, 3, 4]].all()  # camera 1 keeps nothing, camera 0 does
    assert [C[n]["S"] for n in C if n.startswith("segments_")] == [0, 1, 255, 256, 257, 600]


def test_result_record_of_the_model():
    c = kc.CASES["segments_257"]
    total, R = int(km.kept_counts(c).sum()), int(c["row_start"][-1])
    w = km.writer(c, arena_cap=total)
    assert (w["kept_base"], w["n_kept"], w["R"], w["overflow"], w["n_want"]) == (0, total, R, 0, 0)
    w = km.writer(c, prev=(5, 3), arena_cap=8 + total)
    assert (w["kept_base"], w["n_kept"], w["overflow"]) == (8, total, 0) and w["records"][:8].tobytes() == b"\xff" * 256 and w["records"]["segID1"][8] == 0
    w = km.writer(c, prev=(5, 3), arena_cap=8 + total - 1)
    assert (w["kept_base"], w["n_kept"], w["overflow"], w["n_want"]) == (8, 0, 2, total) and w["records"].tobytes() == b"\xff" * (32 * (7 + total))
    assert (w["rt"] == -1).all() and (w["best_pos"] == km.BESTPOS_CANARY).all()
    w = km.writer(c, cand_cap=R - 1, arena_cap=total)
    assert (w["n_kept"], w["overflow"], w["n_want"]) == (0, 1, 0)


def test_the_rebuild_model_agrees_with_the_writer_model():
    for name, c in kc.CASES.items():
        total = int(km.kept_counts(c).sum())
        w = km.writer(c, arena_cap=total)
        qt, rt, err = km.rebuild(w["records"], c["S"], c["l2g"])
        assert err == 0 and np.array_equal(qt, w["side"]) and np.array_equal(rt, w["rt"]), name
        # and the run table against a count over the records
        local = {int(g): q for q, g in enumerate(c["l2g"])}
        for y in range(c["S"]):
            mine = [(i, local[int(r["camID2"])]) for i, r in enumerate(w["records"]) if r["segID1"] == y] if c["S"] <= 9 else None
            if mine is not None:
                for q in range(c["N"] + 1):
                    assert rt[q, y] == int((w["records"]["segID1"] < y).sum()) + sum(1 for _, cam in mine if cam < q), (name, y, q)


def test_lists_for_the_rebuild():
    assert [len(l["records"]) for l in kc.GOOD_LISTS] == [0, 1, 64, 65, 1025]
    for l in kc.GOOD_LISTS:
        assert km.rebuild(l["records"], l["S"], l["l2g"])[2] == 0
    where = {"descent_inside_a_wave": 11, "descent_across_63_64": 64, "descent_across_255_256": 256, "descent_across_the_grid_stride": 512,
             "descent_across_the_seam_pass_stride": 16384}
    for name, l in kc.BAD_LISTS.items():
        qt, rt, err = km.rebuild(l["records"], l["S"], l["l2g"])
        assert err == 1, name
        local = {int(g): q for q, g in enumerate(l["l2g"])}
        key = [(int(r["segID1"]) << 8) | local.get(int(r["camID2"]), 0xff) for r in l["records"]]
        down = [i for i in range(1, len(key)) if key[i - 1] > key[i]]
        if name in where:
            assert down == [where[name]], (name, down)
        else:
            assert int((qt >> 16 == 0xffff).sum()) == 1 and len(down) <= 1
    # the strides the last two descents are meant for: the pass over the records runs (n + 1023) / 1024 workgroups of 256 threads per job (at most 512),
    # the seam pass looks at every 64th boundary with 256 threads per workgroup
    assert (len(kc.BAD_LISTS["descent_across_the_grid_stride"]["records"]) + 1023) // 1024 * 256 == 512
    assert len(kc.BAD_LISTS["descent_across_the_seam_pass_stride"]["records"]) > 256 * 64 == 16384


RT_LANES = [   # option rt_g, average run -> lanes per run
    (-1, 0.0, 1), (-1, 1.0, 1), (-1, 1.5, 2), (-1, 2.0, 2), (-1, 2.01, 4), (-1, 33.0, 64), (-1, 64.0, 64), (-1, 1e9, 64), (-1, float("inf"), 64),
    (-2, 5.0, 8), (-(1 << 31), 5.0, 8),                                          # any negative value: the rule by the average run
    (0, 1e9, 1), (0, 0.0, 1),                                                    # 0: a run per thread, as the option says
    (1, 50.0, 1), (2, 50.0, 2), (3, 50.0, 2), (4, 0.0, 4), (5, 0.0, 4), (7, 0.0, 4), (8, 0.0, 8), (31, 0.0, 16), (32, 0.0, 32), (63, 0.0, 32), (64, 0.0, 64),
    (65, 0.0, 64), (100, 0.0, 64), (256, 0.0, 64), (257, 0.0, 64), (512, 0.0, 64), (1024, 0.0, 64), (1025, 0.0, 64), (1 << 30, 0.0, 64), ((1 << 31) - 1, 0.0, 64),
]


def test_lanes_per_run_are_a_power_of_two_up_to_64():
    from line3d_amd import capi
    for opt, avg, want in RT_LANES:
        assert capi.rt_lanes(opt, avg) == want, (opt, avg)
    rng = np.random.default_rng(3)
    for opt in list(range(-3, 1100)) + rng.integers(-2 ** 31, 2 ** 31 - 1, 2000).tolist():
        for avg in (0.0, 0.3, 17.0, 1e30, float("nan")):
            g = capi.rt_lanes(opt, avg)
            assert g in (1, 2, 4, 8, 16, 32, 64) and 256 % g == 0 and 1024 % g == 0 and 256 // g > 0, (opt, avg, g)
            if opt > 0:
                assert g <= opt and (g == 64 or 2 * g > opt)         # rounded down
