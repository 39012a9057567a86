"""What Line3D::performMatching leaves behind (line3D.cc:834-884) for a schedule and its kept lists, in plain Python: dictionaries and sets, numpy
only for the records and the median.  It never calls into the library under test (tests/test_products_cases_cpu.py holds it to the oracle's
matching_commit + greedy_selection).

A case (tests/products_cases.py) is a dict: view_ids (ascending, the dense map), S (view id -> segments), chain (the chain views in processing
order, each a dict: id, S, l2g, n_tbm, source_cam, source_index, kept, R, best, bestpos -- what Context.test_products takes)."""
import math

import numpy as np

MATCH_DTYPE = np.dtype([("segID1", "<u4"), ("camID2", "<u4"), ("segID2", "<u4"), ("depths", "<f4", (4,)), ("confidence", "<f4")])
NO_MATCH = np.zeros((), MATCH_DTYPE)
NO_MATCH["segID1"] = 0xffffffff


def seg_base(case):
    base, acc = {}, 0
    for vid in case["view_ids"]:
        base[vid] = acc
        acc += case["S"][vid]
    return base, acc


def early_list(case, k):
    """cudawrapper.cu:877-878 / view.cc:200-224: the localized existing list of an early-return view -- what its sources pushed (line3D.cc:838-872),
    in push order, with the source's LOCAL camera number and confidence 0."""
    v = case["chain"][k]
    out = []
    for cam, si in zip(v["source_cam"], v["source_index"]):
        if si < 0 or si >= k or case["chain"][si]["n_tbm"] <= 0:        # (a source is a verified earlier view)
            continue
        for m in case["chain"][si]["kept"]:
            if int(m["camID2"]) != v["id"]:
                continue
            r = np.zeros((), MATCH_DTYPE)
            r["segID1"], r["camID2"], r["segID2"], r["confidence"] = m["segID2"], cam, m["segID1"], 0.0
            r["depths"] = (m["depths"][2], m["depths"][3], m["depths"][0], m["depths"][1])
            out.append(r)
    return out


def median_of(best):
    """cudawrapper.cu:1058-1076: both depths of every segment whose best.x != -1, sorted, element n // 2; -1.0 when there is none.  std::sort leaves
    the order of -0.0 and +0.0 open; the rule here: -0.0 first."""
    best = np.asarray(best, np.float32).reshape(-1, 2)
    vals = [float(x) for b in best if b[0] != np.float32(-1.0) for x in b]
    if not vals:
        return np.float32(-1.0)
    vals.sort(key=lambda f: (f, 0 if math.copysign(1.0, f) < 0 else 1))
    got = np.float32(vals[len(vals) // 2])
    assert got == np.sort(np.array(vals, np.float32))[len(vals) // 2]
    return got


def model(case):
    """-> dict(rows: per dense id the sorted, unique dense ids of its potential correspondences; pot_start, pot_tgt: the same as CSR; best: MATCH
    records per dense id (segID1 0xffffffff: none); median: float32 per chain view; verified, n_kept, n_candidates: the summary; lists: the list every
    chain view commits)"""
    base, nd = seg_base(case)
    S = case["S"]
    potential = {}
    best = np.full(nd, NO_MATCH, dtype=MATCH_DTYPE)
    median, verified, n_kept, n_cand, lists = [], [], [], [], []
    for k, v in enumerate(case["chain"]):
        vid = v["id"]
        assert vid in base and S[vid] == v["S"]
        if v["n_tbm"] > 0:
            lst = list(v["kept"])
            for s in range(v["S"]):
                p = int(v["bestpos"][s])
                if p >= 0 and len(lst) > 0:
                    best[base[vid] + s] = lst[p]
            median.append(median_of(v["best"]) if v["R"] > 0 else np.float32(1.0))
            n_cand.append(int(v["R"]))
        else:
            lst = early_list(case, k)
            seen = set()
            for m in lst:                                   # view.cc:165-183: the first of the highest confidence -- all are 0
                s = int(m["segID1"])
                if s < v["S"] and s not in seen:
                    seen.add(s)
                    best[base[vid] + s] = m
            median.append(np.float32(1.0))
            n_cand.append(0)
        for m in lst:                                       # line3D.cc:861-865
            ref, tgt = (vid, int(m["segID1"])), (int(m["camID2"]), int(m["segID2"]))
            potential.setdefault(ref, set()).add(tgt)
            potential.setdefault(tgt, set()).add(ref)
        verified.append(1 if v["n_tbm"] > 0 else 0)
        n_kept.append(len(lst))
        lists.append(lst)
    inside = lambda key: key[0] in base and key[1] < S[key[0]]
    rows, pot_start, pot_tgt = [], [0], []
    for vid in case["view_ids"]:
        for s in range(S[vid]):
            row = sorted(base[c] + t for (c, t) in potential.get((vid, s), ()) if inside((c, t)))
            rows.append(row)
            pot_tgt += row
            pot_start.append(len(pot_tgt))
    return dict(rows=rows, pot_start=np.array(pot_start, np.int64), pot_tgt=np.array(pot_tgt, np.int32), best=best, median=np.array(median, np.float32),
                verified=verified, n_kept=n_kept, n_candidates=n_cand, lists=lists, base=base, n_dense=nd, potential=potential)
