"""Measures the tolerance of the refinement tests and writes tests/golden/refine_tolerance.json (CPU only: python tests/golden/make_golden_refine.py).

The product sums an evaluation's terms in 64 lane-strided partial sums and a tree, the model of tests/refine_model.py sequentially: the two differ by what a
change of summation order costs.  That cost is measured with the MODEL alone: every group of every case of tests/refine_cases.py is run with its members in
forward order, reversed, and in three seeded permutations, and per quantity (refine_cases.differences: angle, offset, rms, points) the largest difference to
the forward run is recorded.  The tolerance is 16 times that spread -- the product's order is one more order of the same kind, the factor covers the orders
not sampled -- with a floor of 1e-14.  Recorded as well, per group: the smallest gap between adjacent sort keys t over the extent (the CPU test asserts
that it exceeds 1000 times the end-point tolerance: the sweep order cannot flip) -- and the CPU test asserts that no tolerance exceeds 1e-6."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import refine_cases as rc  # noqa: E402
import refine_model as rm  # noqa: E402

FACTOR, FLOOR = 16.0, 1e-14


def main():
    out = {"factor": FACTOR, "floor": FLOOR, "orders": ["forward", "reversed", "permutation seeds 1, 2, 3"], "cases": {}}
    for case in rc.CASES:
        groups = []
        for g, sl in enumerate(rc.group_slices(case)):
            n, E = sl.stop - sl.start, rc.extent_of(case, g)
            base = rm.refine(*rc.reordered(case, g, np.arange(n)))[0]
            if base["status"] == 2 and not np.all(np.isfinite(base["line"])):
                groups.append(None)                                      # (not finite: nothing to compare)
                continue
            spread = {q: 0.0 for q in rc.QUANTITIES}
            for order in [np.arange(n)[::-1]] + [np.random.default_rng(s).permutation(n) for s in (1, 2, 3)]:
                d = rc.differences(base, rm.refine(*rc.reordered(case, g, order))[0], E)
                for q in rc.QUANTITIES:
                    spread[q] = max(spread[q], d[q])
            t = np.sort(base["t"])
            groups.append({"spread": spread, "tolerance": {q: max(FACTOR * spread[q], FLOOR) for q in rc.QUANTITIES}, "min_key_gap": float(np.diff(t).min() / E)})
            print(case["name"], g, groups[-1])
        out["cases"][case["name"]] = groups
    with open(os.path.join(HERE, "refine_tolerance.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
