#!/usr/bin/env python3
"""Record tests/golden/band_walk_trips.npz: `evaluated_pairs` and `exact_reevaluations` of every case of
tests/test_gpu_band_walk_trips.py, as the library loaded gives them (needs a GPU).

    YAW_AMD_LIB=<library built from the commit before a change of the walk loop> python tools/make_golden_band_walk_trips.py [--out FILE]

The test then holds a rewritten loop to the same work: the same entries evaluated, the same evaluations settled by the exact
predicate. Every case must match the oracle here too -- a record is only taken from a correct run."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_band_walk_trips as walk  # noqa: E402
from oracle import oracle  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "band_walk_trips.npz"))
args = ap.parse_args()

cats = walk._scene()
dev = walk.table._Device(0, cats)
ids, evaluated, exact = [], [], []
try:
    for case in walk.CASES:
        cid, pair, grid, _, reach = case
        counts, sums, st = walk.run_case(dev, case)
        a, b = walk.PAIRS[pair]
        exp_c, exp_s = oracle.count_jobs(cats[a], cats[b], walk.JOBS, walk.thresholds(grid))
        assert st.variants == set(reach), (cid, st.variants)
        assert np.array_equal(counts, exp_c), cid
        np.testing.assert_allclose(sums, exp_s, rtol=walk.RTOL_W, atol=0, err_msg=cid)
        print(cid, st.evaluated_pairs, st.exact_reevaluations)
        ids.append(cid); evaluated.append(st.evaluated_pairs); exact.append(st.exact_reevaluations)
finally:
    dev.close()
np.savez(args.out, case=np.array(ids), evaluated_pairs=np.array(evaluated, dtype=np.int64),
         exact_reevaluations=np.array(exact, dtype=np.int64))
print("wrote", args.out)
