#!/usr/bin/env python3
"""Record tests/golden/lane_image.npz: `evaluated_pairs` and `exact_reevaluations` of every case of
tests/test_gpu_lane_image.py, as the library loaded gives them (needs a GPU).

    YAW_AMD_LIB=<library built from the commit before a change of the per-item path> python tools/make_golden_lane_image.py [--out FILE]

The test then holds the changed path to the same work: the same band entries walked, the same evaluations settled by the exact
predicate. Every case must match the oracle here too -- a record is only taken from a correct run."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_lane_image as lane  # noqa: E402
from oracle import oracle  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lane_image.npz"))
args = ap.parse_args()

devs = {scene: lane.table._Device(0, make()) for scene, make in lane.SCENES.items()}
ids, evaluated, exact = [], [], []
try:
    for case in lane.CASES:
        cid, scene, pair, grid, _, reach = case
        counts, sums, st = lane.run_case(devs[scene], case)
        cats = lane.SCENES[scene]()
        a, b = lane.PAIRS[pair]
        exp_c, exp_s = oracle.count_jobs(cats[a], cats[b], lane.JOBS, lane.thresholds(grid))
        assert st.variants == set(reach), (cid, st.variants)
        assert np.array_equal(counts, exp_c), cid
        np.testing.assert_allclose(sums, exp_s, rtol=lane.RTOL_W, atol=0, err_msg=cid)
        print(cid, st.evaluated_pairs, st.exact_reevaluations, flush=True)
        ids.append(cid); evaluated.append(st.evaluated_pairs); exact.append(st.exact_reevaluations)
finally:
    for d in devs.values():
        d.close()
np.savez_compressed(args.out, case=np.array([s.encode() for s in ids]), evaluated_pairs=np.array(evaluated, dtype=np.int64),
                    exact_reevaluations=np.array(exact, dtype=np.int64))
print("wrote", args.out)
