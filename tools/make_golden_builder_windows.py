#!/usr/bin/env python3
"""Record ``tests/golden/builder_windows.npz``: what the strip item builder makes of the cases of tests/builder_cases.py --
per case the evaluated pairs, the workgroups, the layout mode, whether merged triple runs were streamed, the band variant
(``CountStats``) and the evaluated pairs per job (``yawhip_job_work``). These numbers are the windows themselves: a builder
that hands the count kernels supersets of the right windows still counts what the oracle counts, but not these.

Run on the commit whose windows are to be kept (the parent of a change to the builder), on a GPU, with its library built:

    python tools/make_golden_builder_windows.py [--out FILE] [--check]

``--check`` compares the run with the committed file instead of writing one (exit status 1 on a difference). Counts are
checked against the oracle on the way, so a fixture is never recorded from a wrong count.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import builder_cases as bc  # noqa: E402
from yet_another_wizz_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "builder_windows.npz"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    ctx = _lib.Context(0)
    rec = {}
    for case in bc.CASES:
        counts, sums, st, work = bc.run_case(ctx, case)
        exp_c, exp_s = bc.expected(case["pairing"], case["weighted"])
        assert np.array_equal(counts, exp_c), case["name"]
        if case["weighted"]:
            np.testing.assert_allclose(sums, exp_s, rtol=1e-10, atol=0, err_msg=case["name"])
        for f in bc.STAT_FIELDS:
            rec[f"{case['name']}.{f}"] = np.int64(getattr(st, f))
        rec[f"{case['name']}.job_work"] = work.astype(np.int64)
        print(case["name"], {f: int(getattr(st, f)) for f in bc.STAT_FIELDS}, "work", int(work.sum()), "pairs", int(exp_c.sum()),
              flush=True)
    ctx.close()
    if args.check:
        old = np.load(args.out)
        bad = [k for k in rec if k not in old.files or not np.array_equal(old[k], rec[k])]
        print("differs:", bad if bad else "nothing")
        return 1 if bad else 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
