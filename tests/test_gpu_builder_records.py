"""GPU: the strip item builder reads one record per lane tile (first object, length, run, keys of its first and last
object) and one per streamed run (first entry, length, keys of its first and last entry, inv, in front of the run's grid)
instead of looking the same values up in the offset table and the key columns. Every case of tests/builder_cases.py checks

  * the counts against the brute-force oracle, bit for bit (weighted sums to 1e-10 relative): the contract of
    tests/test_gpu_kernel_parity.py, and
  * the windows themselves: ``stats.evaluated_pairs``, ``stats.n_workgroups`` and the per-job work of ``yawhip_job_work`` equal
    what the commit before the records produced for the same seed (tests/golden/builder_windows.npz, recorded there with
    tools/make_golden_builder_windows.py). The oracle alone would also pass with windows that are supersets of the right ones.

The scenes hold the shapes at which a record can be wrong: runs of length 1, runs whose keys are all equal (inv = 0), empty
runs between others, partner strips outside the streamed group on both sides, last lane tiles of 1, 63 and 127 objects,
merged triple runs and three separate windows, trimmed and untrimmed windows, both strip grids, all three tile sizes,
per-(patch, bin) layouts with half bands, weights, and a job table of 1 025 jobs."""
import numpy as np
import pytest

import builder_cases as bc
from conftest import load_golden

RTOL_W = 1e-10


@pytest.fixture(scope="module")
def ctx():
    from yet_another_wizz_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def parent():
    return load_golden("builder_windows.npz")


def test_the_scene_holds_the_runs_it_is_meant_to():
    """The row has one key and the run lengths named in builder_cases (strips of the latitude grid, from the columns)."""
    for name in ("binned", "unbinned"):
        cat = bc.catalog(name, False)
        nb = cat["nb"]
        lo, hi = cat["off"][4 * nb], cat["off"][5 * nb]  # patch 4, all bins
        assert len(np.unique(cat["z"][lo:hi])) == 1  # one sort key for the whole row
        lat = np.arctan2(cat["y"][lo:hi], np.hypot(cat["z"][lo:hi], cat["x"][lo:hi]))
        strips, lengths = np.unique(np.floor((lat + 0.5 * np.pi) / bc.STRIP).astype(np.int64), return_counts=True)
        assert dict(zip((strips - strips[0] + 1).tolist(), lengths.tolist())) == bc.ROW_COUNTS
        lo, hi = cat["off"][5 * nb], cat["off"][6 * nb]
        assert hi - lo == len(bc.SINGLE_STRIPS)
    assert {c % 64 for c in bc.ROW_COUNTS.values()} >= {1, 63} and 127 in {c % 128 for c in bc.ROW_COUNTS.values()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_windows_are_the_parents_and_counts_the_oracles(ctx, parent, name):
    case = bc.CASES[bc.CASE_NAMES.index(name)]
    counts, sums, st, work = bc.run_case(ctx, case)
    exp_c, exp_s = bc.expected(case["pairing"], case["weighted"])
    assert exp_c.sum() > 100000
    got = {f: int(getattr(st, f)) for f in bc.STAT_FIELDS}
    want = {f: int(parent[f"{name}.{f}"]) for f in bc.STAT_FIELDS}
    print(name, "got", got, "parent", want, "work", int(work.sum()), "parent", int(parent[f"{name}.job_work"].sum()))
    # the case runs on the path it is meant for
    assert st.layout_mode == case["mode"]
    if case["kernel"] == "band":
        assert st.band_variant == 32
        assert st.merged_triples == (1 if case["options"]["triple_runs"] == 2 else 0)
    # the oracle's counts
    assert np.array_equal(counts, exp_c)
    if case["weighted"]:
        np.testing.assert_allclose(sums, exp_s, rtol=RTOL_W, atol=0)
    else:
        assert np.array_equal(sums, exp_c.astype(np.float64))
    # the parent's windows
    assert got == want
    assert np.array_equal(work, parent[f"{name}.job_work"])
    assert work.sum() > 0
