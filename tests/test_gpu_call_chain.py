"""The chain a warm count call puts on the stream -- item builder, count kernel(s), ``k_call_tail`` -- with no fill in front of
it: the tail zeroes counters and counts of the slot's result block behind its own reads, and a slot whose last call did not
end that way (rejected, builder only, counts left on the device, abandoned) fills the block itself. Whatever ran before, a
count gives the oracle's numbers, bit for bit the same every time; and ``kernel_ms`` / ``count_ms``, taken from device clock
stamps, keep their order and stay inside the wall time of the call."""
import time

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

P = 6
EDGES = np.linspace(0.1, 0.9, 5)  # four redshift bins
T = np.tile(np.array([[1e-7, 4e-6]]), (4, 1))  # one annulus
T_OTHER = np.tile(np.array([[2e-7, 9e-6]]), (4, 1))
ALL_JOBS = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)
OTHER_JOBS = np.array([(p, q) for p in range(P) for q in range(P) if (p + q) % 3 != 1], dtype=np.int32)


def _layout(rng, n, bins, weights=False):
    import yet_another_wizz_amd as yaw

    ra, dec = rng.uniform(40.0, 48.0, n), rng.uniform(-4.0, 4.0, n)
    centers = yaw.AngularCoordinates(np.deg2rad([[41.5 + 2.5 * (i % 3), -2.0 + 4.0 * (i // 3)] for i in range(P)]))
    z = rng.uniform(0.1, 0.9, n) if bins else None
    w = rng.uniform(0.5, 1.5, n) if weights else None
    cat = yaw.Catalog.from_arrays(ra, dec, weights=w, redshifts=z, patch_centers=centers)
    return cat.build_trees(EDGES if bins else None)


def _one_scale(n_bins):
    return np.tile(np.array([[[0, 1]]], dtype=np.int32), (n_bins, 1, 1))  # slices int32[B, S = 1, 2]


def _dense(fine, jobs):
    """[S = 1, B, P, P] from per-job fine values f64[n_jobs, B, 1]: an independent scatter."""
    out = np.zeros((1, fine.shape[1], P, P))
    for j, (a, b) in enumerate(jobs):
        out[0, :, a, b] = fine[j, :, 0]
    return out


class World:
    """Catalogues of the shapes of test_gpu_call_overhead.py and the oracle's counts for them, made once."""

    def __init__(self):
        rng = np.random.default_rng(77)
        self.binned = _layout(rng, 30000, True)
        self.plain = _layout(rng, 40000, False)
        self.binned_w = _layout(rng, 30000, True, weights=True)
        self.binned2 = _layout(rng, 40000, True)
        self.slices = _one_scale(4)
        self.fine = helpers.oracle_count_fine(self.binned, self.plain, ALL_JOBS, T)[0]
        self.fine_w = helpers.oracle_count_fine(self.binned_w, self.plain, ALL_JOBS, T)[0]
        self.fine_bb = helpers.oracle_count_fine(self.binned, self.binned2, ALL_JOBS, T)[0]
        assert self.fine.sum() > 0 and self.fine_w.sum() > 0 and self.fine_bb.sum() > 0


@pytest.fixture(scope="module")
def world():
    return World()


def _timed(call):
    """(result, stats) of ``call`` with the timing fields checked against the wall time measured around it."""
    t0 = time.perf_counter()
    out, st = call()
    wall_ms = (time.perf_counter() - t0) * 1e3
    print(f"count_ms {st.count_ms:.4f}  kernel_ms {st.kernel_ms:.4f}  wall {wall_ms:.4f} ms")
    assert 0.0 < st.count_ms <= st.kernel_ms <= wall_ms, (st.count_ms, st.kernel_ms, wall_ms)
    return out, st


def _count(w, l1=None, l2=None, jobs=ALL_JOBS, t=T):
    from yet_another_wizz_amd import engine

    l1, l2 = l1 or w.binned, l2 or w.plain
    return _timed(lambda: engine.count_dense(l1, l2, jobs, t, _one_scale(len(t)), None, False))[0]


def test_block_is_clean_between_different_calls(world):
    """Call A, a call with other jobs and thresholds, A again: both A tensors are the oracle's, bit for bit. The other call
    has fewer rows, so A's second run has counts where nothing of the call between them lay."""
    w = world
    expect = _dense(w.fine, ALL_JOBS)
    first = _count(w)
    other = _count(w, jobs=OTHER_JOBS, t=T_OTHER)
    again = _count(w)
    assert np.array_equal(first, expect) and np.array_equal(again, expect)
    assert other.sum() > first[0][:, OTHER_JOBS[:, 0], OTHER_JOBS[:, 1]].sum()  # wider annulus: really another count
    # and from the smaller block to the larger one: the larger one's counts lie where the smaller one's tail did not clean
    assert np.array_equal(_count(w, jobs=OTHER_JOBS[:5].copy()), _dense(w.fine, ALL_JOBS) * _mask(OTHER_JOBS[:5]))
    assert np.array_equal(_count(w), expect)


def _mask(jobs):
    m = np.zeros((1, 1, P, P))
    m[0, 0, jobs[:, 0], jobs[:, 1]] = 1.0
    return m


def test_block_is_clean_between_weighted_calls(world):
    """The same with a weighted pair (sums behind the counts in the block, written by the reduction): A, a shorter job list,
    A -- and then an unweighted count in the same slot, whose counts lie where the weighted call's sums were."""
    w = world
    expect = _dense(w.fine_w, ALL_JOBS)
    first = _count(w, l1=w.binned_w)
    _count(w, l1=w.binned_w, jobs=OTHER_JOBS, t=T_OTHER)
    again = _count(w, l1=w.binned_w)
    assert np.array_equal(first, again)
    np.testing.assert_allclose(first, expect, rtol=helpers.RTOL_W, atol=0)
    short = _count(w, l1=w.binned_w, jobs=ALL_JOBS[:7].copy())
    np.testing.assert_allclose(short, expect * _mask(ALL_JOBS[:7]), rtol=helpers.RTOL_W, atol=0)
    assert np.array_equal(_count(w), _dense(w.fine, ALL_JOBS))  # unweighted, larger counts part than the call before


def test_block_is_clean_with_sums_of_an_unweighted_pair(world):
    """``want_sums`` on an unweighted pair (k_counts_to_double behind the count kernel): counts and sums of A, of another
    call, of A again; then counts alone, whose block is laid out as before."""
    from yet_another_wizz_amd import _lib, engine

    w = world
    ctx, d1, d2 = engine._device_pair(w.binned, w.plain, T, 2)

    def both(jobs, t):
        def call():
            counts, sums, st = _lib.count_pairs(ctx, d1, d2, jobs, t, want_counts=True, want_sums=True)
            return (counts, sums), st
        return _timed(call)[0]

    c0, s0 = both(ALL_JOBS, T)
    both(OTHER_JOBS, T_OTHER)
    c1, s1 = both(ALL_JOBS, T)
    assert np.array_equal(c0, w.fine.astype(np.int64)) and np.array_equal(s0, w.fine)
    assert np.array_equal(c1, c0) and np.array_equal(s1, s0)
    both(OTHER_JOBS[:5].copy(), T)  # a short block: its sums lie inside the counts of the next call
    counts, sums, _ = _lib.count_pairs(ctx, d1, d2, ALL_JOBS, T)
    assert sums is None and np.array_equal(counts, c0)


def test_rejected_and_builder_only_calls_between_counts(world):
    """A rejected call, a call after ``set_option`` and a ``job_work`` call (the builder alone: it leaves its counters in the
    block) sit between counts: the counts do not change."""
    from yet_another_wizz_amd import _lib, engine

    w = world
    expect = _dense(w.fine, ALL_JOBS)
    assert np.array_equal(_count(w), expect)
    bad = ALL_JOBS.copy()
    bad[7, 1] = P
    with pytest.raises(_lib.YawhipError, match=rf"job 7 has a patch id outside \[0,{P}\)"):
        engine.count_dense(w.binned, w.plain, bad, T, w.slices, None, False)
    assert np.array_equal(_count(w), expect)
    ctx = engine.get_context()
    ctx.set_option("band_fp32", 0)
    try:
        assert np.array_equal(_count(w), expect)
    finally:
        ctx.set_option("band_fp32", 1)
    assert np.array_equal(_count(w), expect)
    work = engine.job_work(w.binned, w.plain, ALL_JOBS, T)
    assert work.shape == (len(ALL_JOBS),) and work.sum() > 0
    assert np.array_equal(_count(w), expect)
    assert np.array_equal(engine.job_work(w.binned, w.plain, ALL_JOBS, T), work)
    assert np.array_equal(_count(w), expect)
    ctx.set_option("spin_wait", 0)  # the blocking wait sees the same block
    try:
        assert np.array_equal(_count(w), expect)
    finally:
        ctx.set_option("spin_wait", 1)
    assert np.array_equal(_count(w), expect)


def test_nine_requests_in_four_slots(world):
    """A batch of nine requests -- more than twice the slots, binned x unbinned next to binned x binned, weighted next to
    unweighted, one request twice -- equals nine single calls bit for bit, twice over (the second time every slot starts from
    what the first batch left)."""
    from yet_another_wizz_amd import engine

    w = world
    requests = [(w.binned, w.plain, ALL_JOBS, False), (w.binned, w.binned2, ALL_JOBS, False), (w.binned_w, w.plain, OTHER_JOBS, False),
                (w.binned, w.plain, OTHER_JOBS, False), (w.binned, w.plain, ALL_JOBS, False), (w.binned, w.binned2, OTHER_JOBS[:5].copy(), False),
                (w.binned_w, w.plain, ALL_JOBS, False), (w.binned, w.binned2, ALL_JOBS[::2].copy(), False), (w.binned, w.plain, ALL_JOBS[:1].copy(), False)]
    singles = [_count(w, l1=l1, l2=l2, jobs=jobs) for l1, l2, jobs, _ in requests]
    assert np.array_equal(singles[0], _dense(w.fine, ALL_JOBS)) and np.array_equal(singles[1], _dense(w.fine_bb, ALL_JOBS))
    np.testing.assert_allclose(singles[6], _dense(w.fine_w, ALL_JOBS), rtol=helpers.RTOL_W, atol=0)
    for _ in range(2):
        t0 = time.perf_counter()
        batch = engine.count_dense_batch(requests, T, w.slices, None)
        wall_ms = (time.perf_counter() - t0) * 1e3
        assert len(batch) == 9
        for (dense, st), single in zip(batch, singles):
            assert np.array_equal(dense, single)
            assert 0.0 < st.count_ms <= st.kernel_ms <= wall_ms, (st.count_ms, st.kernel_ms, wall_ms)


def test_split_request_in_front_of_an_unsplit_one(world):
    """A weighted job list cut in pieces by a small ``slab_budget`` and an unsplit request behind it in the same batch: both
    give the oracle's values, and so does the next plain call."""
    from yet_another_wizz_amd import engine

    w = world
    ctx = engine.get_context()
    _, st_w = engine.count_dense(w.binned_w, w.plain, ALL_JOBS, T, w.slices, None, False)
    ctx.set_option("slab_budget_bytes", 4096)
    try:
        t0 = time.perf_counter()
        batch = engine.count_dense_batch([(w.binned_w, w.plain, ALL_JOBS, False), (w.binned, w.plain, ALL_JOBS, False)], T, w.slices, None)
        wall_ms = (time.perf_counter() - t0) * 1e3
    finally:
        ctx.set_option("slab_budget_bytes", 1 << 30)
    assert batch[0][1].n_launches > st_w.n_launches  # in pieces
    np.testing.assert_allclose(batch[0][0], _dense(w.fine_w, ALL_JOBS), rtol=helpers.RTOL_W, atol=0)
    assert np.array_equal(batch[1][0], _dense(w.fine, ALL_JOBS))
    for _, st in batch:
        assert 0.0 < st.count_ms <= st.kernel_ms <= wall_ms, (st.count_ms, st.kernel_ms, wall_ms)
    assert np.array_equal(_count(w), _dense(w.fine, ALL_JOBS))


def test_small_block_and_empty_job_list(world):
    """One job and one bin (a result block of sixteen bytes behind the counters) and an empty job list return the right
    shapes; the call after each is correct."""
    from yet_another_wizz_amd import engine

    w = world
    rng = np.random.default_rng(3)
    plain2 = _layout(rng, 30000, False)
    t1 = T[:1].copy()
    job = np.array([[2, 1]], dtype=np.int32)
    expect1 = helpers.oracle_count_fine(plain2, w.plain, job, t1)[0]
    assert expect1.shape == (1, 1, 1) and expect1.sum() > 0
    expect = _dense(w.fine, ALL_JOBS)
    for _ in range(2):
        one = _count(w, l1=plain2, jobs=job, t=t1)
        assert one.shape == (1, 1, P, P) and one[0, 0, 2, 1] == expect1[0, 0, 0] and one.sum() == expect1.sum()
        assert np.array_equal(_count(w), expect)
        none, st = engine.count_dense(w.binned, w.plain, np.zeros((0, 2), dtype=np.int32), T, w.slices, None, False)
        assert none.shape == (1, 4, P, P) and not none.any() and st.n_launches == 0
        assert np.array_equal(_count(w), expect)
