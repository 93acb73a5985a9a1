"""The host path around the count kernel of ``yawhip_count_pairs_dense(_batch)``: remembered plans never let an invalid call
through, and the dense epilogue (the tensor written slice by slice) gives the tensor an independent scatter of the fine
counts gives, also for a request that is finished after many other plans were made."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 6
EDGES = np.linspace(0.1, 0.9, 5)  # four redshift bins


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


def _dense_from_fine(fine, jobs, slices, fine_factors, halve):
    """[S, B, P, P] from per-job fine values f64[n_jobs, B, E - 1], as PatchLinkage.count_pairs' epilogue defines it."""
    n_bins, n_scales = slices.shape[:2]
    out = np.zeros((n_scales, n_bins, P, P))
    scaled = fine if fine_factors is None else fine * fine_factors[None]
    for s in range(n_scales):
        for k in range(n_bins):
            lo, hi = slices[k, s]
            if hi <= lo:
                continue
            for j, (a, b) in enumerate(jobs):
                v = scaled[j, k, lo] if hi - lo == 1 else scaled[j, k, lo:hi].sum()
                out[s, k, a, b] = v * (0.5 if halve and a == b else 1.0)
    return out


def test_invalid_calls_are_rejected_next_to_their_valid_twins():
    """An invalid call fails with the same status and message before any valid call and right after a valid call that
    differs from it in one job id, one threshold or the job count -- a remembered plan is never taken for it -- and again
    after an option was set."""
    from yet_another_wizz_amd import _lib, engine

    rng = np.random.default_rng(5)
    l1, l2 = _layout(rng, 30000, True), _layout(rng, 40000, False)
    jobs = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)
    t = np.tile(np.array([[1e-7, 4e-6]]), (4, 1))
    slices = _one_scale(4)
    bad_job = jobs.copy()
    bad_job[7, 1] = P
    bad_t = t.copy()
    bad_t[2, 1] = 5e-8  # descending
    more_jobs = np.concatenate([jobs, np.array([[0, -1]], dtype=np.int32)])
    cases = [
        (bad_job, t, rf"status -1\): job 7 has a patch id outside \[0,{P}\)"),
        (jobs, bad_t, r"status -1\): thresholds of bin 2 are not ascending non-negative numbers"),
        (more_jobs, t, rf"status -1\): job {len(jobs)} has a patch id outside \[0,{P}\)"),
    ]

    def rejected():
        for jb, th, msg in cases:
            with pytest.raises(_lib.YawhipError, match=msg):
                engine.count_dense(l1, l2, jb, th, slices, None, False)

    rejected()  # nothing remembered yet
    good, st = engine.count_dense(l1, l2, jobs, t, slices, None, False)
    truth, _ = engine.count_fine(l1, l2, jobs, t, kernel="exact")
    assert np.array_equal(good, _dense_from_fine(truth, jobs, slices, None, False)) and good.sum() > 0
    for _ in range(2):  # the valid twin's plan is remembered now, and used in between
        rejected()
        again, _ = engine.count_dense(l1, l2, jobs, t, slices, None, False)
        assert np.array_equal(again, good)
    ctx = engine.get_context()
    ctx.set_option("band_fp32", 0)
    try:
        rejected()
        other, st = engine.count_dense(l1, l2, jobs, t, slices, None, False)
        assert st.band_variant == 64 and np.array_equal(other, good)
        rejected()
    finally:
        ctx.set_option("band_fp32", 1)
    rejected()
    back, st = engine.count_dense(l1, l2, jobs, t, slices, None, False)
    assert st.band_variant == 32 and np.array_equal(back, good)


@pytest.mark.parametrize("n_fine", [1, 3], ids=["one-fine-bin", "separation-weights"])
def test_dense_tensor_of_a_weighted_autocorrelation_equals_the_scattered_fine_values(n_fine):
    """Weighted catalogue against itself with ``halve_diagonal``, with and without separation weights: the tensor of a
    single call, of a batch (twice, the second on remembered plans, next to a request that is not halved) and an
    independent scatter of ``count_fine``'s values agree -- single call and batch bit for bit."""
    from yet_another_wizz_amd import engine

    rng = np.random.default_rng(11)
    lay = _layout(rng, 50000, True, weights=True)
    jobs = np.array([(p, q) for p in range(P) for q in range(P) if abs(p - q) != 4], dtype=np.int32)
    edges = np.geomspace(1e-7, 6e-6, n_fine + 1)
    t = np.tile(edges[None], (4, 1)) * np.linspace(1.0, 1.3, 4)[:, None]
    fine_factors = rng.uniform(0.5, 2.0, (4, n_fine))
    if n_fine == 1:
        slices = _one_scale(4)
    else:  # two scales; the second one is empty in bin 1
        slices = np.tile(np.array([[[0, 3], [1, 2]]], dtype=np.int32), (4, 1, 1))
        slices[1, 1] = (2, 2)
    fine, _ = engine.count_fine(lay, lay, jobs, t)
    for ff in (None, fine_factors):
        single, st = engine.count_dense(lay, lay, jobs, t, slices, ff, True)
        plain, _ = engine.count_dense(lay, lay, jobs, t, slices, ff, False)
        expect = _dense_from_fine(fine, jobs, slices, ff, True)
        assert single.shape == expect.shape and single.sum() > 0
        if n_fine == 1:  # one element per sum: the same products in the same order
            assert np.array_equal(single, expect)
            assert np.array_equal(plain, _dense_from_fine(fine, jobs, slices, ff, False))
        else:
            np.testing.assert_allclose(single, expect, rtol=1e-13, atol=0)
        diag = np.eye(P, dtype=bool)
        assert np.array_equal(single[..., diag] * 2.0, plain[..., diag]) and np.array_equal(single[..., ~diag], plain[..., ~diag])
        for _ in range(2):
            batch = engine.count_dense_batch([(lay, lay, jobs, True), (lay, lay, jobs, False), (lay, lay, jobs[::2].copy(), True)],
                                             t, slices, ff)
            assert np.array_equal(batch[0][0], single) and np.array_equal(batch[1][0], plain)
            half_list, _ = engine.count_dense(lay, lay, jobs[::2].copy(), t, slices, ff, True)
            assert np.array_equal(batch[2][0], half_list)
            for name in ("evaluated_pairs", "candidate_pairs", "n_workgroups", "count_variant_weighted"):
                assert getattr(batch[0][1], name) == getattr(st, name), name


def test_unsplit_request_behind_split_ones_in_one_batch():
    """Weighted requests whose slabs exceed the budget are counted in pieces when their turn to finish comes, and every piece
    makes a plan of its own -- far more than a context keeps. An unweighted request enqueued behind them in the same batch is
    finished after all those plans came and went: its tensor is still the single call's, bit for bit."""
    from yet_another_wizz_amd import engine

    rng = np.random.default_rng(23)
    wl = _layout(rng, 40000, True, weights=True)
    ul = _layout(rng, 40000, True)
    jobs = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)
    t = np.tile(np.geomspace(1e-7, 6e-6, 4)[None], (4, 1))
    slices = np.tile(np.array([[[0, 3], [1, 2]]], dtype=np.int32), (4, 1, 1))
    ff = rng.uniform(0.5, 2.0, (4, 3))
    single_u, st_u = engine.count_dense(ul, ul, jobs, t, slices, ff, True)
    single_w, st_w = engine.count_dense(wl, wl, jobs, t, slices, ff, True)
    single_x, _ = engine.count_dense(wl, ul, jobs, t, slices, ff, False)
    fine_u, _ = engine.count_fine(ul, ul, jobs, t, kernel="exact")
    np.testing.assert_allclose(single_u, _dense_from_fine(fine_u, jobs, slices, ff, True), rtol=1e-13, atol=0)
    assert single_u.sum() > 0 and single_w.sum() > 0
    ctx = engine.get_context()
    requests = [(wl, wl, jobs, True), (wl, ul, jobs, False), (ul, ul, jobs, True), (ul, ul, jobs[::2].copy(), True)]
    half_u, _ = engine.count_dense(ul, ul, jobs[::2].copy(), t, slices, ff, True)
    for _ in range(2):
        ctx.set_option("slab_budget_bytes", 4096)
        try:
            batch = engine.count_dense_batch(requests, t, slices, ff)
        finally:
            ctx.set_option("slab_budget_bytes", 1 << 30)
        # in pieces, each a plan of its own: more of them than a context keeps (16)
        assert batch[0][1].n_launches > 16 * st_w.n_launches, (batch[0][1].n_launches, st_w.n_launches)
        assert batch[2][1].n_launches == st_u.n_launches      # not split: it waited in its slot meanwhile
        assert np.array_equal(batch[0][0], single_w) and np.array_equal(batch[1][0], single_x)
        assert np.array_equal(batch[2][0], single_u) and np.array_equal(batch[3][0], half_u)
