"""The dense epilogue (``dense_scatter`` of csrc/yawhip_dense.hip) through ``yawhip_count_pairs_dense``: the tensor
[scale][bin][patch i][patch j] equals one assembled in numpy from the [jobs, B, E - 1] output of ``yawhip_count_pairs`` -- the
same products in the same order ((value x separation weight) x half; several fine bins: numpy's sum of the weighted fine
bins, x half), so ``np.array_equal``. One case per route of the epilogue: one fine bin per (job, bin) from integer counts,
the same from weighted sums, and per-scale values recombined from several fine bins (``comb``); each with and without the
halved diagonal. (``dense_scatter`` has no exported hook -- one would change the ABI tests/test_abi.py pins -- so the test
needs the device.)"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu
P, B, S = 3, 2, 2
ARCMIN = np.pi / 10800


@pytest.fixture(scope="module")
def ctx():
    from yet_another_wizz_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _catalog(seed, n, nb, weighted):
    rng = np.random.default_rng(seed)
    ra = np.deg2rad(rng.uniform(100.0, 101.5, n))
    dec = np.arcsin(rng.uniform(np.sin(np.deg2rad(30.0)), np.sin(np.deg2rad(31.5)), n))
    patch = rng.integers(0, P, n)
    z = rng.uniform(0.1, 0.9, n)
    w = rng.uniform(0.5, 1.5, n) if weighted else None
    return oracle.sort_catalog(ra, dec, z, w, patch, P, np.linspace(0.1, 0.9, nb + 1) if nb > 1 else None, "right")


ROUTES = {
    # route: (weighted, fine-bin edges in arcmin, slices [S][2] of every bin)
    "unweighted": (False, [1.0, 8.0], [[0, 1], [0, 1]]),
    "weighted": (True, [1.0, 8.0], [[0, 1], [0, 1]]),
    "comb": (False, [1.0, 2.0, 4.0, 8.0], [[0, 2], [1, 3]]),
}


@pytest.mark.parametrize("halve", [True, False])
@pytest.mark.parametrize("route", list(ROUTES))
def test_dense_tensor_is_the_scatter_of_the_job_rows(ctx, route, halve):
    from yet_another_wizz_amd import _lib

    weighted, edges, sl = ROUTES[route]
    c1, c2 = _catalog(51, 4000, B, weighted), _catalog(52, 5000, 1, weighted)
    up = lambda c: _lib.DeviceCatalog(ctx, c["x"], c["y"], c["z"], c["w"], P, c["nb"], c["off"])
    d1, d2 = up(c1), up(c2)
    jobs = np.array([(p, q) for p in range(P) for q in range(P) if (p, q) != (2, 0)], dtype=np.int32)  # one slot stays unlinked
    t = np.ascontiguousarray(np.tile(oracle.thresholds_for(np.array(edges) * ARCMIN), (B, 1)))
    nf = t.shape[1] - 1
    slices = np.ascontiguousarray(np.tile(np.array(sl, dtype=np.int32), (B, 1, 1)))  # [B, S, 2]
    fine_factors = np.ascontiguousarray(0.25 + np.arange(B * nf, dtype=np.float64).reshape(B, nf) / 7.0)
    counts, sums, _ = _lib.count_pairs(ctx, d1, d2, jobs, t, want_counts=True, want_sums=True)
    fine = sums if weighted else counts.astype(np.float64)
    assert counts.sum() > 10000 and np.all(counts.any(axis=(1, 2)))
    want = np.zeros((S, B, P, P))
    for j, (p, q) in enumerate(jobs):
        half = 0.5 if halve and p == q else 1.0
        for k in range(B):
            for s in range(S):
                lo, hi = slices[k, s]
                if nf == 1:
                    value = fine[j, k, 0] * fine_factors[k, 0]
                else:
                    value = np.ascontiguousarray(fine[j, k, lo:hi] * fine_factors[k, lo:hi]).sum()
                want[s, k, p, q] = value * half
    got, _ = _lib.count_pairs_dense(ctx, d1, d2, jobs, t, slices, fine_factors, halve)
    assert np.array_equal(got, want)
    assert not got[:, :, 2, 0].any() and got[:, :, 0, 0].all()
    # and without separation weights
    want1 = want / 1.0
    got1, _ = _lib.count_pairs_dense(ctx, d1, d2, jobs, t, slices, None, halve)
    for j, (p, q) in enumerate(jobs):
        half = 0.5 if halve and p == q else 1.0
        for k in range(B):
            for s in range(S):
                lo, hi = slices[k, s]
                want1[s, k, p, q] = (fine[j, k, 0] if nf == 1 else np.ascontiguousarray(fine[j, k, lo:hi]).sum()) * half
    assert np.array_equal(got1, want1)
