"""GPU: the per-lens radial count (``yawhip_dsigma_count_radial``) on the device against the exact reference of
tests/golden/dsigma_radial_exact.npz (tools/make_golden_dsigma_radial_exact.py: mpmath, ``R2 = m_l (2 asin(chord / 2))^2``
against the edges -- not the contract's series): a scene at 0.5 to 30 arcseconds at dec 0, 60, +-89.99 degrees and across the
wrap of the right ascension, with ``m`` a factor 17 apart between neighbouring lenses, and one from 3 arcmin to 5.6 degrees
(over the pole, across the wrap) whose nearest lenses reach the cap of 0.01 and which holds pairs that the chord, or a series
cut after ``s2 / 12``, would put into another bin, and pairs that pass the kernel's outer test and have no bin.

With unit columns ``W`` is the integer pair count ``N`` of the file, bit for bit; with the file's columns and with those of the
shear driver (``f = 1``, ``c = 0``, ``u = 0``) the sums hold the rule of tests/shear_exact.py with the ``K`` of this file. Every
case prints its worst ratio. A few hundred objects per call; nothing here reads mpmath."""
import numpy as np
import pytest

import dsigma_radial_exact as dre
import shear_exact as se
from test_gpu_dsigma_radial import count

pytestmark = pytest.mark.gpu
AXES = [0, 1, 2]


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("fold", [False, True], ids=["nb=2", "nb=1"])
@pytest.mark.parametrize("name", dre.SCENES)
def test_counts_and_sums_are_the_exact_ones(name, fold, sort_axis):
    fx = dre.fixture()
    jobs, r2, K = fx[f"{name}.jobs"], fx[f"{name}.r2"], float(fx["K"])
    key = f"radial {name} nb={1 if fold else 2} axis={sort_axis}"
    N = dre.counts(fx, name, fold)
    T, X, W, stats = count(*dre.scene(fx, name, "unit", fold), jobs, r2, sort_axis)
    assert stats.n_workgroups == len(jobs) * 2 and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    assert N.sum() > 1000 and np.array_equal(W, N), (key, np.abs(W - N).sum())
    assert not np.any(T) and not np.any(X)
    for columns in ("real", "shear"):
        T, X, W, stats = count(*dre.scene(fx, name, columns, fold), jobs, r2, sort_axis)
        assert stats.n_workgroups == len(jobs) * 2 and 0 < stats.evaluated_pairs <= stats.candidate_pairs
        se.check(f"{key} {columns}", "TX", (T, X), W, dre.expected(fx, name, columns, fold), K)


@pytest.mark.parametrize("fold", [False, True], ids=["nb=2", "nb=1"])
def test_the_whole_segment_streamed_gives_the_windowed_bits(fold):
    """``wide`` with the two handles on different sort axes: no window, every pair of a job evaluated -- the pairs just
    beyond the last edge (``wide.not_capped``) included -- and the same bits of the pair counts ``W``. (With real columns the
    sources come in another order and ``W`` is another sum of the same terms: it holds the rule.)"""
    fx = dre.fixture()
    jobs, r2 = fx["wide.jobs"], fx["wide.r2"]
    lens, src = dre.scene(fx, "wide", "unit", fold)
    windowed = count(lens, src, jobs, r2, 2, 2)
    whole = count(lens, src, jobs, r2, 2, 0)
    assert whole[3].evaluated_pairs == whole[3].candidate_pairs >= windowed[3].evaluated_pairs > 0
    assert np.array_equal(whole[2], windowed[2]) and np.array_equal(whole[2], dre.counts(fx, "wide", fold))
    T, X, W, stats = count(*dre.scene(fx, "wide", "real", fold), jobs, r2, 2, 0)
    assert stats.evaluated_pairs == stats.candidate_pairs
    se.check(f"radial wide nb={1 if fold else 2} streamed whole", "TX", (T, X), W, dre.expected(fx, "wide", "real", fold), float(fx["K"]))
