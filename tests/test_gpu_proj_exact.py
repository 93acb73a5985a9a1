"""GPU: the two projected counts (``yawhip_proj_count``, ``yawhip_proj_count_pi``) on the device against the exact reference of
tests/golden/proj_exact.npz (tools/make_golden_proj_exact.py: mpmath, ``R2 = ((d_a + d_b) / 2)^2 (2 asin(chord / 2))^2`` against
the radius edges, ``p = |c_a - c_b|`` against the cut and the pi edges -- not the contract's series): a scene at 0.5 to 30
arcseconds at dec 0, 60, +-89.99 degrees and across the wrap of the right ascension, with ``d`` a factor 4 apart between
neighbours, and one from 3 arcmin to 5.6 degrees (over the pole, across the wrap) whose nearest objects reach the cap of 0.01
and which holds pairs that the chord, or a series cut after ``s2 / 12``, would put into another bin, and pairs that pass the
kernel's outer test and have no bin, on either side of the cut in ``p``.

With unit weights ``W`` is the integer pair count ``N`` of the file and the planes are ``N_pi``, bit for bit, on one handle and
on two; with the file's weights every element holds ``|ours - exact| <= K 2^-53 A`` with the ``K`` of this file, and is ``+0.0``
where the reference is empty. Every case prints its worst ratio. A few hundred objects per call; nothing here reads mpmath."""
import numpy as np
import pytest

import proj_exact as pe
from test_gpu_projected import upload
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
AXES = [0, 1, 2]


def run(fx, name, fold, two, weighted, axis_a, axis_b=None):
    """Both counts of one case on one upload -> ``{None: (W, stats), <edge set>: (W_pi, stats)}``."""
    ctx = engine.get_context(0)
    cells, r2 = pe.cells(fx, name, fold, two), fx[f"{name}.r2"]
    first = upload(ctx, pe.scene(fx, name, "a", fold, weighted), axis_a)
    second = upload(ctx, pe.scene(fx, name, "b", fold, weighted), axis_a if axis_b is None else axis_b) if two else first
    try:
        out = {None: _lib.proj_count(ctx, first, second, cells, r2, float(fx["pmax"]))}
        for edges in pe.PI_SETS:
            out[edges] = _lib.proj_count_pi(ctx, first, second, cells, r2, fx[f"pi.{edges}"])
    finally:
        first.free()
        if two:
            second.free()
    for _, stats in out.values():
        assert stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    return out


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("fold", [False, True], ids=["nb=2", "nb=1"])
@pytest.mark.parametrize("name", pe.SCENES)
def test_counts_and_sums_are_the_exact_ones(name, fold, sort_axis):
    fx = pe.fixture()
    K = float(fx["K"])
    for two in (False, True):
        key = f"proj {name} nb={1 if fold else 2} axis={sort_axis} {'two handles' if two else 'one handle'}"
        N = pe.counts(fx, name, fold, two)
        got = run(fx, name, fold, two, False, sort_axis)
        assert N.sum() > 1000 and np.array_equal(got[None][0], N), (key, np.abs(got[None][0] - N).sum())
        for edges in pe.PI_SETS:
            N_pi = pe.counts_pi(fx, name, fold, two, edges)
            assert np.array_equal(got[edges][0], N_pi), (key, edges, np.abs(got[edges][0] - N_pi).sum())
        got = run(fx, name, fold, two, True, sort_axis)
        for edges in (None,) + pe.PI_SETS:
            pe.check(f"{key} {edges or 'single'}", got[edges][0], *pe.expected(fx, name, fold, two, edges), K)


@pytest.mark.parametrize("fold", [False, True], ids=["nb=2", "nb=1"])
def test_the_whole_segment_streamed_gives_the_windowed_bits(fold):
    """``wide`` with the two handles on different sort axes: no window, every pair of a cell evaluated -- the pairs just
    beyond the last edge (``wide.not_capped``) included, which must land nowhere -- and the same bits of ``N`` and ``N_pi``."""
    fx = pe.fixture()
    assert np.count_nonzero(fx["wide.not_capped"][:, 0] == 1) >= 8
    windowed = run(fx, "wide", fold, True, False, 2, 2)
    whole = run(fx, "wide", fold, True, False, 2, 0)
    for edges in (None,) + pe.PI_SETS:
        exp = pe.counts(fx, "wide", fold, True) if edges is None else pe.counts_pi(fx, "wide", fold, True, edges)
        assert whole[edges][1].evaluated_pairs == whole[edges][1].candidate_pairs >= windowed[edges][1].evaluated_pairs > 0
        assert np.array_equal(whole[edges][0], windowed[edges][0]) and np.array_equal(whole[edges][0], exp)
