"""GPU: the two redshift-space counts (``yawhip_proj_count_smu``, ``yawhip_proj_count_smu_signed``) on the device against the
exact reference of tests/golden/smu_exact.npz (tools/make_golden_smu_exact.py: mpmath, ``S2 = ((d_a + d_b) / 2)^2 (2 asin(chord /
2))^2 + (c_b - c_a)^2`` against the s edges, ``m2[k] S2 < P2`` and ``sm2[k] S2 < sign(ps) P2`` against the float64 squares of the mu
edges -- not the contract's series): a scene at 0.5 to 30 arcseconds at dec 0, 60, +-89.99 degrees and across the wrap of the
right ascension, with ``d`` a factor 4 apart between neighbours, and one from 3 arcmin to 5.6 degrees (over the pole, across
the wrap) whose nearest objects reach the cap of 0.01. The second holds pairs that the chord, or a series cut after
``s2 / 12``, would put into another s bin or another mu plane, and pairs that pass the kernel's outer test ``fl(fl(DD s2) + P2)``
and have no bin; both hold pairs far along the line of sight and near on the sky, pairs with ``c_a == c_b`` bit for bit and
pairs at one sky position.

With unit weights the planes are the integers ``N_mu`` / ``N_smu`` of the file, bit for bit, on one handle and on two; with the
file's weights every element holds ``|ours - exact| <= K 2^-53 A`` with the ``K`` of this file, and is ``+0.0`` where the
reference is empty. Every case prints its worst ratio. A few hundred objects per call; nothing here reads mpmath."""
import numpy as np
import pytest

import smu_exact as se
from test_gpu_projected import upload
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
AXES = [0, 1, 2]


def run(fx, name, fold, two, weighted, axis_a, axis_b=None, unsigned=True, signed=False):
    """The counts of one case on one upload -> ``{(signed, <edge set>): (W, stats)}``."""
    ctx = engine.get_context(0)
    cells, s2 = se.cells(fx, name, fold, two), fx[f"{name}.s2"]
    a, b = se.handles(fx, name, fold, two, weighted)
    first = upload(ctx, a, axis_a)
    second = upload(ctx, b, axis_a if axis_b is None else axis_b) if two else first
    out = {}
    try:
        for edges in se.MU_SETS if unsigned else ():
            out[False, edges] = _lib.proj_count_smu(ctx, first, second, cells, s2, se.squares(fx, edges))
        for edges in se.SIGNED_SETS if signed else ():
            out[True, edges] = _lib.proj_count_smu_signed(ctx, first, second, cells, s2, se.squares(fx, edges, True))
    finally:
        first.free()
        if two:
            second.free()
    for _, stats in out.values():
        assert stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    return out


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("fold", [False, True], ids=["nb=2", "nb=1"])
@pytest.mark.parametrize("name", se.SCENES)
def test_unsigned_counts_and_sums_are_the_exact_ones(name, fold, sort_axis):
    fx = se.fixture()
    K = float(fx["K"])
    for two in (False, True):
        key = f"smu {name} nb={1 if fold else 2} axis={sort_axis} {'two handles' if two else 'one handle'}"
        got = run(fx, name, fold, two, False, sort_axis)
        for edges in se.MU_SETS:
            N = se.counts(fx, name, fold, two, edges)
            assert N.sum() > 1000 and np.array_equal(got[False, edges][0], N), (key, edges, np.abs(got[False, edges][0] - N).sum())
        got = run(fx, name, fold, two, True, sort_axis)
        for edges in se.MU_SETS:
            se.check(f"{key} {edges}", got[False, edges][0], *se.expected(name, fold, two, edges), K)


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("fold", [False, True], ids=["nb=2", "nb=1"])
@pytest.mark.parametrize("name", se.SCENES)
def test_signed_counts_and_sums_are_the_exact_ones(name, fold, sort_axis):
    fx = se.fixture()
    K = float(fx["K"])
    key = f"signed smu {name} nb={1 if fold else 2} axis={sort_axis}"
    got = run(fx, name, fold, True, False, sort_axis, unsigned=False, signed=True)
    for edges in se.SIGNED_SETS:
        N = se.counts(fx, name, fold, True, edges, signed=True)
        assert N.sum() > 1000 and np.array_equal(got[True, edges][0], N), (key, edges, np.abs(got[True, edges][0] - N).sum())
        if edges != "asymmetric":
            assert np.array_equal(se.fold_planes(got[True, edges][0]), se.counts(fx, name, fold, True, edges)), (key, edges)
    got = run(fx, name, fold, True, True, sort_axis, unsigned=False, signed=True)
    for edges in se.SIGNED_SETS:
        se.check(f"{key} {edges}", got[True, edges][0], *se.expected(name, fold, True, edges, signed=True), K)


@pytest.mark.parametrize("fold", [False, True], ids=["nb=2", "nb=1"])
def test_the_whole_segment_streamed_gives_the_windowed_bits(fold):
    """``wide`` with the two handles on different sort axes: no window, every pair of a cell evaluated -- the pairs just
    beyond the last edge (``wide.not_capped``) included, which must land nowhere -- and the same bits, both kernels."""
    fx = se.fixture()
    assert np.count_nonzero(fx["wide.not_capped"][:, 0] == 1) >= 8
    windowed = run(fx, "wide", fold, True, False, 2, 2, signed=True)
    whole = run(fx, "wide", fold, True, False, 2, 0, signed=True)
    assert set(whole) == {(False, edges) for edges in se.MU_SETS} | {(True, edges) for edges in se.SIGNED_SETS}
    for (signed, edges), (W, stats) in whole.items():
        assert stats.evaluated_pairs == stats.candidate_pairs >= windowed[signed, edges][1].evaluated_pairs > 0
        assert np.array_equal(W, windowed[signed, edges][0]) and np.array_equal(W, se.counts(fx, "wide", fold, True, edges, signed))


@pytest.mark.parametrize("name", se.SCENES)
def test_exchanging_the_handles_reverses_the_planes_but_for_the_pairs_at_ps_zero(name):
    """``count(a, b, edges)`` against ``count(b, a, -edges[::-1])`` with the cells' segments exchanged, as integers. A pair with
    ``ps != 0`` in plane j of one is in plane ``n - 1 - j`` of the other. A pair with ``c_a == c_b`` (``zero_ps``) has ``ps == +0``
    in both calls; the edge 0 of a mirrored set is closed above in both, so the pair lies in the plane BELOW 0 of both -- plane
    ``n / 2 - 1`` of each -- and not in each other's mirror image. With ``asymmetric``, where 0 is no edge, it is in ``(-0.4, 0.1]``
    and in ``(-0.1, 0.4]``, which are."""
    fx = se.fixture()
    cells, s2 = se.cells(fx, name, False, True), fx[f"{name}.s2"]
    a, b = se.handles(fx, name, False, True, False)
    tied = fx[f"{name}.zero_ps"]
    assert np.all(tied[:, 0] == 1) and np.array_equal(a["c"][tied[:, 1]], b["c"][tied[:, 2]]) and np.bincount(tied[:, 3], minlength=2).min() >= 8
    segment = lambda h, i: np.searchsorted(h["off"], i, side="right") - 1  # noqa: E731
    cell_of = {(sa, sb): n for n, (sa, sb, _, _) in enumerate(cells)}
    Z = np.zeros((len(cells), s2.shape[1] - 1))
    np.add.at(Z, ([cell_of[sa, sb] for sa, sb in zip(segment(a, tied[:, 1]), segment(b, tied[:, 2]))], tied[:, 4]), 1.0)
    ab = run(fx, name, False, True, False, 2, unsigned=False, signed=True)
    ctx = engine.get_context(0)
    first, second = upload(ctx, b), upload(ctx, a)
    swapped = np.ascontiguousarray(cells[:, [1, 0, 2, 3]])
    try:
        ba = {edges: _lib.proj_count_smu_signed(ctx, first, second, swapped, s2, -se.squares(fx, edges, True)[::-1])[0] for edges in se.SIGNED_SETS}
    finally:
        first.free(), second.free()
    for edges in se.SIGNED_SETS:
        W, n = ab[True, edges][0], len(ab[True, edges][0])
        assert W.sum() > 1000 and not np.array_equal(W, W[::-1])
        if edges == "asymmetric":
            assert np.array_equal(ba[edges][::-1], W) and np.all(W[1] >= Z)
            continue
        assert fx[f"smu.{edges}"][n // 2] == 0.0
        below, above = n // 2 - 1, n // 2
        moved = W.copy()
        moved[below] -= Z
        moved[above] += Z
        assert np.all(W[below] >= Z) and np.array_equal(ba[edges][::-1], moved), edges
        assert np.all(ba[edges][below] >= Z)  # ... and there they are: below 0 in the exchanged call too
