"""GPU: the two counts with a signed line of sight (``yawhip_proj_count_pi_signed``, ``yawhip_proj_count_smu_signed``; DESIGN.md
section 27) and the drivers on top of them, on the device.

The pi count is held to the exact reference of tests/golden/proj_exact.npz: tests/test_signed_host.py shows that the signed
oracle's membership folds to the file's mpmath integers with no pair at ``ps == 0`` or on an edge, and the sign of a float64
difference is the sign of the true difference, so the oracle's member pairs per signed plane ARE the exact ones; over them
the weighted reference is the sum of the exact products ``w_a w_b`` in ``fractions.Fraction``, rounded once, and the rule is the
file's ``|ours - exact| <= K 2^-53 A``. The mu count has an exact file of its own, tests/golden/smu_exact.npz, and meets it in
tests/test_gpu_smu_exact.py (both scenes up to the cap, the tie ``ps == 0`` at an edge ``mu == 0`` included); here it is held
to the signed oracle (integers) and to ``yawhip_proj_count_smu`` on the same handles (the fold), its weighted planes by the
rule of tests/test_gpu_smu.py."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import proj_exact as pe
import proj_signed_oracle as pso
import smu_scenes as scenes
import smu_signed_oracle as sso
from proj_signed_oracle import fold, mirrored
from test_gpu_projected import upload
from test_gpu_smu import EPS, K as K_SMU
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
MU_ASYMMETRIC = np.array([-1.0, -0.4, 0.1, 0.25, 1.0])
CAP_AT_13_EDGES = 104  # include/yawhip.h: the largest number of signed bins whose carve-up fits 64 KiB of LDS at 13 edges


def lds_bytes(n_edges, n):
    """The carve-up of include/yawhip.h: two stages of 48-byte objects, thresholds, the signed edges, four histograms."""
    return 2 * 256 * 48 + 8 * (((n_edges + 1) & ~1) + ((n + 2) & ~1)) + 4 * n * (n_edges - 1) * 8


def on_device(a, b, calls, axis_a=2, axis_b=None):
    """``calls`` -- functions of ``(ctx, first, second)`` -- on one upload of the oracle's handles ``a`` (first) and ``b``."""
    ctx = engine.get_context(0)
    first = upload(ctx, a, axis_a)
    second = upload(ctx, b, axis_a if axis_b is None else axis_b)
    try:
        return [call(ctx, first, second) for call in calls]
    finally:
        first.free(), second.free()


def pi_signed(cells, r2, edges):
    return lambda ctx, first, second: _lib.proj_count_pi_signed(ctx, first, second, cells, r2, edges)


def smu_signed(cells, s2, sm2):
    return lambda ctx, first, second: _lib.proj_count_smu_signed(ctx, first, second, cells, s2, sm2)


def check_stats(stats, cells):
    assert stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs


# --------------------------------------------------------------------------- 1. pi: the exact reference
@functools.lru_cache(maxsize=None)
def exact_pi(name, fold_bins, edges):
    """``(N, W, A)`` [2 n, n_cells, nf] of the scene's two handles over the mirrored edge set ``edges``: the oracle's member
    pairs per signed plane, the exact sum of ``w_a w_b`` over them (``Fraction``, rounded once) and -- every stored weight is
    > 0 -- the same as ``A``. Computed once per case, shared, never modified."""
    fx = pe.fixture()
    a, b = (pe.scene(fx, name, cat, fold_bins, True) for cat in "ab")
    assert a["w"].min() > 0 and b["w"].min() > 0
    cells, r2, signed_edges = pe.cells(fx, name, fold_bins, True), fx[f"{name}.r2"], mirrored(fx[f"pi.{edges}"])
    n, nf = len(signed_edges) - 1, r2.shape[1] - 1
    N, W = np.zeros((n, len(cells), nf)), np.zeros((n, len(cells), nf))
    for c, (i, j, plane, e) in enumerate(pso.member_pairs(a, b, cells, r2, signed_edges)):
        sums = {}
        for wa, wb, slot in zip(a["w"][i], b["w"][j], zip(plane, e)):
            sums[slot] = sums.get(slot, 0) + Fraction(float(wa)) * Fraction(float(wb))
        for (plane_, e_), total in sums.items():
            W[plane_, c, e_] = float(total)
        np.add.at(N, (plane, c, e), 1.0)
    for arr in (N, W):
        arr.setflags(write=False)
    return N, W, W


def run_pi(name, fold_bins, weighted, axis_a, axis_b=None):
    """The signed count of the scene's two handles over the three stored edge sets mirrored -> ``{edge set: W}``."""
    fx = pe.fixture()
    a, b = (pe.scene(fx, name, cat, fold_bins, weighted) for cat in "ab")
    cells, r2 = pe.cells(fx, name, fold_bins, True), fx[f"{name}.r2"]
    out = on_device(a, b, [pi_signed(cells, r2, mirrored(fx[f"pi.{edges}"])) for edges in pe.PI_SETS], axis_a, axis_b)
    for _, stats in out:
        check_stats(stats, cells)
    return {edges: W for edges, (W, _) in zip(pe.PI_SETS, out)}, [stats for _, stats in out]


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("fold_bins", [False, True], ids=["nb=2", "nb=1"])
@pytest.mark.parametrize("name", pe.SCENES)
def test_signed_pi_counts_and_sums_are_the_exact_ones(name, fold_bins, sort_axis):
    fx = pe.fixture()
    K = float(fx["K"])
    key = f"signed pi {name} nb={1 if fold_bins else 2} axis={sort_axis}"
    unit, _ = run_pi(name, fold_bins, False, sort_axis)
    weighted, _ = run_pi(name, fold_bins, True, sort_axis)
    worst = 0.0
    for edges in pe.PI_SETS:
        N, W, A = exact_pi(name, fold_bins, edges)
        n = len(N) // 2
        assert N.sum() > 1000 and N[:n].sum() != N[n:].sum()
        assert np.array_equal(unit[edges], N), (key, edges, np.abs(unit[edges] - N).sum())
        assert np.array_equal(fold(unit[edges]), pe.counts_pi(fx, name, fold_bins, True, edges)), (key, edges)
        worst = max(worst, pe.check(f"{key} {edges}", weighted[edges], W, A, K))
    print(f"{key}: worst ratio over the edge sets {worst:.3f}")


@pytest.mark.parametrize("fold_bins", [False, True], ids=["nb=2", "nb=1"])
def test_signed_pi_the_whole_segment_streamed_gives_the_windowed_bits(fold_bins):
    """``wide`` with the two handles on different sort axes: no window, every pair of a cell evaluated, the same bits."""
    windowed, st_windowed = run_pi("wide", fold_bins, False, 2, 2)
    whole, st_whole = run_pi("wide", fold_bins, False, 2, 0)
    for edges, st_w, st_all in zip(pe.PI_SETS, st_windowed, st_whole):
        assert st_all.evaluated_pairs == st_all.candidate_pairs >= st_w.evaluated_pairs > 0
        assert np.array_equal(whole[edges], windowed[edges]) and np.array_equal(whole[edges], exact_pi("wide", fold_bins, edges)[0])


# --------------------------------------------------------------------------- 2. mu: the oracle and the unsigned sibling
MU_SETS = {**{name: mirrored(mu) for name, mu in scenes.MU_SETS.items()}, "asymmetric": MU_ASYMMETRIC}


@functools.lru_cache(maxsize=None)
def expected_mu(nb, weighted, mu):
    a, b = scenes.scene(nb, weighted)
    out = sso.smu_signed_cells(a, b, scenes.cells_two_handles(nb), scenes.s_edges(6, nb), sso.signed_squares(MU_SETS[mu]))
    for arr in out:
        arr.setflags(write=False)
    return out


@pytest.mark.parametrize("sort_axis", [0, 2])
@pytest.mark.parametrize("nb", [1, 2])
def test_signed_mu_membership_is_the_oracles_and_folds_to_the_unsigned_count(nb, sort_axis):
    a, b = scenes.scene(nb, False)
    cells, s2 = scenes.cells_two_handles(nb), scenes.s_edges(6, nb)
    calls = [smu_signed(cells, s2, sso.signed_squares(mu)) for mu in MU_SETS.values()]
    calls += [lambda ctx, first, second, mu=mu: _lib.proj_count_smu(ctx, first, second, cells, s2, scenes.squares(mu)) for mu in scenes.MU_SETS.values()]
    out = on_device(a, b, calls, sort_axis)
    signed, unsigned = dict(zip(MU_SETS, out)), dict(zip(scenes.MU_SETS, out[len(MU_SETS):]))
    for name, (W, stats) in signed.items():
        check_stats(stats, cells)
        exp_w, _, exp_n = expected_mu(nb, False, name)
        assert exp_n.sum() > 1000 and np.all(exp_n.sum(axis=(1, 2)) > 0), name  # every signed plane holds pairs
        assert np.array_equal(W, exp_n) and np.array_equal(exp_w, exp_n), (name, np.abs(W - exp_n).sum())
        if name in unsigned:
            plain, plain_stats = unsigned[name]
            assert np.array_equal(fold(W), plain), name
            assert (stats.candidate_pairs, stats.evaluated_pairs) == (plain_stats.candidate_pairs, plain_stats.evaluated_pairs)
        else:
            assert np.array_equal(W.sum(axis=0), signed["uniform4"][0].sum(axis=0))  # the same pairs in other planes


@pytest.mark.parametrize("mu", ["uniform30", "uneven", "asymmetric"])
@pytest.mark.parametrize("nb", [1, 2])
def test_signed_mu_weighted_sums_match_the_oracle(nb, mu):
    a, b = scenes.scene(nb, True)
    cells = scenes.cells_two_handles(nb)
    exp_w, exp_a, exp_n = expected_mu(nb, True, mu)
    ((W, _),) = on_device(a, b, [smu_signed(cells, scenes.s_edges(6, nb), sso.signed_squares(MU_SETS[mu]))])
    assert np.array_equal(W == 0.0, exp_n == 0.0) and not np.any(np.signbit(W[exp_n == 0.0]))  # exact +0.0 where the oracle is empty
    worst = float(np.max(np.abs(W - exp_w)[exp_a > 0] / (EPS * exp_a[exp_a > 0])))
    print(f"signed mu nb={nb} {mu}: worst |ours - oracle| / (eps A) = {worst:.3f}")
    assert np.all(np.abs(W - exp_w) <= K_SMU * EPS * exp_a)


# --------------------------------------------------------------------------- 3. the sign belongs to the handle order
def swapped(cells):
    return np.ascontiguousarray(cells[:, [1, 0, 2, 3]])


@pytest.mark.parametrize("axes", [(2, 2), (0, 2)], ids=["windowed", "whole"])
def test_exchanging_the_handles_reverses_the_planes(axes):
    """``count(a, b, edges)`` against ``count(b, a, -edges[::-1])`` with the cells' segments exchanged: plane j of one is plane
    ``n - 1 - j`` of the other as integers, for both kernels -- whichever side the walk streams."""
    a, b = scenes.scene(2, False)
    cells, t = scenes.cells_two_handles(2), scenes.s_edges(6, 2)
    pe_ = np.array([-3.0, -1.2, -0.1, 0.4, 2.0, 3.5])
    sm2 = sso.signed_squares(MU_ASYMMETRIC)
    (pi_ab, _), (mu_ab, _) = on_device(a, b, [pi_signed(cells, t, pe_), smu_signed(cells, t, sm2)], *axes)
    (pi_ba, _), (mu_ba, _) = on_device(b, a, [pi_signed(swapped(cells), t, -pe_[::-1]), smu_signed(swapped(cells), t, -sm2[::-1])], *axes[::-1])
    margin, least = pso.nearest_signed_pi_margin(a, b, cells, pe_)
    assert margin > 0.0 and least > 0.0  # no pair on an edge: the closed and the open end of a bin hold the same pairs
    assert pi_ab.sum() > 1000 and np.all(pi_ab.sum(axis=(1, 2)) > 0) and not np.array_equal(pi_ab, pi_ab[::-1])
    assert np.array_equal(pi_ab, pi_ba[::-1]) and np.array_equal(pi_ab, pso.proj_pi_signed_cells(a, b, cells, t, pe_)[2])
    assert mu_ab.sum() > 1000 and not np.array_equal(mu_ab, mu_ab[::-1])
    assert np.array_equal(mu_ab, mu_ba[::-1]) and np.array_equal(mu_ab, sso.smu_signed_cells(a, b, cells, t, sm2)[2])


# --------------------------------------------------------------------------- 4. shapes that can go wrong
def test_one_bin_one_sided_ranges_and_thirty_bins():
    a, b = scenes.scene(2, False)
    cells, t = scenes.cells_two_handles(2), scenes.s_edges(6, 2)
    ps_all = np.concatenate([pso.signed_terms(a, b, np.arange(a["off"][sa], a["off"][sa + 1])[:, None], np.arange(b["off"][sb], b["off"][sb + 1])[None, :])[1].ravel()
                             for sa, sb, _, _ in cells])
    assert ps_all.min() < -3.0 and ps_all.max() > 3.0
    pi_sets = [np.array([-1.5, 2.5]), np.array([0.5, 2.0]), np.array([-2.0, -0.5]), np.array([0.5, 1.0, 2.0]), np.array([-2.0, -1.0, -0.5]),
               np.linspace(-3.0, 3.0, 31)]
    mu_sets = [np.array([-1.0, 1.0]), np.linspace(-1.0, 1.0, 31)]
    out = on_device(a, b, [pi_signed(cells, t, edges) for edges in pi_sets] + [smu_signed(cells, t, sso.signed_squares(mu)) for mu in mu_sets]
                    + [lambda ctx, first, second: _lib.proj_count_smu(ctx, first, second, cells, t, np.array([0.0, 1.0]))])
    for edges, (W, _) in zip(pi_sets, out):
        exp = pso.proj_pi_signed_cells(a, b, cells, t, edges)[2]
        assert W.shape == exp.shape and exp.sum() > 100 and np.array_equal(W, exp), edges
    # the mirror of a one-sided range holds other pairs: the lower cut is what keeps them apart
    assert not np.array_equal(out[1][0], out[2][0]) and not np.array_equal(out[3][0], out[4][0][::-1])
    for mu, (W, _) in zip(mu_sets, out[len(pi_sets):]):
        exp = sso.smu_signed_cells(a, b, cells, t, sso.signed_squares(mu))[2]
        assert exp.sum() > 1000 and np.array_equal(W, exp), len(mu)
    assert np.array_equal(out[len(pi_sets)][0], out[-1][0])  # one signed mu bin is the one unsigned bin: no cut


def test_the_largest_number_of_bins_that_fits_runs_and_one_more_is_refused():
    cap = CAP_AT_13_EDGES
    assert lds_bytes(13, cap) <= 65536 < lds_bytes(13, cap + 1)
    a, b = scenes.scene(1, False)
    cells, t = scenes.cells_two_handles(1), scenes.s_edges(12, 1)
    at_cap = lambda n: (np.linspace(-3.0, 3.0, n + 1), sso.signed_squares(np.linspace(-1.0, 1.0, n + 1)))

    def refused(call, bins, rows):
        def run(ctx, first, second):
            with pytest.raises(_lib.YawhipError, match=f"{cap + 1} {bins} bins of 12 {rows} bins do not fit the LDS of a workgroup: at most {cap} {bins} bins at n_edges=13"):
                call(ctx, first, second)
        return run

    (W_pi, _), (W_mu, _), _, _ = on_device(a, b, [pi_signed(cells, t, at_cap(cap)[0]), smu_signed(cells, t, at_cap(cap)[1]),
                                                  refused(pi_signed(cells, t, at_cap(cap + 1)[0]), "pi", "radius"),
                                                  refused(smu_signed(cells, t, at_cap(cap + 1)[1]), "mu", "s")])
    exp = pso.proj_pi_signed_cells(a, b, cells, t, at_cap(cap)[0])[2]
    assert exp.sum() > 1000 and np.count_nonzero(exp.sum(axis=(1, 2))) >= 90 and np.array_equal(W_pi, exp)
    exp = sso.smu_signed_cells(a, b, cells, t, at_cap(cap)[1])[2]
    assert exp.sum() > 1000 and np.count_nonzero(exp.sum(axis=(1, 2))) >= 90 and np.array_equal(W_mu, exp)


def test_cells_without_an_order_and_bad_edges_are_refused():
    a, b = scenes.scene(2, False)
    cells, t = scenes.cells_two_handles(2), scenes.s_edges(6, 2)
    pe_, sm2 = np.array([-2.0, 0.0, 2.0]), np.array([-1.0, 0.0, 1.0])
    marked = cells.copy()
    marked[3, 3] = 1
    itself = scenes.cells_one_handle(2)
    assert np.any(itself[:, 0] == itself[:, 1]) and np.any(itself[:, 0] != itself[:, 1])
    off_diagonal = itself[itself[:, 0] != itself[:, 1]]
    off_diagonal[:, 3] = 0

    def run(ctx, first, second):
        for count, edges in ((_lib.proj_count_pi_signed, pe_), (_lib.proj_count_smu_signed, sm2)):
            with pytest.raises(_lib.YawhipError, match="cell 3 pairs a segment with itself or is marked diagonal"):
                count(ctx, first, second, marked, t, edges)
            with pytest.raises(_lib.YawhipError, match="cell 0 pairs a segment with itself or is marked diagonal"):
                count(ctx, first, first, itself, t, edges)  # a segment against itself on one handle
            unmarked = itself.copy()
            unmarked[:, 3] = 0
            with pytest.raises(_lib.YawhipError, match="cell 0 pairs a segment with itself or is marked diagonal"):
                count(ctx, first, first, unmarked, t, edges)
            W, _ = count(ctx, first, first, off_diagonal, t, edges)  # two segments of ONE handle have an order
            oracle = pso.proj_pi_signed_cells if count is _lib.proj_count_pi_signed else sso.smu_signed_cells
            assert W.sum() > 100 and np.array_equal(W, oracle(a, a, off_diagonal, t, edges)[2])
        for bad in ([-2.0, np.inf], [-np.inf, 2.0], [-2.0, np.nan, 2.0], [-2.0, 1.0, 1.0, 2.0], [2.0, -2.0], [1.0]):
            with pytest.raises(_lib.YawhipError, match="signed pi edges must be finite and strictly ascending|n_pi must be >= 1"):
                _lib.proj_count_pi_signed(ctx, first, second, cells, t, np.array(bad))
        for bad in ([0.0, 0.5, 1.0], [-1.0, 0.5, 0.9], [-1.0, 0.5, 0.5, 1.0], [-1.0, np.nan, 1.0], [-1.0]):
            with pytest.raises(_lib.YawhipError, match="signed squared mu edges must|n_mu must be >= 1"):
                _lib.proj_count_smu_signed(ctx, first, second, cells, t, np.array(bad))
        mu = np.array([-1.0, -1e-200, 1e-200, 1.0])  # ascends strictly, its squares do not
        with pytest.raises(_lib.YawhipError, match="signed squared mu edges must be finite and strictly ascending"):
            _lib.proj_count_smu_signed(ctx, first, second, cells, t, sso.signed_squares(mu))
        return True

    assert on_device(a, b, [run]) == [True]


def test_handles_without_objects_and_an_empty_cell_list():
    a, b = scenes.scene(2, False)
    cells, t = scenes.cells_two_handles(2), scenes.s_edges(6, 2)
    none = np.empty(0, dtype=np.float64)
    nobody = dict({c: none for c in "xyzdc"}, w=None, nb=2, off=np.zeros(len(a["off"]), dtype=np.int64))
    pe_, sm2 = np.array([-2.0, 0.0, 2.0]), np.array([-1.0, 0.0, 1.0])
    for first, second in ((a, nobody), (nobody, b), (nobody, dict(nobody))):
        for W, stats in on_device(first, second, [pi_signed(cells, t, pe_), smu_signed(cells, t, sm2)]):
            assert stats.evaluated_pairs == 0 and stats.candidate_pairs == 0 and stats.n_workgroups == len(cells)
            assert W.shape == (2, len(cells), 6) and np.all(W == 0.0) and not np.any(np.signbit(W))
    no_cells = np.empty((0, 4), dtype=np.int32)
    for W, stats in on_device(a, b, [pi_signed(no_cells, t, pe_), smu_signed(no_cells, t, sm2)]):
        assert W.shape == (2, 0, 6) and stats.n_workgroups == 0 and stats.candidate_pairs == 0


# --------------------------------------------------------------------------- 5. the entry points in turn on one pair of handles
def test_signed_and_unsigned_entry_points_alternate_on_one_pair_of_handles():
    """Few / full / few cells through the four entry points in turn on ONE pair of handles: the call's input block (with the
    signed edges one value longer or shorter than the last call's) and its result block are laid out anew in the same
    buffers, and every turn is the bits of the same call on fresh handles."""
    a, b = scenes.scene(2, True)
    full, t = scenes.cells_two_handles(2), scenes.s_edges(6, 2)
    few = np.ascontiguousarray(full[[1, 6, 11]])
    pe_, half = np.array([-3.0, -1.2, 0.4, 2.0, 3.5]), np.array([0.0, 1.0, 3.5])
    mu, m2 = sso.signed_squares(MU_ASYMMETRIC), scenes.squares(scenes.MU_UNEVEN)
    pi_unsigned = lambda cells: lambda ctx, first, second: _lib.proj_count_pi(ctx, first, second, cells, t, half)
    smu_unsigned = lambda cells: lambda ctx, first, second: _lib.proj_count_smu(ctx, first, second, cells, t, m2)
    turns = [pi_signed(few, t, pe_), pi_unsigned(full), pi_signed(full, t, pe_), smu_unsigned(few), smu_signed(full, t, mu), pi_unsigned(few),
             smu_signed(few, t, mu), smu_unsigned(full), pi_signed(few, t, pe_)]
    together = on_device(a, b, turns)
    assert np.array_equal(together[0][0], together[-1][0]) and together[2][0].sum() > 1000
    for n, turn in enumerate(turns):
        ((alone, _),) = on_device(a, b, [turn])
        assert alone.shape == together[n][0].shape and np.array_equal(alone, together[n][0]), n


# --------------------------------------------------------------------------- 6. the drivers through the real library
def test_the_drivers_count_the_patch_free_pairs_on_the_device():
    import yet_another_wizz_amd as yaw
    from test_signed_host import DRIVER_MU, DRIVER_PI, HALF_MU, HALF_PI, PI_MAX, check_counts, driver_scenario, patch_free, sides

    config, data1, data2, rand1, rand2 = driver_scenario()
    catalogs = (data1, data2, rand1, rand2)
    try:
        signed_pi = yaw.crosscorrelate_projected(config, *catalogs, pi_max=PI_MAX, pi_bins=DRIVER_PI, signed=True)
        signed_mu = yaw.crosscorrelate_multipoles(config, *catalogs, mu_bins=DRIVER_MU, signed=True)
        plain_pi = yaw.crosscorrelate_projected(config, *catalogs, pi_max=PI_MAX, pi_bins=HALF_PI)
        plain_mu = yaw.crosscorrelate_multipoles(config, *catalogs, mu_bins=HALF_MU)
        pairs = sides(*catalogs)
        hand = {kind: patch_free(config, *cats, pso.proj_pi_signed_cells, DRIVER_PI) for kind, cats in pairs.items()}
        assert all(counts.sum() > 500 for counts in hand.values())
        check_counts(signed_pi, lambda r: r.pi_bins, hand, ("dd", "dr", "rd", "rr"))
        hand = {kind: patch_free(config, *cats, sso.smu_signed_cells, sso.signed_squares(DRIVER_MU)) for kind, cats in pairs.items()}
        check_counts(signed_mu, lambda r: r.mu_bins, hand, ("dd", "dr", "rd", "rr"))
        for signed, plain, bins in ((signed_pi, plain_pi, "pi_bins"), (signed_mu, plain_mu, "mu_bins")):
            for result, unsigned in zip(signed, plain):
                assert type(result.folded()) is type(unsigned)
                for got, exp in zip(getattr(result.folded(), bins), getattr(unsigned, bins)):
                    for kind in ("dd", "dr", "rd", "rr"):
                        assert np.array_equal(getattr(got, kind).counts.counts, getattr(exp, kind).counts.counts), (bins, kind)
                        assert getattr(exp, kind).counts.counts.sum() > 0
        assert all(np.all(np.isfinite(m.data)) for m in signed_mu[0].sample_multipoles()) and np.all(np.isfinite(signed_pi[0].sample().data))
    finally:
        for cat in catalogs:
            cat.drop_layouts()
