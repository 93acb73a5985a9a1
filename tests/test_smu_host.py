"""CPU: the redshift-space clustering (``autocorrelate_multipoles``, ``MultipoleCorrFunc``) above the
device seam -- the C ABI's new name, ``engine.check_mu_edges``, the oracle of tests/smu_oracle.py against itself at one plane
and, pair by pair, against mpmath on the scene that the device tests use, the Legendre weights, the driver with
``engine.count_smu_fine`` replaced by that oracle, and the error cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import proj_oracle
import smu_oracle
import smu_scenes
import yet_another_wizz_amd as yaw
from conftest import ROOT
from helpers import use_oracle_engine
from smu_scenes import MU_4, MU_30, MU_SETS, MU_UNEVEN, squares
from test_dsigma_host import jackknife
from test_projected_host import NEIGHBOURS, ZEDGES
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, engine, measurements

EPS = 2.0**-53
MARGIN = 1e-9


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_smu_fine", smu_oracle.count_smu_fine)
    use_oracle_engine(monkeypatch)


# --------------------------------------------------------------------------- 1. ABI
def test_the_new_symbol_is_declared_bound_and_built_at_abi_6():
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "yawhip_proj_count_smu"
    assert name in _lib.ABI_SYMBOLS
    prototype = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
    assert prototype, name
    arguments = [" ".join(arg.split()) for arg in prototype.group(1).split(",")]
    assert arguments == ["yawhip_ctx *ctx", "yawhip_shear_sources *a", "yawhip_shear_sources *b", "int32_t n_cells", "const int32_t *cells",
                         "int32_t n_rows", "int32_t n_edges", "const double *s2", "int32_t n_mu", "const double *m2", "double *fine_w",
                         "yawhip_stats *stats"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)
    bound = _lib.load_library().yawhip_proj_count_smu
    assert bound.argtypes == _lib.load_library().yawhip_proj_count_pi.argtypes and bound.restype is ctypes.c_int
    assert callable(_lib.proj_count_smu) and callable(engine.count_smu_fine)
    for exported in ("MultipoleCorrFunc", "autocorrelate_multipoles"):
        assert exported in yaw.__all__
    assert yaw.MultipoleCorrFunc is yaw.corrfunc.MultipoleCorrFunc and yaw.autocorrelate_multipoles is measurements.autocorrelate_multipoles


# --------------------------------------------------------------------------- 2. the edges
def test_check_mu_edges_accepts_a_count_or_edges_and_refuses_the_rest():
    for n in (1, 4, np.int64(30)):
        edges = engine.check_mu_edges(n)
        assert edges.dtype == np.float64 and np.array_equal(edges, np.linspace(0.0, 1.0, int(n) + 1))
    assert np.array_equal(engine.check_mu_edges(4), MU_4) and np.array_equal(engine.check_mu_edges(30), MU_30)
    for given in (MU_UNEVEN, list(MU_UNEVEN), tuple(MU_UNEVEN), [0, 1]):
        edges = engine.check_mu_edges(given)
        assert edges.dtype == np.float64 and np.array_equal(edges, np.asarray(given, dtype=np.float64))
    given = MU_UNEVEN.copy()
    engine.check_mu_edges(given)[1] = 0.5
    assert given[1] == 0.05  # the caller's array is not what comes back
    for bad in (0, -3, True, [0.5, 1.0], [0.0, 0.9], [0.0, 1.1], [0.0, 0.3, 0.3, 1.0], [0.0, 0.6, 0.3, 1.0], [0.0, np.nan, 1.0],
                [0.0, 0.5, np.inf], [0.0], [], [[0.0, 1.0]], "four", 2.5, None):
        with pytest.raises(ValueError):
            engine.check_mu_edges(bad)
    for bad, what in ((0, ">= 1"), ([0.5, 1.0], "start at 0"), ([0.0, 0.9], "end at 1"), ([0.0, 0.6, 0.3, 1.0], "ascend"), (True, "number of bins")):
        with pytest.raises(ValueError, match=what):
            engine.check_mu_edges(bad)


# --------------------------------------------------------------------------- 3. the planes against one plane
@pytest.mark.parametrize("nb", [1, 4])
def test_the_planes_sum_to_the_one_plane_count_and_the_scene_stays_off_the_edges(nb):
    """``sum_j N[j]`` is the ``N`` of the ``n_mu = 1`` count, exactly; and the scene conditions of DESIGN.md section 23, in
    float64: no pair within 1e-9 (relative) of an s edge, no ``fl(m2_k S2)`` within 1e-9 of ``P2`` over ALL pairs and inner
    edges, every mu plane and every s bin populated."""
    a, b = smu_scenes.scene(nb, True)
    s2 = smu_scenes.s_edges(12, nb)
    for first, second, cells in ((a, a, smu_scenes.cells_one_handle(nb)), (a, b, smu_scenes.cells_two_handles(nb))):
        one = smu_oracle.smu_cells(first, second, cells, s2, np.array([0.0, 1.0]))
        for name, mu in MU_SETS.items():
            W, A, N = smu_oracle.smu_cells(first, second, cells, s2, squares(mu))
            assert N.shape == (len(mu) - 1, len(cells), 12) and np.array_equal(N.sum(axis=0), one[2][0])
            np.testing.assert_allclose(W.sum(axis=0), one[0][0], rtol=1e-13)
            margin_s, margin_mu = smu_oracle.nearest_margins(first, second, cells, s2, squares(mu))
            per_plane, per_bin = int(N.sum(axis=(1, 2)).min()), int(N.sum(axis=(0, 1)).min())
            print(f"nb={nb} {'one handle' if first is second else 'two handles'} {name}: nearest to an s edge {margin_s:.3e}, to a mu edge "
                  f"{margin_mu:.3e}, fewest pairs in a mu plane {per_plane}, in an s bin {per_bin}")
            assert margin_s > MARGIN and margin_mu > MARGIN and per_plane >= 132 and per_bin >= 5


# --------------------------------------------------------------------------- 4. the oracle's membership, exactly
def exact_pairs(a, b, cells, s2, same):
    """Every pair of the cells at 50 digits: ``(cell, fine bin or -1, S^2, p^2, w_a w_b)`` with ``theta = 2 asin(chord / 2)``,
    ``R^2 = ((d_a + d_b) / 2)^2 theta^2``, ``p = |c_a - c_b|`` and ``S^2 = R^2 + p^2`` of the float64 inputs, and the smallest
    relative distance of any ``S^2`` from an edge > 0 of its row."""
    import mpmath

    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    cols_a = {c: [mpf(float(v)) for v in a[c]] for c in "xyzdc"}
    cols_b = cols_a if same else {c: [mpf(float(v)) for v in b[c]] for c in "xyzdc"}
    wa = [mpf(1)] * len(a["x"]) if a["w"] is None else [mpf(float(v)) for v in a["w"]]
    wb = wa if same else ([mpf(1)] * len(b["x"]) if b["w"] is None else [mpf(float(v)) for v in b["w"]])
    nf = s2.shape[1] - 1
    pairs, margin_s = [], mpf(1)
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        edges = [mpf(float(v)) for v in s2[row]]
        for i in range(int(a["off"][sa]), int(a["off"][sa + 1])):
            ax, ay, az, ad, ac = (cols_a[c][i] for c in "xyzdc")
            for j in range(int(b["off"][sb]), int(b["off"][sb + 1])):
                if diagonal and j >= i:
                    break
                dx, dy, dz = ax - cols_b["x"][j], ay - cols_b["y"][j], az - cols_b["z"][j]
                theta = 2 * mpmath.asin(mpmath.sqrt(dx * dx + dy * dy + dz * dz) / 2)
                D = (ad + cols_b["d"][j]) / 2
                p = ac - cols_b["c"][j]
                P2 = p * p
                S2 = D * D * theta * theta + P2
                below = 0
                for edge in edges:
                    if edge > 0:
                        margin_s = min(margin_s, abs(S2 / edge - 1))
                    below += edge < S2
                pairs.append((n, below - 1 if 0 < below <= nf else -1, S2, P2, wa[i] * wb[j]))
    return pairs, float(margin_s)


def test_the_oracles_membership_is_exact_on_the_device_scene():
    """For the scene of tests/test_gpu_smu.py (four redshift bins, twelve fine bins, one handle and two) every pair is
    classified at 50 digits, in s and in mu -- the plane by ``m2_k S^2 < p^2`` with the float64 squares of the edges taken
    exactly -- for the three mu sets. No pair lies within 1e-9 (relative) of an s edge and no ``m2_k S^2`` within 1e-9 of
    ``p^2``, inside the s range or not, so the comparison leaves out no pair, and the oracle's integer count per mu bin, cell
    and fine bin is the exact one. The oracle's weighted sums are then held against the exact sums: the worst
    ``|W - exact| / (eps A)`` is printed; four times it, rounded up to a power of two, is the ``K`` of the device tests."""
    import mpmath

    import test_gpu_smu

    nb = 4
    a, b = smu_scenes.scene(nb, True)
    s2 = smu_scenes.s_edges(12, nb)
    worst = 0.0
    for first, second, cells in ((a, a, smu_scenes.cells_one_handle(nb)), (a, b, smu_scenes.cells_two_handles(nb))):
        same = first is second
        pairs, margin_s = exact_pairs(first, second, cells, s2, same)
        assert margin_s > MARGIN and min(P2 for _, _, _, P2, _ in pairs) > 0
        for name, mu in MU_SETS.items():
            m2 = squares(mu)
            n_mu = len(m2) - 1
            inner = [mpmath.mpf(float(v)) for v in m2[1:-1]]
            margin_mu = float(min(abs(edge * S2 / P2 - 1) for _, _, S2, P2, _ in pairs for edge in inner))
            count = np.zeros((n_mu, len(cells), 12), dtype=np.int64)
            sums = {}
            for n, e, S2, P2, ww in pairs:
                if e >= 0:
                    plane = sum(edge * S2 < P2 for edge in inner)
                    count[plane, n, e] += 1
                    sums[plane, n, e] = sums.get((plane, n, e), 0) + ww
            print(f"{'one handle' if same else 'two handles'} {name}: {count.sum()} member pairs of {len(pairs)}, nearest to a mu edge "
                  f"{margin_mu:.3e}, fewest pairs in a mu plane {count.sum(axis=(1, 2)).min()}")
            assert margin_mu > MARGIN
            W, A, N = smu_oracle.smu_cells(first, second, cells, s2, m2)
            assert count.sum() > 3000 and np.array_equal(N, count.astype(np.float64))
            unit = smu_oracle.smu_cells(smu_scenes.unweighted(first), smu_scenes.unweighted(second), cells, s2, m2, same=same)
            assert np.array_equal(unit[0], N)  # unit weights: W is the count
            for slot, exact in sums.items():
                worst = max(worst, float(abs(exact - float(W[slot]))) / (EPS * A[slot]))
    print(f"the oracle's worst |W - exact| / (eps A): {worst:.3f}")
    assert worst <= test_gpu_smu.K_ORACLE_RATIO * 1.0000001  # the figure K was derived from still holds
    assert test_gpu_smu.K == 2.0 ** np.ceil(np.log2(4.0 * test_gpu_smu.K_ORACLE_RATIO))


# --------------------------------------------------------------------------- 5. the Legendre weights
def legendre_by_hand(ell, x):
    """The antiderivative of ``P_ell`` written out: 0, 2, 4 only."""
    x = np.asarray(x, dtype=np.float64)
    return {0: x, 2: 0.5 * (x**3 - x), 4: (7.0 * x**5 - 10.0 * x**3 + 3.0 * x) / 8.0}[ell]


def placeholder(binning_cf, mu):
    return yaw.MultipoleCorrFunc(mu, [binning_cf] * (len(mu) - 1))


def test_the_legendre_weights_integrate_the_polynomials(stand_in):
    """``sum_j I_0j = 1`` and ``sum_j I_ellj = 0`` for ``ell`` = 2, 4 on the three mu sets, to 1e-15: a mu-independent ``xi``
    has no quadrupole and no hexadecapole. Odd ``ell`` and ``ell > 8`` are refused."""
    config, data, random = unit_scenario()
    (first, _) = yaw.autocorrelate_multipoles(config, data, random, mu_bins=1)
    for mu in MU_SETS.values():
        mcf = placeholder(first.mu_bins[0], mu)
        for ell in (0, 2, 4):
            weights = mcf.legendre_weights(ell)
            assert weights.shape == (len(mu) - 1,)
            np.testing.assert_allclose(weights, np.diff(legendre_by_hand(ell, mu)), rtol=0, atol=1e-15)
            assert abs(weights.sum() - (1.0 if ell == 0 else 0.0)) <= 1e-15
        for ell in (6, 8, np.int64(2)):
            assert abs(mcf.legendre_weights(ell).sum()) <= 1e-14
        # every plane holds the same xi: the monopole is xi, the others vanish
        xi = first.mu_bins[0].sample()
        np.testing.assert_allclose(mcf.sample(0).data, xi.data, rtol=1e-14)
        np.testing.assert_allclose(mcf.sample().samples, xi.samples, rtol=1e-14)
        for ell in (2, 4):
            assert np.all(np.abs(mcf.sample(ell).data) <= 1e-14 * np.abs(xi.data))
        for bad in (1, 3, 10, -2, 2.0, True, "2", None):
            with pytest.raises(ValueError, match="even integer in 0 ... 8"):
                mcf.sample(bad)


# --------------------------------------------------------------------------- 6. the driver on the oracle stand-in
DRIVER_MU = np.array([0.0, 0.2, 0.65, 1.0])  # uneven widths


def driver_scenario():
    """The three neighbouring patches of tests/test_projected_host.py, two redshift bins: 90 weighted data objects and 150
    randoms around every centre, the redshifts in two thin shells (0.3 and 0.5, 0.0008 wide: 3 Mpc along the line of sight
    against scales of up to 2 Mpc), so that every mu plane holds pairs within and across the patches."""
    rng = np.random.default_rng(37)
    kw = dict(patch_centers=yaw.AngularCoordinates(np.array(NEIGHBOURS)), degrees=False)
    cats = []
    for n, weighted in ((90, True), (150, False)):
        ra, dec = (np.concatenate(c) for c in zip(*(ring_around(rng, ra_c, dec_c, n, 1e-5, 1.8e-3) for ra_c, dec_c in NEIGHBOURS)))
        z = rng.choice([0.3, 0.5], len(ra)) + rng.uniform(-0.0004, 0.0004, len(ra))
        cats.append(yaw.Catalog.from_arrays(ra, dec, redshifts=z, weights=rng.uniform(0.5, 1.5, len(ra)) if weighted else None, **kw))
    return cats


def driver_config(unit, rweight=-0.8):
    if unit == "kpc":
        return yaw.Configuration.create(rmin=[100.0, 300.0], rmax=[2000.0, 1000.0], unit="kpc", rweight=rweight, resolution=12, edges=ZEDGES)
    return yaw.Configuration.create(rmin=[0.15, 0.4], rmax=[2.8, 1.5], unit="Mpc/h", rweight=rweight, resolution=12, edges=ZEDGES)


def unit_scenario():
    """``driver_scenario`` without weights, and a configuration without ``rweight``: every count is an integer."""
    _, random = driver_scenario()
    rng = np.random.default_rng(43)
    ra, dec = (np.concatenate(c) for c in zip(*(ring_around(rng, ra_c, dec_c, 90, 1e-5, 1.8e-3) for ra_c, dec_c in NEIGHBOURS)))
    z = rng.choice([0.3, 0.5], len(ra)) + rng.uniform(-0.0004, 0.0004, len(ra))
    data = yaw.Catalog.from_arrays(ra, dec, redshifts=z, patch_centers=yaw.AngularCoordinates(np.array(NEIGHBOURS)), degrees=False)
    return driver_config("kpc", rweight=None), data, random


def by_hand_smu(config, cat1, cat2, mu_edges):
    """The counts [n_mu, S, B, P, P] from the oracle's fine sums and the radial plan over all nine patch pairs (the upper
    triangle of an auto count), and their one normalisation [B, P, P] (``test_projected_pi_host.by_hand_pi``'s method)."""
    auto = cat2 is None
    plans = measurements.radial_plans(config)
    s2 = measurements.threshold_table(plans)
    unit = config.scales.scales.unit
    layouts = [cat.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True) for cat in ((cat1,) if auto else (cat1, cat2))]
    handles = [proj_oracle.as_handle(layout, *engine.proj_columns(layout, config.cosmology, unit)) for layout in layouts]
    jobs = [(p, q) for p in range(3) for q in range(p if auto else 0, 3)]
    cells = np.array([(p * 2 + k, q * 2 + k, k, auto and p == q) for p, q in jobs for k in range(2)])
    W, _, _ = smu_oracle.smu_cells(handles[0], handles[-1], cells, s2, squares(mu_edges))
    counts = np.zeros((len(W), len(plans), 2, 3, 3))
    for j, plane in enumerate(W):
        per_scale = measurements.CombinePlan(plans)(np.moveaxis(plane.reshape(len(jobs), 2, -1), 0, -1))  # [S, B, J]
        for n, (p, q) in enumerate(jobs):
            counts[j, :, :, p, q] = per_scale[:, :, n]
    sums = [np.array([[(layout.w[lo:hi].sum() if layout.w is not None else float(hi - lo))
                       for lo, hi in zip(layout.offsets[p * 2:p * 2 + 2], layout.offsets[p * 2 + 1:p * 2 + 3])] for p in range(3)]).T
            for layout in layouts]  # [B, P]
    norm = sums[0][:, :, None] * sums[-1][:, None, :]
    if auto:
        norm = np.triu(norm)
        norm[:, np.arange(3), np.arange(3)] *= 0.5
    return counts, norm


def check_smu_driver(unit, count_rr, mu_bins=DRIVER_MU, rtol=1e-12):
    """``autocorrelate_multipoles`` against the oracle's fine sums recombined by hand: the counts of every mu plane,
    ``sample_xi()`` against Landy-Szalay (Davis-Peebles without RR), and every multipole against
    ``(2 ell + 1) sum_j xi_j I_ellj`` with the weights written out, data and jackknife samples; ``engine.count_smu_fine`` is
    whatever the caller left in place."""
    data, random = driver_scenario()
    config = driver_config(unit)
    mu_edges = engine.check_mu_edges(mu_bins)
    n_mu = len(mu_edges) - 1
    result = yaw.autocorrelate_multipoles(config, data, random, mu_bins=mu_bins, count_rr=count_rr)
    assert len(result) == 2
    hand = dict(dd=by_hand_smu(config, data, None, mu_edges), dr=by_hand_smu(config, data, random, mu_edges))
    if count_rr:
        hand["rr"] = by_hand_smu(config, random, None, mu_edges)
    for s, mcf in enumerate(result):
        assert type(mcf) is yaw.MultipoleCorrFunc and len(mcf.mu_bins) == n_mu == mcf.num_mu and np.array_equal(mcf.mu_edges, mu_edges)
        per_plane = []
        for j, cf in enumerate(mcf.mu_bins):
            assert type(cf) is yaw.CorrFunc and cf.rd is None and (cf.rr is not None) == count_rr
            assert cf.dd.auto and not cf.dr.auto
            ratio = {}
            for kind, (counts, norm) in hand.items():
                got = getattr(cf, kind)
                assert got.sum_weights is getattr(mcf.mu_bins[0], kind).sum_weights  # ONE normalisation for all planes
                assert np.count_nonzero(counts[j, s]) >= (2 * 4 if got.auto else 2 * 6)  # pairs across the patch borders too
                np.testing.assert_allclose(got.counts.counts, counts[j, s], rtol=rtol, atol=0, err_msg=f"{kind} mu bin {j}")
                (c_tot, c_jk), (n_tot, n_jk) = jackknife(counts[j, s]), jackknife(norm)
                ratio[kind] = (c_tot / n_tot, c_jk / n_jk)
            dd, dr = (np.array([ratio[kind][0], *ratio[kind][1]]) for kind in ("dd", "dr"))  # [1 + P, B]: data, then samples
            if count_rr:  # each ratio is held to rtol: the estimator moves by that of their magnitudes over RR
                rr = np.array([ratio["rr"][0], *ratio["rr"][1]])
                expected, bound = ((dd - dr) + (rr - dr)) / rr, 4.0 * rtol * (np.abs(dd) + 2.0 * np.abs(dr) + np.abs(rr)) / np.abs(rr)
            else:
                expected, bound = (dd - dr) / dr, 4.0 * rtol * np.abs(dd / dr)
            xi = mcf.sample_xi()[j]
            assert type(xi) is yaw.CorrData and xi.samples.shape == (3, 2) and np.all(np.isfinite(xi.data))
            assert np.all(np.abs(np.array([xi.data, *xi.samples]) - expected) <= bound)
            assert np.array_equal(xi.data, cf.sample().data) and np.array_equal(xi.samples, cf.sample().samples)
            per_plane.append((expected, bound))
        multipoles = mcf.sample_multipoles()
        assert len(multipoles) == 3
        for ell, got in zip((0, 2, 4), multipoles):
            assert type(got) is yaw.CorrData and got.samples.shape == (3, 2)
            weights = np.diff(legendre_by_hand(ell, mu_edges))
            expected = (2 * ell + 1) * sum(w * e for w, (e, _) in zip(weights, per_plane))
            scale = (2 * ell + 1) * sum(abs(w) * np.abs(e) for w, (e, _) in zip(weights, per_plane))
            bound = (2 * ell + 1) * sum(abs(w) * b for w, (_, b) in zip(weights, per_plane)) + 1e-12 * scale
            assert np.all(np.abs(np.array([got.data, *got.samples]) - expected) <= bound), ell
            assert np.array_equal(got.data, mcf.sample(ell).data)
            # errors and covariance are those of the summed samples
            summed = yaw.CorrData(mcf.binning, got.data, got.samples)
            assert np.array_equal(got.error, summed.error) and np.array_equal(got.covariance, summed.covariance)
    return result


@pytest.mark.parametrize("count_rr", [True, False], ids=["LS", "DP"])
@pytest.mark.parametrize("unit", ["kpc", "Mpc/h"])
def test_the_multipole_driver_on_the_oracle_stand_in(stand_in, unit, count_rr):
    check_smu_driver(unit, count_rr)


def test_an_int_gives_equal_bins_and_the_planes_share_one_normalisation(stand_in):
    data, random = driver_scenario()
    config = driver_config("kpc")
    (first, _) = yaw.autocorrelate_multipoles(config, data, random, mu_bins=4)
    assert np.array_equal(first.mu_edges, MU_4) and first.num_mu == 4
    layout = data.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    links = yaw.PatchLinkage.from_catalogs(config, data, max_angle=measurements.radial_max_angle(config, layout))
    binned = links.count_smu_pairs(data, mu_bins=3)
    assert len(binned) == 2 and all(len(per_mu) == 3 and all(type(nc) is yaw.NormalisedCounts for nc in per_mu) for per_mu in binned)
    assert len({id(nc.sum_weights) for per_mu in binned for nc in per_mu}) == 1  # all planes share the one PatchedSumWeights
    one = links.count_smu_pairs(data, mu_bins=1)
    for per_mu, (single,) in zip(binned, one):  # the planes sum to the one-plane count
        np.testing.assert_allclose(sum(nc.counts.counts for nc in per_mu), single.counts.counts, rtol=1e-12)


# --------------------------------------------------------------------------- 7. the result class
def test_multipole_corrfunc_round_trips_compares_and_subsets(stand_in):
    config, data, random = unit_scenario()
    (mcf, other) = yaw.autocorrelate_multipoles(config, data, random, mu_bins=DRIVER_MU)
    state = mcf.to_dict()
    assert set(state) == {"mu_edges", "mu_bins"} and len(state["mu_bins"]) == 3 and set(state["mu_bins"][0]) == {"dd", "dr", "rr"}
    again = yaw.MultipoleCorrFunc.from_dict(state)
    assert again == mcf and again is not mcf and not (mcf == other) and mcf != other
    assert (mcf == mcf.mu_bins[0]) is False and mcf.is_compatible(other) and not mcf.is_compatible(mcf.mu_bins[0])
    moved = yaw.MultipoleCorrFunc([0.0, 0.25, 0.65, 1.0], mcf.mu_bins)
    assert moved != mcf and not mcf.is_compatible(moved)
    with pytest.raises(ValueError, match="mu edges differ"):
        mcf.is_compatible(moved, require=True)
    with pytest.raises(ValueError):
        mcf.mu_edges[1] = 0.3  # the edges are read-only
    assert (mcf.num_bins, mcf.num_patches, mcf.auto, mcf.binning) == (2, 3, True, mcf.mu_bins[0].binning)
    one_bin = mcf.bins_subset(slice(1, 2))
    assert type(one_bin) is yaw.MultipoleCorrFunc and one_bin.num_bins == 1 and one_bin.num_mu == 3
    assert all(sub == cf.bins_subset(slice(1, 2)) for sub, cf in zip(one_bin.mu_bins, mcf.mu_bins))
    assert np.array_equal(one_bin.sample(2).data, mcf.sample(2).data[1:2])
    two_patches = mcf.patches_subset([0, 2])
    assert two_patches.num_patches == 2 and all(sub == cf.patches_subset([0, 2]) for sub, cf in zip(two_patches.mu_bins, mcf.mu_bins))
    assert two_patches.sample().samples.shape == (2, 2)
    # what the constructor refuses
    with pytest.raises(ValueError):
        yaw.MultipoleCorrFunc(mcf.mu_edges[:-1], mcf.mu_bins)
    for edges in ([0.1, 0.2, 0.65, 1.0], [0.0, 0.2, 0.65, 0.9], [0.0, 0.65, 0.65, 1.0], [0.0, np.nan, 0.65, 1.0]):
        with pytest.raises(ValueError, match="start at 0, end at 1"):
            yaw.MultipoleCorrFunc(edges, mcf.mu_bins)
    with pytest.raises(TypeError):
        yaw.MultipoleCorrFunc([0.0, 1.0], [mcf.mu_bins[0].dd])
    with pytest.raises(ValueError):
        yaw.MultipoleCorrFunc([0.0, 0.5, 1.0], [mcf.mu_bins[0], yaw.CorrFunc(mcf.mu_bins[1].dd, mcf.mu_bins[1].dr)])
    with pytest.raises(ValueError):
        yaw.MultipoleCorrFunc([0.0, 0.5, 1.0], [mcf.mu_bins[0], one_bin.mu_bins[1]])


def test_a_mu_bin_with_empty_rr_gives_nan_there_and_in_every_multipole(stand_in):
    """Nothing is masked: a mu bin narrower than any pair of the randoms has RR = 0 and ``xi = x / 0`` there; every multipole
    carries it, as ``CorrFunc.sample()`` would."""
    config, data, random = unit_scenario()
    edges = np.array([0.0, 1e-9, 0.5, 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        (mcf, _) = yaw.autocorrelate_multipoles(config, data, random, mu_bins=edges)
        assert mcf.mu_bins[0].rr.counts.counts.sum() == 0.0 and mcf.mu_bins[1].rr.counts.counts.sum() > 0.0
        xi = mcf.sample_xi()
        assert not np.any(np.isfinite(xi[0].data)) and np.all(np.isfinite(xi[1].data)) and np.all(np.isfinite(xi[2].data))
        for multipole in mcf.sample_multipoles((0, 2, 4, 6, 8)):
            assert not np.any(np.isfinite(multipole.data))


# --------------------------------------------------------------------------- 8. error cases
def test_the_multipole_drivers_reject_what_they_cannot_use(stand_in, monkeypatch):
    data, random = driver_scenario()
    config = driver_config("kpc")
    angular = yaw.Configuration.create(rmin=[1.0], rmax=[5.0], unit="arcmin", edges=config.binning.edges)
    with pytest.raises(ValueError, match="physical or comoving unit"):
        yaw.autocorrelate_multipoles(angular, data, random, mu_bins=4)
    links = yaw.PatchLinkage.from_catalogs(config, data, random)
    for bad, what in (([0.5, 1.0], "start at 0"), ([0.0, 0.5, 0.9], "end at 1"), ([0.0, 0.6, 0.3, 1.0], "ascend"),
                      ([0.0, 0.3, 0.3, 1.0], "ascend"), (0, ">= 1"), (True, "number of bins")):
        with pytest.raises(ValueError, match=what):
            yaw.autocorrelate_multipoles(config, data, random, mu_bins=bad)
        with pytest.raises(ValueError, match=what):
            links.count_smu_pairs(data, mu_bins=bad)
    with pytest.raises(ValueError, match="separate Catalog"):
        yaw.autocorrelate_multipoles(config, data, data, mu_bins=4)
    rng = np.random.default_rng(3)
    bare = yaw.Catalog.from_arrays(rng.uniform(0.3, 0.305, 50), rng.uniform(0.1, 0.1005, 50),
                                   patch_centers=yaw.AngularCoordinates(np.array(NEIGHBOURS)), degrees=False)
    with pytest.raises(ValueError):  # catalogues without redshifts
        yaw.autocorrelate_multipoles(config, bare, random, mu_bins=4)
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        yaw.autocorrelate_multipoles(config, data, random, mu_bins=4)
    with pytest.raises(NotImplementedError):
        links.count_smu_pairs(data, mu_bins=4)


def test_the_lds_cap_refusal_becomes_a_value_error_and_the_squares_reach_the_library(monkeypatch):
    """The library's refusal, as the engine sees it, is translated; any other error of the library passes as it is; and what
    the library receives are the float64 products ``mu * mu``."""
    layout = object()
    monkeypatch.setattr(engine, "_proj_handles", lambda *args: (None, None, None))
    seen = []

    def refuse(message):
        def proj_count_smu(ctx, a, b, cells, s2, m2):
            seen.append(np.array(m2))
            raise _lib.YawhipError(f"yawhip_proj_count_smu failed (status 1): {message}")

        monkeypatch.setattr(_lib, "proj_count_smu", proj_count_smu)

    refuse("yawhip_proj_count_smu: 105 mu bins of 12 s bins do not fit the LDS of a workgroup: at most 104 mu bins at n_edges=13")
    with pytest.raises(ValueError, match=r"105 mu bins are too many for 13 s edges.*at most 104 mu bins"):
        engine.count_smu_fine(layout, layout, np.zeros((0, 4)), np.zeros((1, 13)), mu_edges=np.linspace(0.0, 1.0, 106), cosmology=None, unit="kpc")
    assert np.array_equal(seen[-1], np.linspace(0.0, 1.0, 106) * np.linspace(0.0, 1.0, 106))
    refuse("yawhip_proj_count_smu: the squared mu edges must be finite and strictly ascending (edge 1)")
    with pytest.raises(_lib.YawhipError, match="strictly ascending"):  # squares that no longer ascend: the library's refusal
        engine.count_smu_fine(layout, layout, np.zeros((0, 4)), np.zeros((1, 13)), mu_edges=np.array([0.0, 1e-200, 1.0]), cosmology=None, unit="kpc")
    assert seen[-1][1] == 0.0
