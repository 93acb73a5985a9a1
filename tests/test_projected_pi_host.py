"""CPU: the pi-binned projected clustering (``autocorrelate_projected(pi_bins=...)``, ``ProjectedCorrFunc``; DESIGN.md section
22) above the device seam -- the C ABI's new name, ``engine.check_pi_edges``, the oracle of tests/proj_pi_oracle.py against
the single-cylinder oracle and, pair by pair, against mpmath on the scene that the device tests use, the driver with
``engine.count_projected_pi_fine`` replaced by that oracle, and the error cases."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import proj_oracle
import proj_pi_oracle
import proj_scenes
import yet_another_wizz_amd as yaw
from conftest import ROOT
from helpers import use_oracle_engine
from proj_pi_oracle import UNEVEN, UNIFORM_4, UNIFORM_30
from test_dsigma_host import jackknife
from test_projected_host import NEIGHBOURS, driver_config, driver_scenario
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, engine, measurements

EPS = 2.0**-53
MARGIN = 1e-9
EDGE_SETS = {"uniform4": UNIFORM_4, "uniform30": UNIFORM_30, "uneven": UNEVEN}


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_projected_fine", proj_oracle.count_projected_fine)
    monkeypatch.setattr(engine, "count_projected_pi_fine", proj_pi_oracle.count_projected_pi_fine)
    use_oracle_engine(monkeypatch)


# --------------------------------------------------------------------------- 1. ABI
def test_the_new_symbol_is_declared_bound_and_built_at_abi_6():
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "yawhip_proj_count_pi"
    assert name in _lib.ABI_SYMBOLS
    prototype = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
    assert prototype, name
    arguments = [" ".join(arg.split()) for arg in prototype.group(1).split(",")]
    assert arguments == ["yawhip_ctx *ctx", "yawhip_shear_sources *a", "yawhip_shear_sources *b", "int32_t n_cells", "const int32_t *cells",
                         "int32_t n_rows", "int32_t n_edges", "const double *r2", "int32_t n_pi", "const double *pe", "double *fine_w",
                         "yawhip_stats *stats"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)
    bound = _lib.load_library().yawhip_proj_count_pi
    single = _lib.load_library().yawhip_proj_count
    # yawhip_proj_count argument for argument, (n_pi, pe) in the place of pmax
    assert bound.argtypes[:8] == single.argtypes[:8] and bound.argtypes[10:] == single.argtypes[9:]
    assert bound.argtypes[8] is ctypes.c_int32 and bound.argtypes[9] is single.argtypes[7] and bound.restype is ctypes.c_int
    assert callable(_lib.proj_count_pi) and callable(engine.count_projected_pi_fine)
    assert "ProjectedCorrFunc" in yaw.__all__ and yaw.ProjectedCorrFunc is yaw.corrfunc.ProjectedCorrFunc


# --------------------------------------------------------------------------- 2. the edges
def test_check_pi_edges_accepts_a_count_or_edges_and_refuses_the_rest():
    for n in (1, 4, np.int64(30)):
        edges = engine.check_pi_edges(n, 40.0)
        assert edges.dtype == np.float64 and np.array_equal(edges, np.linspace(0.0, 40.0, int(n) + 1))
    assert np.array_equal(engine.check_pi_edges(4, 40.0), UNIFORM_4)
    for given in (UNEVEN, list(UNEVEN), tuple(UNEVEN), [0, 40]):
        edges = engine.check_pi_edges(given, 40)
        assert edges.dtype == np.float64 and np.array_equal(edges, np.asarray(given, dtype=np.float64))
    given = UNEVEN.copy()
    engine.check_pi_edges(given, 40.0)[1] = 0.5
    assert given[1] == 0.7  # the caller's array is not what comes back
    for bad in (0, -3, True, [0.5, 40.0], [0.0, 39.0], [0.0, 41.0], [0.0, 10.0, 10.0, 40.0], [0.0, 20.0, 10.0, 40.0],
                [0.0, np.nan, 40.0], [0.0], [], [[0.0, 40.0]], "four", 2.5, None):
        with pytest.raises(ValueError):
            engine.check_pi_edges(bad, 40.0)
    with pytest.raises(ValueError, match="pi_max"):
        engine.check_pi_edges([0.0, np.inf], np.inf)
    with pytest.raises(ValueError, match="pi_max"):
        engine.check_pi_edges(4, 0.0)


# --------------------------------------------------------------------------- 3. the oracle against the single-cylinder oracle
SCENES = ((1, 96), (4, 24))


@functools.lru_cache(maxsize=None)
def scene(nb):
    per_segment = dict(SCENES)[nb]
    return proj_scenes.handle(proj_scenes.SEED_A, nb, per_segment), proj_scenes.handle(proj_scenes.SEED_B, nb, per_segment)


@pytest.mark.parametrize("nb", [1, 4])
def test_the_planes_sum_to_the_single_cylinder_oracle(nb):
    """``sum_j N[j]`` is the ``N`` of ``proj_cells`` at ``pmax = pe[-1]``, exactly; and on the shared scenes no pair lies within
    1e-9 (relative) of a pi edge and none has ``p == 0`` (the table of DESIGN.md section 22 has the figures)."""
    a, b = scene(nb)
    r2 = proj_scenes.radius_edges(12, nb)
    for first, second, cells in ((a, a, proj_scenes.cells_one_handle(nb)), (a, b, proj_scenes.cells_two_handles(nb))):
        for name, pe in EDGE_SETS.items():
            W, A, N = proj_pi_oracle.proj_pi_cells(first, second, cells, r2, pe)
            single = proj_oracle.proj_cells(first, second, cells, r2, float(pe[-1]))
            assert N.shape == (len(pe) - 1, len(cells), 12)
            assert np.array_equal(N.sum(axis=0), single[2])
            np.testing.assert_allclose(W.sum(axis=0), single[0], rtol=1e-13)
            margin, least = proj_pi_oracle.nearest_pi_margin(first, second, cells, pe)
            print(f"nb={nb} {'one handle' if first is second else 'two handles'} {name}: nearest margin {margin:.3e}, "
                  f"fewest pairs in a pi bin {int(N.sum(axis=(1, 2)).min())}, least p {least:.3e}")
            assert margin > MARGIN and least > 0.0 and N.sum(axis=(1, 2)).min() >= 200  # (every pi bin is well filled)
    # an infinite last edge: the last plane holds what lies beyond the edge before it
    open_ended = np.array([0.0, 10.0, np.inf])
    N = proj_pi_oracle.proj_pi_cells(a, a, proj_scenes.cells_one_handle(nb), r2, open_ended)[2]
    assert np.array_equal(N.sum(axis=0), proj_oracle.proj_cells(a, a, proj_scenes.cells_one_handle(nb), r2, np.inf)[2])
    assert np.array_equal(N[0], proj_oracle.proj_cells(a, a, proj_scenes.cells_one_handle(nb), r2, 10.0)[2])


# --------------------------------------------------------------------------- 4. the oracle's membership, exactly
def exact_pairs(a, b, cells, r2, same):
    """Every pair of the cells at 50 digits: ``(cell, fine bin or -1, p, w_a w_b)`` with ``theta = 2 asin(chord / 2)``,
    ``R^2 = ((d_a + d_b) / 2)^2 theta^2`` and ``p = |c_a - c_b|`` of the float64 inputs (the method of
    tests/test_projected_host.py), and the smallest relative distance of any ``R^2`` from an edge > 0 of its row."""
    import mpmath

    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    cols_a = {c: [mpf(float(v)) for v in a[c]] for c in "xyzdc"}
    cols_b = cols_a if same else {c: [mpf(float(v)) for v in b[c]] for c in "xyzdc"}
    wa = [mpf(1)] * len(a["x"]) if a["w"] is None else [mpf(float(v)) for v in a["w"]]
    wb = wa if same else ([mpf(1)] * len(b["x"]) if b["w"] is None else [mpf(float(v)) for v in b["w"]])
    nf = r2.shape[1] - 1
    pairs, margin_r = [], mpf(1)
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        edges = [mpf(float(v)) for v in r2[row]]
        for i in range(int(a["off"][sa]), int(a["off"][sa + 1])):
            ax, ay, az, ad, ac = (cols_a[c][i] for c in "xyzdc")
            for j in range(int(b["off"][sb]), int(b["off"][sb + 1])):
                if diagonal and j >= i:
                    break
                dx, dy, dz = ax - cols_b["x"][j], ay - cols_b["y"][j], az - cols_b["z"][j]
                theta = 2 * mpmath.asin(mpmath.sqrt(dx * dx + dy * dy + dz * dz) / 2)
                D = (ad + cols_b["d"][j]) / 2
                R2 = D * D * theta * theta
                below = 0
                for edge in edges:
                    if edge > 0:
                        margin_r = min(margin_r, abs(R2 / edge - 1))
                    below += edge < R2
                pairs.append((n, below - 1 if 0 < below <= nf else -1, abs(ac - cols_b["c"][j]), wa[i] * wb[j]))
    return pairs, float(margin_r)


def test_the_oracles_membership_in_pi_is_exact_on_the_device_scene():
    """For the scene of tests/test_gpu_projected_pi.py (four redshift bins, twelve fine bins, one handle and two) every pair is
    classified at 50 digits, in radius and in pi, for the three edge sets. No pair -- inside the radius range or not -- lies
    within 1e-9 (relative) of a pi edge, none within 1e-9 of a radius edge and none at ``p == 0``, so the comparison leaves out
    no pair, and the oracle's integer count per pi bin, cell and fine bin is the exact one. The oracle's weighted sums are then
    held against the exact sums: the worst ``|W - exact| / (eps A)`` is printed; four times it, rounded up to a power of two,
    is the ``K`` of the device tests."""
    import mpmath

    import test_gpu_projected_pi

    nb = 4
    a, b = scene(nb)
    r2 = proj_scenes.radius_edges(12, nb)
    worst = 0.0
    for first, second, cells in ((a, a, proj_scenes.cells_one_handle(nb)), (a, b, proj_scenes.cells_two_handles(nb))):
        same = first is second
        pairs, margin_r = exact_pairs(first, second, cells, r2, same)
        assert margin_r > MARGIN and min(p for _, _, p, _ in pairs) > 0
        for name, pe in EDGE_SETS.items():
            n_pi = len(pe) - 1
            edges = [mpmath.mpf(float(v)) for v in pe]
            margin_p = float(min(abs(p / edge - 1) for _, _, p, _ in pairs for edge in edges[1:]))
            margin_64 = proj_pi_oracle.nearest_pi_margin(first, second, cells, pe)[0]
            count = np.zeros((n_pi, len(cells), 12), dtype=np.int64)
            sums = {}
            for n, e, p, ww in pairs:
                plane = sum(edge < p for edge in edges[1:])
                if e >= 0 and plane < n_pi:
                    count[plane, n, e] += 1
                    sums[plane, n, e] = sums.get((plane, n, e), 0) + ww
            print(f"{'one handle' if same else 'two handles'} {name}: {count.sum()} member pairs of {len(pairs)}, nearest to a pi edge "
                  f"{margin_p:.3e} (float64: {margin_64:.3e}), fewest pairs in a pi bin {count.sum(axis=(1, 2)).min()}")
            assert margin_p > MARGIN and margin_64 > MARGIN
            W, A, N = proj_pi_oracle.proj_pi_cells(first, second, cells, r2, pe)
            assert count.sum() > 3000 and np.array_equal(N, count.astype(np.float64))
            unit = proj_pi_oracle.proj_pi_cells(proj_scenes.unweighted(first), proj_scenes.unweighted(second), cells, r2, pe, same=same)
            assert np.array_equal(unit[0], N)  # unit weights: W is the count
            for slot, exact in sums.items():
                worst = max(worst, float(abs(exact - float(W[slot]))) / (EPS * A[slot]))
    print(f"the oracle's worst |W - exact| / (eps A): {worst:.3f}")
    assert worst <= test_gpu_projected_pi.K_ORACLE_RATIO * 1.0000001  # the figure K was derived from still holds
    assert test_gpu_projected_pi.K == 2.0 ** np.ceil(np.log2(4.0 * test_gpu_projected_pi.K_ORACLE_RATIO))


# --------------------------------------------------------------------------- 5. the driver on the oracle stand-in
PI_MAX = 60.0
DRIVER_EDGES = np.array([0.0, 10.0, 25.0, 60.0])  # uneven widths; every pi bin holds pairs across the patch borders


def by_hand_pi(config, cat1, cat2, pi_edges):
    """``test_projected_host.by_hand`` per pi bin: the counts [n_pi, S, B, P, P] from the oracle's fine sums and the radial
    plan over all nine patch pairs (the upper triangle of an auto count), and their one normalisation [B, P, P]."""
    auto = cat2 is None
    plans = measurements.radial_plans(config)
    r2 = measurements.threshold_table(plans)
    unit = config.scales.scales.unit
    layouts = [cat.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True) for cat in ((cat1,) if auto else (cat1, cat2))]
    handles = [proj_oracle.as_handle(layout, *engine.proj_columns(layout, config.cosmology, unit)) for layout in layouts]
    jobs = [(p, q) for p in range(3) for q in range(p if auto else 0, 3)]
    cells = np.array([(p * 2 + k, q * 2 + k, k, auto and p == q) for p, q in jobs for k in range(2)])
    W, _, _ = proj_pi_oracle.proj_pi_cells(handles[0], handles[-1], cells, r2, pi_edges)
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


def check_pi_driver(unit, count_rr, pi_bins=DRIVER_EDGES, rtol=1e-12):
    """``autocorrelate_projected(pi_bins=...)`` against the oracle's fine sums recombined by hand: the counts of every pi bin,
    ``sample_xi()`` against Landy-Szalay (Davis-Peebles without RR) and ``sample()`` against ``2 sum dpi xi``, data and
    jackknife samples; ``engine.count_projected_pi_fine`` is whatever the caller left in place."""
    data, random = driver_scenario()
    config = driver_config(unit)
    pi_edges = engine.check_pi_edges(pi_bins, PI_MAX)
    n_pi = len(pi_edges) - 1
    result = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX, count_rr=count_rr, pi_bins=pi_bins)
    assert len(result) == 2
    hand = dict(dd=by_hand_pi(config, data, None, pi_edges), dr=by_hand_pi(config, data, random, pi_edges))
    if count_rr:
        hand["rr"] = by_hand_pi(config, random, None, pi_edges)
    for s, pcf in enumerate(result):
        assert type(pcf) is yaw.ProjectedCorrFunc and len(pcf.pi_bins) == n_pi == pcf.num_pi and np.array_equal(pcf.pi_edges, pi_edges)
        xi_data, xi_samples = [], []
        for j, cf in enumerate(pcf.pi_bins):
            assert type(cf) is yaw.CorrFunc and cf.rd is None and (cf.rr is not None) == count_rr
            assert cf.dd.auto and not cf.dr.auto
            ratio = {}
            for kind, (counts, norm) in hand.items():
                got = getattr(cf, kind)
                assert got.sum_weights is getattr(pcf.pi_bins[0], kind).sum_weights  # ONE normalisation for all planes
                assert np.count_nonzero(counts[j, s]) >= (2 * 4 if got.auto else 2 * 6)
                np.testing.assert_allclose(got.counts.counts, counts[j, s], rtol=rtol, atol=0, err_msg=f"{kind} pi bin {j}")
                (c_tot, c_jk), (n_tot, n_jk) = jackknife(counts[j, s]), jackknife(norm)
                ratio[kind] = (c_tot / n_tot, c_jk / n_jk)
            dd, dr = (np.array([ratio[kind][0], *ratio[kind][1]]) for kind in ("dd", "dr"))  # [1 + P, B]: data, then samples
            if count_rr:  # each ratio is held to rtol: the estimator moves by that of their magnitudes over RR
                rr = np.array([ratio["rr"][0], *ratio["rr"][1]])
                expected, bound = ((dd - dr) + (rr - dr)) / rr, 4.0 * rtol * (np.abs(dd) + 2.0 * np.abs(dr) + np.abs(rr)) / np.abs(rr)
            else:
                expected, bound = (dd - dr) / dr, 4.0 * rtol * np.abs(dd / dr)
            xi = pcf.sample_xi()[j]
            assert type(xi) is yaw.CorrData and xi.samples.shape == (3, 2) and np.all(np.isfinite(xi.data))
            assert np.all(np.abs(np.array([xi.data, *xi.samples]) - expected) <= bound)
            # ... and it is the bin's own CorrFunc.sample()
            assert np.array_equal(xi.data, cf.sample().data) and np.array_equal(xi.samples, cf.sample().samples)
            xi_data.append((expected, bound))
        wp = pcf.sample()
        assert type(wp) is yaw.CorrData and wp.samples.shape == (3, 2)
        dpi = np.diff(pi_edges)
        expected = 2.0 * sum(d * e for d, (e, _) in zip(dpi, xi_data))
        bound = 2.0 * sum(d * b for d, (_, b) in zip(dpi, xi_data)) + 8.0 * n_pi * EPS * 2.0 * sum(d * np.abs(e) for d, (e, _) in zip(dpi, xi_data))
        assert np.all(np.abs(np.array([wp.data, *wp.samples]) - expected) <= bound)
        # errors and covariance are those of the summed samples
        summed = yaw.CorrData(pcf.binning, wp.data, wp.samples)
        assert np.array_equal(wp.error, summed.error) and np.array_equal(wp.covariance, summed.covariance)
    return result


@pytest.mark.parametrize("count_rr", [True, False], ids=["LS", "DP"])
@pytest.mark.parametrize("unit", ["kpc", "Mpc/h"])
def test_the_pi_driver_on_the_oracle_stand_in(stand_in, unit, count_rr):
    check_pi_driver(unit, count_rr)


def test_an_int_gives_equal_bins_and_none_gives_todays_objects(stand_in):
    data, random = driver_scenario()
    config = driver_config("kpc")
    (first, _) = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX, pi_bins=3)
    assert np.array_equal(first.pi_edges, [0.0, 20.0, 40.0, 60.0]) and first.num_pi == 3
    plain = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX, pi_bins=None)
    default = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX)
    assert all(type(cf) is yaw.CorrFunc for cf in plain) and plain == default
    layout = data.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    links = yaw.PatchLinkage.from_catalogs(config, data, max_angle=measurements.radial_max_angle(config, layout))
    single = links.count_projected_pairs(data, pi_max=PI_MAX)
    assert all(type(nc) is yaw.NormalisedCounts for nc in single) and single == links.count_projected_pairs(data, pi_max=PI_MAX, pi_bins=None)
    binned = links.count_projected_pairs(data, pi_max=PI_MAX, pi_bins=3)
    assert len(binned) == 2 and all(len(per_pi) == 3 and all(type(nc) is yaw.NormalisedCounts for nc in per_pi) for per_pi in binned)
    assert len({id(nc.sum_weights) for per_pi in binned for nc in per_pi}) == 1  # all planes share the one PatchedSumWeights
    one_bin = links.count_projected_pairs(data, pi_max=PI_MAX, pi_bins=1)  # one pi bin is the cylinder
    for per_pi, nc in zip(one_bin, single):
        assert per_pi[0] == nc


def unit_scenario():
    """``driver_scenario`` without weights, and a configuration without ``rweight``: every count is an integer."""
    _, random = driver_scenario()
    rng = np.random.default_rng(29)
    ra, dec = (np.concatenate(c) for c in zip(*(ring_around(rng, ra_c, dec_c, 90, 1e-5, 1.8e-3) for ra_c, dec_c in NEIGHBOURS)))
    data = yaw.Catalog.from_arrays(ra, dec, redshifts=rng.uniform(0.22, 0.58, len(ra)), patch_centers=yaw.AngularCoordinates(np.array(NEIGHBOURS)),
                                   degrees=False)
    config = yaw.Configuration.create(rmin=[100.0, 300.0], rmax=[2000.0, 1000.0], unit="kpc", resolution=12, edges=driver_config("kpc").binning.edges)
    return config, data, random


def check_cylinder(config, data, random, exact):
    """``cylinder()`` against ``autocorrelate_projected(pi_bins=None)``: the same counts -- bit for bit where they are
    integers (``exact``), else to the 1e-12 of two orders of summation -- on an equal normalisation, and so the same
    single-cylinder estimate."""
    binned = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX, pi_bins=DRIVER_EDGES)
    plain = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX)
    for pcf, cf in zip(binned, plain):
        cyl = pcf.cylinder()
        assert type(cyl) is yaw.CorrFunc and cyl.to_dict().keys() == cf.to_dict().keys() and cyl.rr is not None
        for kind, counts in cf.to_dict().items():
            got = cyl.to_dict()[kind]
            assert got.sum_weights == counts.sum_weights and np.count_nonzero(counts.counts.counts) >= 2 * 4
            if exact:
                assert np.array_equal(got.counts.counts, counts.counts.counts), kind
            else:
                np.testing.assert_allclose(got.counts.counts, counts.counts.counts, rtol=1e-12, atol=0, err_msg=kind)
        if exact:
            assert cyl == cf and np.array_equal(cyl.sample().data, cf.sample().data)
        else:
            np.testing.assert_allclose(cyl.sample().data, cf.sample().data, rtol=1e-9, atol=1e-11)
    return binned


def test_the_cylinder_is_the_single_cylinder_measurement(stand_in):
    config, data, random = unit_scenario()
    check_cylinder(config, data, random, exact=True)  # unit weights, no rweight: integers
    data, random = driver_scenario()
    check_cylinder(driver_config("kpc"), data, random, exact=False)  # weighted data and rweight


def test_projected_corrfunc_round_trips_compares_and_subsets(stand_in):
    config, data, random = unit_scenario()
    (pcf, other) = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX, pi_bins=DRIVER_EDGES)
    state = pcf.to_dict()
    assert set(state) == {"pi_edges", "pi_bins"} and len(state["pi_bins"]) == 3 and set(state["pi_bins"][0]) == {"dd", "dr", "rr"}
    again = yaw.ProjectedCorrFunc.from_dict(state)
    assert again == pcf and again is not pcf and not (pcf == other) and pcf != other
    assert (pcf == pcf.pi_bins[0]) is False and pcf.is_compatible(other) and not pcf.is_compatible(pcf.pi_bins[0])
    moved = yaw.ProjectedCorrFunc(pcf.pi_edges * 2.0, pcf.pi_bins)
    assert moved != pcf and not pcf.is_compatible(moved) and np.array_equal(moved.sample().data, 2.0 * pcf.sample().data)
    with pytest.raises(ValueError):
        pcf.pi_edges[1] = 3.0  # the edges are read-only
    assert (pcf.num_bins, pcf.num_patches, pcf.auto, pcf.binning) == (2, 3, True, pcf.pi_bins[0].binning)
    one_bin = pcf.bins_subset(slice(1, 2))
    assert type(one_bin) is yaw.ProjectedCorrFunc and one_bin.num_bins == 1 and one_bin.num_pi == 3
    assert all(sub == cf.bins_subset(slice(1, 2)) for sub, cf in zip(one_bin.pi_bins, pcf.pi_bins))
    assert np.array_equal(one_bin.sample().data, pcf.sample().data[1:2])
    two_patches = pcf.patches_subset([0, 2])
    assert two_patches.num_patches == 2 and all(sub == cf.patches_subset([0, 2]) for sub, cf in zip(two_patches.pi_bins, pcf.pi_bins))
    assert two_patches.sample().samples.shape == (2, 2)
    # what the constructor refuses
    with pytest.raises(ValueError):
        yaw.ProjectedCorrFunc(pcf.pi_edges[:-1], pcf.pi_bins)
    with pytest.raises(ValueError):
        yaw.ProjectedCorrFunc([1.0, 2.0, 3.0, 4.0], pcf.pi_bins)
    with pytest.raises(ValueError):
        yaw.ProjectedCorrFunc([0.0, 2.0, 2.0, 4.0], pcf.pi_bins)
    with pytest.raises(TypeError):
        yaw.ProjectedCorrFunc([0.0, 1.0], [pcf.pi_bins[0].dd])
    with pytest.raises(ValueError):
        yaw.ProjectedCorrFunc([0.0, 1.0, 2.0], [pcf.pi_bins[0], yaw.CorrFunc(pcf.pi_bins[1].dd, pcf.pi_bins[1].dr)])
    with pytest.raises(ValueError):
        yaw.ProjectedCorrFunc([0.0, 1.0, 2.0], [pcf.pi_bins[0], one_bin.pi_bins[1]])


def test_a_pi_bin_with_empty_rr_gives_nan_there_and_in_the_sum(stand_in):
    """Nothing is masked: a pi bin narrower than any pair of the randoms has RR = 0 and ``xi = x / 0`` there; the sum carries
    it, as ``CorrFunc.sample()`` would."""
    config, data, random = unit_scenario()
    edges = np.array([0.0, 1e-7, 30.0, PI_MAX])
    with np.errstate(divide="ignore", invalid="ignore"):
        (pcf, _) = yaw.autocorrelate_projected(config, data, random, pi_max=PI_MAX, pi_bins=edges)
        assert pcf.pi_bins[0].rr.counts.counts.sum() == 0.0
        xi = pcf.sample_xi()
        assert not np.any(np.isfinite(xi[0].data)) and np.all(np.isfinite(xi[1].data)) and np.all(np.isfinite(xi[2].data))
        assert not np.any(np.isfinite(pcf.sample().data))
        assert np.all(np.isfinite(pcf.cylinder().sample().data))


# --------------------------------------------------------------------------- 6. error cases
def test_the_pi_drivers_reject_what_they_cannot_use(stand_in, monkeypatch):
    data, random = driver_scenario()
    config = driver_config("kpc")
    angular = yaw.Configuration.create(rmin=[1.0], rmax=[5.0], unit="arcmin", edges=config.binning.edges)
    with pytest.raises(ValueError, match="physical or comoving unit"):
        yaw.autocorrelate_projected(angular, data, random, pi_max=40.0, pi_bins=4)
    for bad, what in (([0.5, 40.0], "start at 0"), ([0.0, 20.0, 39.0], "end at pi_max"), ([0.0, 30.0, 20.0, 40.0], "ascend"),
                      ([0.0, 20.0, 20.0, 40.0], "ascend"), (0, ">= 1")):
        with pytest.raises(ValueError, match=what):
            yaw.autocorrelate_projected(config, data, random, pi_max=40.0, pi_bins=bad)
        links = yaw.PatchLinkage.from_catalogs(config, data, random)
        with pytest.raises(ValueError, match=what):
            links.count_projected_pairs(data, pi_max=40.0, pi_bins=bad)
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        yaw.autocorrelate_projected(config, data, random, pi_max=40.0, pi_bins=4)
    with pytest.raises(NotImplementedError):
        links.count_projected_pairs(data, pi_max=40.0, pi_bins=4)


def test_the_lds_cap_refusal_becomes_a_value_error_that_states_the_cap(monkeypatch):
    """The library's refusal, as the engine sees it, is translated; any other error of the library passes as it is."""
    layout = object()
    monkeypatch.setattr(engine, "_proj_handles", lambda *args: (None, None, None))

    def refuse(message):
        def proj_count_pi(*args):
            raise _lib.YawhipError(f"yawhip_proj_count_pi failed (status 1): {message}")

        monkeypatch.setattr(_lib, "proj_count_pi", proj_count_pi)

    refuse("yawhip_proj_count_pi: 105 pi bins of 12 radius bins do not fit the LDS of a workgroup: at most 104 pi bins at n_edges=13")
    with pytest.raises(ValueError, match=r"105 pi bins are too many for 13 radius edges.*at most 104 pi bins"):
        engine.count_projected_pi_fine(layout, layout, np.zeros((0, 4)), np.zeros((1, 13)), pi_edges=np.linspace(0.0, 40.0, 106),
                                       cosmology=None, unit="kpc")
    refuse("yawhip_proj_count_pi: the first pi edge must be 0")
    with pytest.raises(_lib.YawhipError, match="first pi edge"):
        engine.count_projected_pi_fine(layout, layout, np.zeros((0, 4)), np.zeros((1, 13)), pi_edges=np.array([1.0, 2.0]), cosmology=None, unit="kpc")
