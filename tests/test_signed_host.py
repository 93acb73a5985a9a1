"""CPU: the cross-correlations with a signed line of sight (``yawhip_proj_count_pi_signed``, ``yawhip_proj_count_smu_signed``;
DESIGN.md section 27) without a device -- the fold identities that tie the signed oracles (tests/proj_signed_oracle.py,
tests/smu_signed_oracle.py) to the exact reference of tests/golden/proj_exact.npz and to the unsigned oracle, the engine's
edge checks, the two result classes, and both drivers through the oracles' stand-ins against a patch-free brute force."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import proj_exact
import proj_oracle
import proj_signed_oracle as pso
import smu_oracle
import smu_scenes
import smu_signed_oracle as sso
import yet_another_wizz_amd as yaw
from conftest import ROOT
from helpers import use_oracle_engine
from proj_signed_oracle import fold, mirrored
from test_projected_host import NEIGHBOURS
from test_shear_host import ring_around
from test_smu_host import driver_config
from yet_another_wizz_amd import _lib, engine, measurements


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_projected_fine", proj_oracle.count_projected_fine)
    monkeypatch.setattr(engine, "count_projected_pi_signed_fine", pso.count_projected_pi_signed_fine)
    monkeypatch.setattr(engine, "count_smu_signed_fine", sso.count_smu_signed_fine)
    import proj_pi_oracle

    monkeypatch.setattr(engine, "count_projected_pi_fine", proj_pi_oracle.count_projected_pi_fine)
    monkeypatch.setattr(engine, "count_smu_fine", smu_oracle.count_smu_fine)
    use_oracle_engine(monkeypatch)


# --------------------------------------------------------------------------- 1. header and bindings
def test_the_two_symbols_are_declared_bound_and_built_at_abi_6():
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)
    for name, table, n, edges in (("yawhip_proj_count_pi_signed", "r2", "n_pi", "pe"), ("yawhip_proj_count_smu_signed", "s2", "n_mu", "sm2")):
        assert name in _lib.ABI_SYMBOLS
        prototype = re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S)
        assert prototype, name
        arguments = [" ".join(arg.split()) for arg in prototype.group(1).split(",")]
        assert arguments == ["yawhip_ctx *ctx", "yawhip_shear_sources *a", "yawhip_shear_sources *b", "int32_t n_cells", "const int32_t *cells",
                             "int32_t n_rows", "int32_t n_edges", f"const double *{table}", f"int32_t {n}", f"const double *{edges}",
                             "double *fine_w", "yawhip_stats *stats"]
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        bound = getattr(_lib.load_library(), name)
        assert bound.argtypes == _lib.load_library().yawhip_proj_count_pi.argtypes and bound.restype is ctypes.c_int
    assert callable(_lib.proj_count_pi_signed) and callable(_lib.proj_count_smu_signed)
    assert callable(engine.count_projected_pi_signed_fine) and callable(engine.count_smu_signed_fine)
    for exported in ("SignedProjectedCorrFunc", "SignedMultipoleCorrFunc", "crosscorrelate_projected", "crosscorrelate_multipoles"):
        assert exported in yaw.__all__ and getattr(yaw, exported) is not None


# --------------------------------------------------------------------------- 2. the fold identities on the oracles
@pytest.mark.parametrize("fold_bins", [False, True], ids=["nb=2", "nb=1"])
@pytest.mark.parametrize("name", proj_exact.SCENES)
def test_the_signed_pi_planes_fold_to_the_exact_integers(name, fold_bins):
    """On the exact fixture, two handles: over each stored pi set mirrored, no pair has ``ps == 0`` or lies on an edge, every
    live cell holds different totals on the two sides (a swapped sign is visible in each), and the signed unit-weight planes
    fold to the stored ``N_pi`` as integers."""
    fx = proj_exact.fixture()
    a, b = (proj_exact.scene(fx, name, cat, fold_bins, False) for cat in "ab")
    cells, r2 = proj_exact.cells(fx, name, fold_bins, True), fx[f"{name}.r2"]
    for edges in proj_exact.PI_SETS:
        pe = mirrored(fx[f"pi.{edges}"])
        margin, least = pso.nearest_signed_pi_margin(a, b, cells, pe)
        assert margin > 0.0 and least > 0.0, (edges, margin, least)
        W, _, N = pso.proj_pi_signed_cells(a, b, cells, r2, pe)
        n = len(pe) // 2
        negative, positive = N[:n].sum(axis=(0, 2)), N[n:].sum(axis=(0, 2))
        live = (negative + positive) > 0
        assert live.sum() >= 8 and np.all(negative[live] != positive[live]), (edges, negative, positive)
        assert np.array_equal(W, N)
        assert np.array_equal(fold(N), proj_exact.counts_pi(fx, name, fold_bins, True, edges)), edges
    print(f"{name} nb={1 if fold_bins else 2}: {int(negative.sum())} negative / {int(positive.sum())} positive member pairs, "
          f"{int(np.sum(negative[live] != positive[live]))} of {int(live.sum())} live cells asymmetric")


@pytest.mark.parametrize("nb", [1, 2])
def test_the_signed_mu_planes_fold_to_the_unsigned_oracle(nb):
    """The same on the scene of the redshift-space tests: no pair at ``ps == 0``, no product ``fl(sm2[k] S2)`` on ``sP2``, every
    live cell asymmetric, and the signed predicate folds to ``smu_oracle.smu_cells`` exactly."""
    a, b = smu_scenes.scene(nb, False)
    cells, s2 = smu_scenes.cells_two_handles(nb), smu_scenes.s_edges(6, nb)
    for name, mu in smu_scenes.MU_SETS.items():
        sm2 = sso.signed_squares(mirrored(mu))
        assert np.array_equal(sm2[len(mu) - 1:], smu_scenes.squares(mu)) and np.array_equal(sm2, -sm2[::-1])
        margin, least = sso.nearest_signed_mu_margin(a, b, cells, sm2)
        assert margin > 0.0 and least > 0.0, (name, margin, least)
        W, _, N = sso.smu_signed_cells(a, b, cells, s2, sm2)
        n = len(sm2) // 2
        negative, positive = N[:n].sum(axis=(0, 2)), N[n:].sum(axis=(0, 2))
        live = (negative + positive) > 0
        assert live.sum() >= 16 and np.all(negative[live] != positive[live]), (name, negative, positive)
        assert np.array_equal(W, N)
        assert np.array_equal(fold(N), smu_oracle.smu_cells(a, b, cells, s2, smu_scenes.squares(mu))[2]), name
    print(f"nb={nb}: {int(negative.sum())} negative / {int(positive.sum())} positive member pairs, {int(live.sum())} live cells")


def test_the_planes_of_the_signed_oracles_by_hand():
    """The two plane rules on numbers written out: the closed first bin, half-open bins after it, the two cuts, an edge at 0."""
    pe = np.array([-3.0, -1.0, 0.0, 2.0])
    assert pso.signed_pi_bin(np.array([-3.0, -2.0, -1.0, -0.5, 0.0, 1e-300, 2.0]), pe).tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert pso.signed_pi_bin(np.array([-3.0000001, 2.0000001, np.inf, -np.inf]), pe).tolist() == [3, 3, 3, 3]
    assert pso.signed_pi_bin(np.array([4.9, 5.0, 20.0, 20.1, -7.0]), np.array([5.0, 20.0])).tolist() == [1, 0, 0, 1, 1]  # one-sided, one bin
    sm2 = sso.signed_squares([-1.0, -0.5, 0.0, 0.5, 1.0])
    assert sm2.tolist() == [-1.0, -0.25, 0.0, 0.25, 1.0]
    S2 = np.full(6, 4.0)  # mu = ps / 2: -0.9, -0.5 (on the edge: the lower bin), -0.1, 0 (the bin below the edge at 0), 0.4, 1
    ps = np.array([-1.8, -1.0, -0.2, 0.0, 0.8, 2.0])
    assert sso.signed_mu_plane(S2, np.copysign(ps * ps, ps), sm2).tolist() == [0, 0, 1, 1, 2, 3]


# --------------------------------------------------------------------------- 3. the engine's edge checks
def test_check_signed_pi_edges_accepts_a_count_or_edges_and_refuses_the_rest():
    for n in (1, 4, 6, np.int64(7), 30):  # linspace to the ulp, and exactly antisymmetric: an even n folds
        got = engine.check_signed_pi_edges(n, 40.0)
        np.testing.assert_allclose(got, np.linspace(-40.0, 40.0, int(n) + 1), rtol=3e-16, atol=1e-14)
        assert np.array_equal(got, -got[::-1]) and got[0] == -40.0 and got[-1] == 40.0 and np.all(np.diff(got) > 0.0)
        assert n % 2 or got[int(n) // 2] == 0.0
    assert np.array_equal(engine.check_signed_pi_edges(4, 40.0), np.linspace(-40.0, 40.0, 5))
    uneven = [-40.0, -3.0, 1.0, 2.5, 40.0]  # not symmetric inside, no edge at 0
    got = engine.check_signed_pi_edges(uneven, 40.0)
    assert got.dtype == np.float64 and got.tolist() == uneven
    for bad, words in ((0, ">= 1"), (-2, ">= 1"), (True, "number of bins"), ("four", "number of bins"), (None, "at least two"),
                       ([40.0], "at least two"), ([[-40.0, 40.0]], "at least two"), ([-40.0, np.nan, 40.0], "finite"),
                       ([-40.0, np.inf], "finite"), ([0.0, 20.0, 40.0], "start at -pi_max"), ([-39.0, 40.0], "start at -pi_max"),
                       ([-40.0, 5.0, 5.0, 40.0], "ascend strictly"), ([-40.0, 10.0, 5.0, 40.0], "ascend strictly"),
                       ([-40.0, 0.0, 41.0], "end at pi_max")):
        with pytest.raises(ValueError, match=words):
            engine.check_signed_pi_edges(bad, 40.0)
    for pi_max in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="pi_max"):
            engine.check_signed_pi_edges(4, pi_max)


def test_check_signed_mu_edges_accepts_a_count_or_edges_and_refuses_the_rest():
    for n in (1, 5, 6, np.int64(30)):
        got = engine.check_signed_mu_edges(n)
        np.testing.assert_allclose(got, np.linspace(-1.0, 1.0, int(n) + 1), rtol=3e-16, atol=3e-16)
        assert np.array_equal(got, -got[::-1]) and got[0] == -1.0 and got[-1] == 1.0 and (n % 2 or got[int(n) // 2] == 0.0)
    assert engine.check_signed_mu_edges([-1, -0.4, 0.1, 0.25, 1]).tolist() == [-1.0, -0.4, 0.1, 0.25, 1.0]
    for bad, words in ((0, ">= 1"), (False, "number of bins"), ("x", "number of bins"), ([1.0], "at least two"),
                       ([-1.0, np.nan, 1.0], "finite"), ([0.0, 0.5, 1.0], "start at -1"), ([-1.0, 0.5, 0.5, 1.0], "ascend strictly"),
                       ([-1.0, 0.0, 0.9], "end at 1")):
        with pytest.raises(ValueError, match=words):
            engine.check_signed_mu_edges(bad)


# --------------------------------------------------------------------------- 4. the drivers on the stand-ins
PI_MAX = 2.5
HALF_PI, HALF_MU = np.array([0.0, 0.9, PI_MAX]), np.array([0.0, 0.2, 0.65, 1.0])  # uneven widths: what signed=False bins by
DRIVER_PI, DRIVER_MU = mirrored(HALF_PI), mirrored(HALF_MU)  # ... and their mirrored sets, 4 and 6 signed bins


@functools.lru_cache(maxsize=None)
def scenario_columns():
    """Two different unit-weight samples (80 and 70 objects around each of the three neighbouring patch centres) and their
    randoms (130 and 120): the redshifts in the two thin shells of tests/test_smu_host.py, 3 Mpc deep against scales of up
    to 2 Mpc, the second sample shifted behind the first by a third of that so that the two signs hold different counts."""
    rng = np.random.default_rng(53)
    out = []
    for n, shift in ((80, 0.0), (70, 0.00012), (130, 0.0), (120, 0.00012)):
        ra, dec = (np.concatenate(c) for c in zip(*(ring_around(rng, ra_c, dec_c, n, 1e-5, 1.8e-3) for ra_c, dec_c in NEIGHBOURS)))
        out.append((ra, dec, rng.choice([0.3, 0.5], len(ra)) + rng.uniform(-0.0004, 0.0004, len(ra)) + shift))
    return out


def driver_scenario():
    """``(config, data1, data2, rand1, rand2)``: fresh catalogues of ``scenario_columns`` and a configuration without
    ``rweight``, so that every count is an integer."""
    kw = dict(patch_centers=yaw.AngularCoordinates(np.array(NEIGHBOURS)), degrees=False)
    return (driver_config("kpc", rweight=None), *(yaw.Catalog.from_arrays(ra, dec, redshifts=z, **kw) for ra, dec, z in scenario_columns()))


def patch_free(config, cat1, cat2, count_cells, edges):
    """The counts [n, S, B] of two catalogues without patches: per redshift bin ALL objects of the first against ALL of the
    second in one cell of the oracle ``count_cells(a, b, cells, table, edges)``, the fine bins summed per scale by the radial
    plan."""
    plans = measurements.radial_plans(config)
    table = measurements.threshold_table(plans)
    unit = config.scales.scales.unit
    handles = []
    for cat in (cat1, cat2):
        layout = cat.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
        h = proj_oracle.as_handle(layout, *engine.proj_columns(layout, config.cosmology, unit))
        nb, off = layout.num_bins, np.asarray(layout.offsets)
        order = [np.concatenate([np.arange(off[p * nb + k], off[p * nb + k + 1]) for p in range(layout.num_patches)]) for k in range(nb)]
        flat = {c: np.concatenate([h[c][idx] for idx in order]) for c in "xyzdc"}
        assert h["w"] is None
        handles.append(dict(flat, w=None, nb=nb, off=np.concatenate([[0], np.cumsum([len(idx) for idx in order])]).astype(np.int64)))
    nb = handles[0]["nb"]
    cells = np.array([(k, k, k, 0) for k in range(nb)], dtype=np.int32)
    N = count_cells(handles[0], handles[1], cells, table, edges)[2]  # [n, B, nf]
    return np.array([measurements.CombinePlan(plans)(np.moveaxis(plane[None], 0, -1))[:, :, 0] for plane in N])  # [n, S, B]


def check_counts(results, bins_of, hand, kinds):
    """Every count of ``results`` (one per scale) summed over the patch pairs equals the patch-free ``hand[kind]`` [n, S, B]
    as integers, and only ``kinds`` are present."""
    for s, result in enumerate(results):
        for j, cf in enumerate(bins_of(result)):
            assert type(cf) is yaw.CorrFunc and set(cf.to_dict()) == set(kinds)
            for kind in kinds:
                got = getattr(cf, kind)
                assert not got.auto
                total = got.counts.counts.sum(axis=(1, 2))
                assert np.array_equal(total, hand[kind][j, s]), (kind, s, j, total, hand[kind][j, s])


def sides(data1, data2, rand1, rand2):
    """Which catalogues ``crosscorrelate`` pairs in each slot of ``CorrFunc(dd, dr, rd, rr)``."""
    return dict(dd=(data1, data2), dr=(data1, rand2), rd=(rand1, data2), rr=(rand1, rand2))


def test_the_projected_driver_counts_the_patch_free_pairs_and_folds(stand_in):
    config, data1, data2, rand1, rand2 = driver_scenario()
    pe = engine.check_signed_pi_edges(DRIVER_PI, PI_MAX)
    signed = yaw.crosscorrelate_projected(config, data1, data2, rand1, rand2, pi_max=PI_MAX, pi_bins=DRIVER_PI, signed=True)
    assert len(signed) == 2 and all(type(r) is yaw.SignedProjectedCorrFunc and np.array_equal(r.pi_edges, pe) for r in signed)
    pairs = sides(data1, data2, rand1, rand2)
    hand = {kind: patch_free(config, *cats, pso.proj_pi_signed_cells, pe) for kind, cats in pairs.items()}
    for kind, counts in hand.items():
        assert counts.sum() > 500 and np.all(counts.sum(axis=(1, 2)) > 0)
        assert not np.array_equal(counts[:2].sum(axis=0), counts[2:][::-1].sum(axis=0)), kind  # the two signs differ
    check_counts(signed, lambda r: r.pi_bins, hand, ("dd", "dr", "rd", "rr"))
    # the slots are crosscorrelate's: dr is D1 R2, rd is R1 D2 -- told apart by the normalisation of each
    for kind, (first, second) in pairs.items():
        weights = getattr(signed[0].pi_bins[0], kind).sum_weights
        assert np.array_equal(weights.sum_weights1.sum(axis=1), objects_per_bin(first)), kind
        assert np.array_equal(weights.sum_weights2.sum(axis=1), objects_per_bin(second)), kind
    assert len({tuple(objects_per_bin(cat)) for cat in (data1, data2, rand1, rand2)}) == 4  # (which tells the four apart)
    assert signed[0].pi_bins[0].get_estimator().name == "LS"
    # signed=False is the fold of signed=True, as integers: no pair at ps == 0 or on an edge
    for cat in (data1, data2, rand1, rand2):
        cat.drop_layouts()
    unsigned = yaw.crosscorrelate_projected(config, data1, data2, rand1, rand2, pi_max=PI_MAX, pi_bins=HALF_PI)
    assert all(type(r) is yaw.ProjectedCorrFunc for r in unsigned)
    for folded, plain in zip((r.folded() for r in signed), unsigned):
        assert type(folded) is yaw.ProjectedCorrFunc and np.array_equal(folded.pi_edges, plain.pi_edges)
        for got, exp in zip(folded.pi_bins, plain.pi_bins):
            assert set(got.to_dict()) == set(exp.to_dict()) == {"dd", "dr", "rd", "rr"}
            for kind in ("dd", "dr", "rd", "rr"):
                assert np.array_equal(getattr(got, kind).counts.counts, getattr(exp, kind).counts.counts), kind
                assert getattr(exp, kind).counts.counts.sum() > 0
    # the single cylinder, and fewer randoms
    cylinder = yaw.crosscorrelate_projected(config, data1, data2, rand2=rand2, pi_max=PI_MAX)
    for cf, plain in zip(cylinder, unsigned):
        assert type(cf) is yaw.CorrFunc and set(cf.to_dict()) == {"dd", "dr"} and cf.get_estimator().name == "DP"
        assert np.array_equal(cf.dd.counts.counts, plain.cylinder().dd.counts.counts)
    only_rd = yaw.crosscorrelate_projected(config, data1, data2, rand1, pi_max=PI_MAX, pi_bins=DRIVER_PI, signed=True)
    check_counts(only_rd, lambda r: r.pi_bins, hand, ("dd", "rd"))
    no_rr = yaw.crosscorrelate_projected(config, data1, data2, rand1, rand2, pi_max=PI_MAX, pi_bins=DRIVER_PI, signed=True, count_rr=False)
    check_counts(no_rr, lambda r: r.pi_bins, hand, ("dd", "dr", "rd"))


def objects_per_bin(catalog):
    """The objects of one of ``driver_scenario``'s catalogues (told by its size) in the two redshift bins of the configuration."""
    (z,) = [z for _, _, z in scenario_columns() if len(z) == sum(catalog.get_num_records())]
    return [np.count_nonzero((z > 0.2) & (z <= 0.4)), np.count_nonzero((z > 0.4) & (z <= 0.6))]


def test_the_multipole_driver_counts_the_patch_free_pairs_and_folds(stand_in):
    config, data1, data2, rand1, rand2 = driver_scenario()
    mu = engine.check_signed_mu_edges(DRIVER_MU)
    signed = yaw.crosscorrelate_multipoles(config, data1, data2, rand1, rand2, mu_bins=DRIVER_MU, signed=True)
    assert len(signed) == 2 and all(type(r) is yaw.SignedMultipoleCorrFunc and np.array_equal(r.mu_edges, mu) for r in signed)
    hand = {kind: patch_free(config, *cats, sso.smu_signed_cells, sso.signed_squares(mu)) for kind, cats in sides(data1, data2, rand1, rand2).items()}
    for kind, counts in hand.items():
        assert counts.sum() > 500 and np.all(counts.sum(axis=(1, 2)) > 0)
        assert not np.array_equal(counts[:3].sum(axis=0), counts[3:][::-1].sum(axis=0)), kind
    check_counts(signed, lambda r: r.mu_bins, hand, ("dd", "dr", "rd", "rr"))
    for cat in (data1, data2, rand1, rand2):
        cat.drop_layouts()
    unsigned = yaw.crosscorrelate_multipoles(config, data1, data2, rand1, rand2, mu_bins=HALF_MU)
    for folded, plain in zip((r.folded() for r in signed), unsigned):
        assert type(folded) is type(plain) is yaw.MultipoleCorrFunc and np.array_equal(folded.mu_edges, plain.mu_edges)
        for got, exp in zip(folded.mu_bins, plain.mu_bins):
            for kind in ("dd", "dr", "rd", "rr"):
                assert np.array_equal(getattr(got, kind).counts.counts, getattr(exp, kind).counts.counts), kind
    # the multipoles of the measured counts: finite, the odd ones there, and (2 ell + 1) / 2 sum_j xi_j I_ell,j by hand
    first = signed[0]
    multipoles = first.sample_multipoles()
    assert len(multipoles) == 5 and all(type(m) is yaw.CorrData and m.samples.shape == (3, 2) and np.all(np.isfinite(m.data)) for m in multipoles)
    xi = first.sample_xi()
    for ell, got in zip(range(5), multipoles):
        by_hand = (2 * ell + 1) / 2.0 * sum(w * x.data for w, x in zip(np.diff(legendre_primitive(ell, mu)), xi))
        np.testing.assert_allclose(got.data, by_hand, rtol=1e-12, atol=1e-14)


def test_the_drivers_and_the_linkage_reject_what_they_cannot_use(stand_in):
    config, data1, data2, rand1, rand2 = driver_scenario()
    with pytest.raises(ValueError, match="at least one random"):
        yaw.crosscorrelate_projected(config, data1, data2, pi_max=PI_MAX, pi_bins=4, signed=True)
    with pytest.raises(ValueError, match="at least one random"):
        yaw.crosscorrelate_multipoles(config, data1, data2, mu_bins=4, signed=True)
    with pytest.raises(ValueError, match="needs pi_bins"):
        yaw.crosscorrelate_projected(config, data1, data2, rand1, pi_max=PI_MAX, signed=True)
    with pytest.raises(ValueError, match="start at -pi_max"):
        yaw.crosscorrelate_projected(config, data1, data2, rand1, pi_max=PI_MAX, pi_bins=[0.0, PI_MAX], signed=True)
    with pytest.raises(ValueError, match="start at 0"):
        yaw.crosscorrelate_projected(config, data1, data2, rand1, pi_max=PI_MAX, pi_bins=[-PI_MAX, PI_MAX])
    with pytest.raises(ValueError, match="start at -1"):
        yaw.crosscorrelate_multipoles(config, data1, data2, rand1, mu_bins=[0.0, 1.0], signed=True)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_projected(config, data1, data1, rand1, pi_max=PI_MAX, pi_bins=4, signed=True)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_multipoles(config, data1, data2, rand1, rand1, mu_bins=4)
    angular = yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", edges=config.binning.edges)
    with pytest.raises(ValueError):
        yaw.crosscorrelate_multipoles(angular, data1, data2, rand1, mu_bins=4, signed=True)
    layouts = [cat.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True) for cat in (data1, data2)]
    links = yaw.PatchLinkage.from_catalogs(config, data1, data2, max_angle=measurements.radial_max_angle(config, *layouts))
    with pytest.raises(ValueError, match="needs a second catalogue and pi_bins"):
        links.count_projected_pairs(data1, pi_max=PI_MAX, pi_bins=4, signed=True)
    with pytest.raises(ValueError, match="needs a second catalogue and pi_bins"):
        links.count_projected_pairs(data1, data2, pi_max=PI_MAX, signed=True)
    with pytest.raises(ValueError, match="needs a second catalogue"):
        links.count_smu_pairs(data1, mu_bins=4, signed=True)
    counted = links.count_projected_pairs(data1, data2, pi_max=PI_MAX, pi_bins=4, signed=True)
    assert len(counted) == 2 and all(len(per_pi) == 4 and all(type(nc) is yaw.NormalisedCounts for nc in per_pi) for per_pi in counted)
    assert len({id(nc.sum_weights) for per_pi in counted for nc in per_pi}) == 1


def test_the_refusals_of_the_library_become_value_errors(monkeypatch):
    """The cap refusal of either signed call reaches the user as the ``ValueError`` of the siblings, and the multipole seam
    hands the library the signed squares."""
    seen = {}

    def refuse(symbol, bins, rows):
        def call(ctx, a, b, cells, table, edges):
            seen[symbol] = np.array(edges)
            raise _lib.YawhipError(f"{symbol} failed (-1): {symbol}: {len(edges) - 1} {bins} bins of 12 {rows} bins do not fit the LDS of a "
                                   f"workgroup: at most 104 {bins} bins at n_edges=13")
        return call

    monkeypatch.setattr(engine, "_proj_handles", lambda *args: (None, None, None))
    monkeypatch.setattr(_lib, "proj_count_pi_signed", refuse("yawhip_proj_count_pi_signed", "pi", "radius"))
    monkeypatch.setattr(_lib, "proj_count_smu_signed", refuse("yawhip_proj_count_smu_signed", "mu", "s"))
    table = np.ones((1, 13))
    with pytest.raises(ValueError, match="105 pi bins are too many for 13 radius edges.*at most 104 pi bins"):
        engine.count_projected_pi_signed_fine(None, None, None, table, pi_edges=np.linspace(-1.0, 1.0, 106), cosmology=None, unit="kpc")
    mu = np.linspace(-1.0, 1.0, 106)
    with pytest.raises(ValueError, match="105 mu bins are too many for 13 s edges.*at most 104 mu bins"):
        engine.count_smu_signed_fine(None, None, None, table, mu_edges=mu, cosmology=None, unit="kpc")
    assert np.array_equal(seen["yawhip_proj_count_smu_signed"], np.copysign(mu * mu, mu))


# --------------------------------------------------------------------------- 5. the two result classes
def legendre_primitive(ell, x):
    """The antiderivative of ``P_ell`` written out, ``ell`` = 0 ... 4."""
    x = np.asarray(x, dtype=np.float64)
    return {0: x, 1: 0.5 * x**2, 2: 0.5 * (x**3 - x), 3: (5.0 * x**4 - 6.0 * x**2) / 8.0, 4: (7.0 * x**5 - 10.0 * x**3 + 3.0 * x) / 8.0}[ell]


@pytest.fixture
def measured(stand_in):
    config, data1, data2, rand1, rand2 = driver_scenario()
    (pcf, p_other) = yaw.crosscorrelate_projected(config, data1, data2, rand1, rand2, pi_max=PI_MAX, pi_bins=DRIVER_PI, signed=True)
    (mcf, m_other) = yaw.crosscorrelate_multipoles(config, data1, data2, rand1, rand2, mu_bins=DRIVER_MU, signed=True)
    return pcf, p_other, mcf, m_other


def test_the_signed_classes_round_trip_compare_and_subset(measured):
    pcf, p_other, mcf, m_other = measured
    for cf, other, cls, name, bins in ((pcf, p_other, yaw.SignedProjectedCorrFunc, "pi", 4), (mcf, m_other, yaw.SignedMultipoleCorrFunc, "mu", 6)):
        edges, planes = getattr(cf, f"{name}_edges"), getattr(cf, f"{name}_bins")
        assert type(cf) is cls and len(planes) == bins == getattr(cf, f"num_{name}") and name in repr(cf)
        state = cf.to_dict()
        assert set(state) == {f"{name}_edges", f"{name}_bins"} and len(state[f"{name}_bins"]) == bins
        assert set(state[f"{name}_bins"][0]) == {"dd", "dr", "rd", "rr"}
        again = cls.from_dict(state)
        assert again == cf and again is not cf and cf != other and (cf == planes[0]) is False
        assert cf.is_compatible(other) and not cf.is_compatible(planes[0]) and not cf.is_compatible(pcf if cf is mcf else mcf)
        inner = np.array(edges)
        inner[1] = 0.5 * (inner[0] + inner[2]) + 0.01 * (inner[2] - inner[0])
        moved = cls(inner, planes)  # not symmetric inside: legal
        assert moved != cf and not cf.is_compatible(moved)
        with pytest.raises(ValueError, match=f"{name} edges differ"):
            cf.is_compatible(moved, require=True)
        with pytest.raises(TypeError):
            cf.is_compatible(planes[0], require=True)
        with pytest.raises(ValueError):
            edges[1] = 0.0  # the edges are read-only
        assert (cf.num_bins, cf.num_patches, cf.auto, cf.binning) == (2, 3, False, planes[0].binning)
        one_bin = cf.bins_subset(slice(1, 2))
        assert type(one_bin) is cls and one_bin.num_bins == 1 and len(getattr(one_bin, f"{name}_bins")) == bins
        assert all(sub == plane.bins_subset(slice(1, 2)) for sub, plane in zip(getattr(one_bin, f"{name}_bins"), planes))
        assert np.array_equal(one_bin.sample().data, cf.sample().data[1:2])
        two_patches = cf.patches_subset([0, 2])
        assert two_patches.num_patches == 2 and two_patches.sample().samples.shape == (2, 2)
        assert all(sub == plane.patches_subset([0, 2]) for sub, plane in zip(getattr(two_patches, f"{name}_bins"), planes))
        # what the constructor refuses
        with pytest.raises(ValueError, match="one edge more"):
            cls(edges[:-1], planes)
        top = edges[-1]
        for bad in ([-top, 0.0, 0.0, 0.5 * top, top][:bins + 1] if bins == 4 else None, np.where(np.arange(bins + 1) == 1, np.nan, edges),
                    np.concatenate([[-0.5 * top], edges[1:]]), edges[::-1]):
            if bad is not None:
                with pytest.raises(ValueError, match="finite, ascend strictly and span zero symmetrically"):
                    cls(bad, planes)
        with pytest.raises(TypeError):
            cls(edges, [plane.dd for plane in planes])
        with pytest.raises(ValueError):
            cls(edges, [yaw.CorrFunc(planes[0].dd, planes[0].dr), *planes[1:]])
        with pytest.raises(ValueError):
            cls(edges, [getattr(one_bin, f"{name}_bins")[0], *planes[1:]])
    with pytest.raises(ValueError, match="start at -1 and end at 1"):
        yaw.SignedMultipoleCorrFunc(2.0 * mcf.mu_edges, mcf.mu_bins)


def test_w_p_sums_the_signed_bins_without_a_factor_two(measured):
    pcf = measured[0]
    xi = pcf.sample_xi()
    assert len(xi) == 4 and all(np.array_equal(x.data, cf.sample().data) for x, cf in zip(xi, pcf.pi_bins))
    w_p = pcf.sample()
    by_hand = sum(d * x.data for d, x in zip(np.diff(pcf.pi_edges), xi))
    assert type(w_p) is yaw.CorrData and np.all(np.isfinite(w_p.data))
    np.testing.assert_allclose(w_p.data, by_hand, rtol=1e-14)
    np.testing.assert_allclose(w_p.samples, sum(d * x.samples for d, x in zip(np.diff(pcf.pi_edges), xi)), rtol=1e-14)
    # all bins holding ONE xi: w_p = 2 pi_max xi, what the folded class gives with its factor 2 over half the range
    same = yaw.SignedProjectedCorrFunc(pcf.pi_edges, [pcf.pi_bins[0]] * 4)
    np.testing.assert_allclose(same.sample().data, 2.0 * PI_MAX * xi[0].data, rtol=1e-14)  # (any widths)
    np.testing.assert_allclose(same.sample().data, yaw.ProjectedCorrFunc(pcf.pi_edges[2:], [pcf.pi_bins[0]] * 2).sample().data, rtol=1e-14)


def test_folded_sums_the_mirrored_bins_and_refuses_what_has_no_mirror(measured):
    pcf, _, mcf, _ = measured
    for cf, name, cls in ((pcf, "pi", yaw.ProjectedCorrFunc), (mcf, "mu", yaw.MultipoleCorrFunc)):
        edges, planes = getattr(cf, f"{name}_edges"), getattr(cf, f"{name}_bins")
        m = len(planes) // 2
        folded = cf.folded()
        assert type(folded) is cls and np.array_equal(getattr(folded, f"{name}_edges"), edges[m:])
        for j, got in enumerate(getattr(folded, f"{name}_bins")):
            for kind in ("dd", "dr", "rd", "rr"):
                by_hand = getattr(planes[m + j], kind).counts.counts + getattr(planes[m - 1 - j], kind).counts.counts
                assert np.array_equal(getattr(got, kind).counts.counts, by_hand) and by_hand.sum() > 0
                assert getattr(got, kind).sum_weights is getattr(planes[m + j], kind).sum_weights
        odd = type(cf)(np.linspace(edges[0], edges[-1], len(planes)), planes[:-1])  # an odd number of bins: 0 is no edge
        skewed = np.array(edges)
        skewed[1] *= 0.9  # 0 is an edge, the inside not symmetric
        for bad in (odd, type(cf)(skewed, planes)):
            with pytest.raises(ValueError, match=f"symmetric about 0"):
                bad.folded()


def scaled(cf, factor):
    """``cf`` with DD scaled so that its Davis-Peebles ``xi`` is ``factor - 1`` everywhere: ``CorrFunc(factor * rd, rd=rd)``."""
    rd = cf.rd
    return yaw.CorrFunc(yaw.NormalisedCounts(rd.counts * factor, rd.sum_weights), rd=rd)


def test_the_legendre_weights_and_the_parity_of_the_multipoles(measured):
    mcf = measured[2]
    for edges in (mcf.mu_edges, np.array([-1.0, -0.4, 0.1, 0.25, 1.0])):
        cf = yaw.SignedMultipoleCorrFunc(edges, [mcf.mu_bins[0]] * (len(edges) - 1))
        for ell in range(5):
            weights = cf.legendre_weights(ell)
            np.testing.assert_allclose(weights, np.diff(legendre_primitive(ell, edges)), rtol=0, atol=1e-15)
            assert abs(weights.sum() - (2.0 if ell == 0 else 0.0)) <= 1e-15  # int_-1^1 P_ell = 2 delta_ell0
        for ell in (5, 6, 7, 8, np.int64(3)):
            assert abs(cf.legendre_weights(ell).sum()) <= 1e-14
        for bad in (9, -1, 2.0, True, "1", None):
            with pytest.raises(ValueError, match="integer in 0 ... 8"):
                cf.sample(bad)
        # every bin holds the same xi: the monopole is xi and every other multipole vanishes -- on any edges
        xi = mcf.mu_bins[0].sample()
        np.testing.assert_allclose(cf.sample(0).data, xi.data, rtol=1e-14)
        np.testing.assert_allclose(cf.sample().samples, xi.samples, rtol=1e-14)
        for ell in (1, 2, 3, 4):
            assert np.all(np.abs(cf.sample(ell).data) <= 1e-14 * np.abs(xi.data)), ell
    # xi antisymmetric across the mirrored bins: the even multipoles vanish and the dipole does not
    base = mcf.mu_bins[0]
    x = np.array([0.5, 0.3, 0.125])
    odd = yaw.SignedMultipoleCorrFunc(mcf.mu_edges, [scaled(base, 1.0 - v) for v in x[::-1]] + [scaled(base, 1.0 + v) for v in x])
    for j, sample in enumerate(odd.sample_xi()):
        np.testing.assert_allclose(sample.data, np.concatenate([-x[::-1], x])[j], rtol=1e-14)
    for ell in (0, 2, 4):
        assert np.all(np.abs(odd.sample(ell).data) <= 1e-15), ell
    dipole = 1.5 * 2.0 * np.sum(x * np.diff(legendre_primitive(1, mcf.mu_edges[3:])))
    np.testing.assert_allclose(odd.sample(1).data, dipole, rtol=1e-14)
    assert dipole > 0.1 and np.all(np.abs(odd.sample(3).data) > 1e-3)
    assert len(odd.sample_multipoles()) == 5 and len(odd.sample_multipoles((1, 3))) == 2
