"""CPU: shear-shear correlations between redshift bins and between catalogues (``correlate_shear_tomographic``) above the
device seam -- known answers of the contract with the two objects in different bins and in different catalogues, and the
driver with ``engine.count_shear_pair_fine`` replaced by the numpy brute force of tests/shear_pair_oracle.py."""
import os
import re

import numpy as np
import pytest

import shear_auto_oracle
import shear_pair_oracle
import yet_another_wizz_amd as yaw
from conftest import ARCMIN, ROOT
from yet_another_wizz_amd import engine, measurements
from yet_another_wizz_amd.catalog import InconsistentPatchesError, radec_to_xyz

G = 0.03
ZEDGES = np.array([0.1, 0.4, 0.7, 1.0])
PLANES = ("P", "M", "C")


def one_object(ra, dec, shear, nb=1, bin_=0):
    """One patch, ``nb`` bins, one object with unit weight in bin ``bin_``."""
    x, y, z = radec_to_xyz(np.array([ra], dtype=float), np.array([dec], dtype=float))
    off = np.zeros(nb + 1, dtype=np.int64)
    off[bin_ + 1:] = 1
    return dict(x=x, y=y, z=z, w=None, g1=np.array([shear[0]], dtype=float), g2=np.array([shear[1]], dtype=float), nb=nb, off=off)


# --------------------------------------------------------------------------- 1. known answers
@pytest.mark.parametrize("placed", ["two bins", "two catalogues"])
@pytest.mark.parametrize("where", ["equator", "meridian"])
def test_known_answers_from_two_objects(where, placed):
    """The known answers of the auto count (a pair along RA on the equator, a pair on one meridian), the two objects now in
    different redshift bins of one catalogue, then in two catalogues -- where the cell (0, 0, 0, 0) is NOT diagonal."""
    ra, dec = ([0.7, 0.7 + 3.0 * ARCMIN], [0.0, 0.0]) if where == "equator" else ([0.0, 0.0], [0.0, 3.0 * ARCMIN])
    g2 = G * G
    expected = [(((G, 0.0), (G, 0.0)), (g2, g2, 0.0)), (((0.0, G), (0.0, G)), (g2, -g2, 0.0))]
    if where == "equator":
        expected.append((((G, 0.0), (0.0, G)), (0.0, 0.0, g2)))
    t = (2.0 * np.sin(0.5 * np.array([[1.0, 5.0]]) * ARCMIN)) ** 2
    for shears, want in expected:
        if placed == "two bins":
            x, y, z = radec_to_xyz(np.asarray(ra, dtype=float), np.asarray(dec, dtype=float))
            cat = dict(x=x, y=y, z=z, w=None, g1=np.array([s[0] for s in shears]), g2=np.array([s[1] for s in shears]), nb=2,
                       off=np.array([0, 1, 2], dtype=np.int64))
            cells = [(0, 0, 0, 1, 0), (0, 0, 1, 0, 0), (0, 0, 0, 0, 0), (0, 0, 1, 1, 0)]
            P, M, C, W, _ = shear_pair_oracle.shear_pair_cells(cat, cat, cells, t)
            assert np.array_equal(W[:, 0], [1.0, 1.0, 0.0, 0.0])  # one object alone in its bin pairs with nothing
            assert (P[0, 0], M[0, 0], C[0, 0]) == (P[1, 0], M[1, 0], C[1, 0])  # the term is symmetric under the swap
        else:
            cat_a, cat_b = one_object(ra[0], dec[0], shears[0]), one_object(ra[1], dec[1], shears[1])
            P, M, C, W, _ = shear_pair_oracle.shear_pair_cells(cat_a, cat_b, [(0, 0, 0, 0, 0)], t)
            assert W[0, 0] == 1.0
        for value, ref in zip((P[0, 0], M[0, 0], C[0, 0]), want):
            assert abs(value - ref) <= 1e-14 * g2, (where, placed, shears)


def test_a_cell_between_two_catalogues_holds_both_orders():
    """The same segment as ``a`` and as ``b`` of two different catalogue objects: every ordered pair, twice the diagonal."""
    rng = np.random.default_rng(5)
    n = 40
    x, y, z = radec_to_xyz(rng.uniform(0.3, 0.3 + 6 * ARCMIN, n), rng.uniform(0.1, 0.1 + 6 * ARCMIN, n))
    cat = dict(x=x, y=y, z=z, w=rng.uniform(0.5, 2.0, n), g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n), nb=1,
               off=np.array([0, n], dtype=np.int64))
    t = (2.0 * np.sin(0.5 * np.array([[0.5, 2.0, 8.0]]) * ARCMIN)) ** 2
    once = shear_pair_oracle.shear_pair_cells(cat, cat, [(0, 0, 0, 0, 0)], t)
    both = shear_pair_oracle.shear_pair_cells(cat, dict(cat), [(0, 0, 0, 0, 0)], t)
    auto = shear_auto_oracle.shear_auto_jobs(cat, [[0, 0]], t)
    assert once[3].sum() > 100
    for a, b, c in zip(once, both, auto):
        assert np.array_equal(a, c[:, 0]) and np.allclose(b, 2.0 * a, rtol=1e-12, atol=0)


# --------------------------------------------------------------------------- 2. the driver on the oracle stand-in
def tomo_scenario(seed=23, shear=True, redshifts=True, n=1500, unit="arcmin", shift=0.0):
    """1500 weighted sources in three patches 12 arcmin apart and three redshift bins, a coherent shear plus noise."""
    rng = np.random.default_rng(seed)
    centre_ra = 0.30 + np.arange(3) * 12.0 * ARCMIN
    centers = yaw.AngularCoordinates(np.stack([centre_ra + shift, np.full(3, 0.10)], axis=1))
    which = rng.integers(0, 3, n)
    ra = centre_ra[which] + rng.uniform(-6.0, 6.0, n) * ARCMIN
    dec = 0.10 + rng.uniform(-6.0, 6.0, n) * ARCMIN
    columns = dict(weights=rng.uniform(0.5, 1.5, n))
    if shear:
        columns.update(g1=0.05 + rng.normal(0, 0.02, n), g2=-0.02 + rng.normal(0, 0.02, n))
    if redshifts:
        columns.update(redshifts=rng.uniform(0.1, 1.0, n))
    sources = yaw.Catalog.from_arrays(ra, dec, patch_centers=centers, degrees=False, **columns)
    if unit == "arcmin":
        config = yaw.Configuration.create(rmin=[0.9, 2.0], rmax=[8.1, 6.0], unit="arcmin", rweight=-0.8, resolution=12, edges=ZEDGES)
    else:
        config = yaw.Configuration.create(rmin=[100.0, 200.0], rmax=[1000.0, 800.0], unit="kpc", rweight=-0.8, resolution=12, edges=ZEDGES)
    return config, sources


def by_hand(config, cat_a, cat_b, bin_pairs):
    """{(i, j): f64[4, S]} -- sum P, M, C, W of bin pair (i, j) per scale from the oracle's fine bins of a cell list built
    here, combined with a ``CombinePlan`` over the plan of bin min(i, j)."""
    one = cat_b is None
    layout_a = cat_a.build_trees(ZEDGES, with_shear=True)
    layout_b = layout_a if one else cat_b.build_trees(ZEDGES, with_shear=True)
    o_a = shear_auto_oracle.as_catalogue(layout_a)
    o_b = o_a if one else shear_auto_oracle.as_catalogue(layout_b)
    links = yaw.PatchLinkage.from_catalogs(config, *((cat_a,) if one else (cat_a, cat_b)))
    plans, thresholds = links._angular_setup()
    out = {}
    for i, j in bin_pairs:
        jobs = links.get_patch_pairs(cat_a) if one and i == j else links.get_patch_pairs(cat_a, cat_a if one else cat_b)
        assert np.all(jobs[:, 0] <= jobs[:, 1]) if one and i == j else np.any(jobs[:, 0] > jobs[:, 1])
        cells = [(p, q, i, j, min(i, j)) for p, q in jobs]
        fine = shear_pair_oracle.shear_pair_cells(o_a, o_b, cells, thresholds)
        combine = measurements.CombinePlan([plans[min(i, j)]])
        out[i, j] = np.array([combine(f.T[np.newaxis]).sum(axis=2)[:, 0] for f in fine[:4]])  # [4, S]
    return out


def check_result(result, expected, num_bins=3):
    """``result`` of the driver against ``expected`` of ``by_hand``: asked-for slots hold the ratios, the rest NaN."""
    assert isinstance(result, list) and len(result) == 2
    for s, rows in enumerate(result):
        assert len(rows) == num_bins
        for i, triple in enumerate(rows):
            assert len(triple) == 3
            for cf in triple:
                assert type(cf) is yaw.ScalarCorrFunc and cf.dr is None
                assert not cf.dd.kappa_counts.auto and not cf.dd.number_counts.auto
                assert cf.sample().samples.shape == (3, num_bins)  # [P, B]
            data = [cf.sample().data for cf in triple]
            for j in range(num_bins):
                if (i, j) not in expected:
                    continue
                P, M, C, W = expected[i, j][:, s]
                assert W > 0
                np.testing.assert_allclose(data[0][j], P / W, rtol=1e-10)
                np.testing.assert_allclose(data[1][j], M / W, rtol=1e-8, atol=1e-12)
                np.testing.assert_allclose(data[2][j], C / W, rtol=1e-8, atol=1e-12)
                np.testing.assert_allclose(triple[0].dd.number_counts.counts[j].sum(), W, rtol=1e-12)
                assert data[0][j] > 0.05 ** 2  # the coherent part


def check_tomo_scenario():
    """One catalogue with all i <= j and two catalogues with all B * B pairs; ``engine.count_shear_pair_fine`` is whatever
    the caller left in place."""
    config, sources = tomo_scenario()
    upper = [(i, j) for i in range(3) for j in range(i, 3)]
    expected = by_hand(config, sources, None, upper)
    result = yaw.correlate_shear_tomographic(config, sources)
    check_result(result, {**expected, **{(j, i): v for (i, j), v in expected.items()}})
    _, other = tomo_scenario(seed=29, n=1100)
    both = [(i, j) for i in range(3) for j in range(3)]
    check_result(yaw.correlate_shear_tomographic(config, sources, other), by_hand(config, sources, other, both))
    return result


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_shear_pair_fine", shear_pair_oracle.count_shear_pair_fine)
    monkeypatch.setattr(engine, "count_shear_auto_fine", shear_auto_oracle.count_shear_auto_fine)


def test_driver_on_the_oracle_stand_in(stand_in):
    check_tomo_scenario()


def test_same_bin_slots_are_autocorrelate_shear(stand_in):
    """Slot (i, i) of a one-catalogue call: the counts and the jackknife samples of ``autocorrelate_shear``."""
    config, sources = tomo_scenario()
    tomo = yaw.correlate_shear_tomographic(config, sources)
    auto = yaw.autocorrelate_shear(config, sources)
    for rows, triple in zip(tomo, auto):
        for i in range(3):
            for ours, ref in zip(rows[i], triple):
                for name in ("kappa_counts", "number_counts"):
                    got, want = getattr(ours.dd, name).counts[i], getattr(ref.dd, name).counts[i]
                    assert np.any(want != 0) and np.array_equal(got, want)
                    assert np.all(got[np.tril_indices(3, -1)] == 0)  # the upper triangle, every unordered pair once
                assert np.array_equal(ours.sample().data[i], ref.sample().data[i])
                assert np.array_equal(ours.sample().samples[:, i], ref.sample().samples[:, i])


def test_mirror_rule(stand_in):
    """One catalogue: slot j < i of row i is slot i of row j with the patch axes transposed; other slots are zero."""
    config, sources = tomo_scenario()
    for rows in yaw.correlate_shear_tomographic(config, sources):
        for i in range(3):
            for j in range(i):
                for c in range(3):
                    for name in ("kappa_counts", "number_counts"):
                        low, up = getattr(rows[i][c].dd, name).counts[j], getattr(rows[j][c].dd, name).counts[i]
                        assert np.any(up != 0) and np.array_equal(low, up.T)
                np.testing.assert_allclose(rows[i][0].sample().data[j], rows[j][0].sample().data[i], rtol=1e-13)


@pytest.mark.filterwarnings("ignore:invalid value encountered")  # 0 / 0 of the slots not asked for
def test_bin_pairs_restrict_the_count(stand_in, monkeypatch):
    config, sources = tomo_scenario()
    full = yaw.correlate_shear_tomographic(config, sources)
    seen = []

    def spy(layout_a, layout_b, cells, thresholds, **kwargs):
        seen.append(np.array(cells))
        return shear_pair_oracle.count_shear_pair_fine(layout_a, layout_b, cells, thresholds, **kwargs)

    monkeypatch.setattr(engine, "count_shear_pair_fine", spy)
    part = yaw.correlate_shear_tomographic(config, sources, bin_pairs=[(0, 2), (1, 1), (0, 2)])
    (cells,) = seen  # ONE call
    links = yaw.PatchLinkage.from_catalogs(config, sources)
    assert {(ka, kb) for ka, kb in cells[:, 2:4]} == {(0, 2), (1, 1)}
    assert len(cells) == len(links.get_patch_pairs(sources)) + len(links.get_patch_pairs(sources, sources))
    for rows_full, rows_part in zip(full, part):
        for i in range(3):
            for c in range(3):
                got, want = rows_part[i][c], rows_full[i][c]
                for j in range(3):
                    asked = (i, j) in ((0, 2), (2, 0), (1, 1))
                    for name in ("kappa_counts", "number_counts"):
                        counts = getattr(got.dd, name).counts[j]
                        assert np.array_equal(counts, getattr(want.dd, name).counts[j]) if asked else not np.any(counts)
                    assert np.isfinite(got.sample().data[j]) if asked else np.isnan(got.sample().data[j])
    # two catalogues take ordered pairs, i > j included
    _, other = tomo_scenario(seed=29, n=1100)
    del seen[:]
    rows = yaw.correlate_shear_tomographic(config, sources, other, bin_pairs=[(2, 0)])[0]
    assert {(ka, kb) for ka, kb in seen[0][:, 2:4]} == {(2, 0)}
    assert np.isfinite(rows[2][0].sample().data[0]) and np.isnan(rows[0][0].sample().data[2])


def test_physical_scales_take_the_thresholds_of_the_nearer_bin(stand_in, monkeypatch):
    config, sources = tomo_scenario(unit="kpc")
    seen = []

    def spy(layout_a, layout_b, cells, thresholds, **kwargs):
        seen.append((np.array(cells), np.array(thresholds)))
        return shear_pair_oracle.count_shear_pair_fine(layout_a, layout_b, cells, thresholds, **kwargs)

    monkeypatch.setattr(engine, "count_shear_pair_fine", spy)
    result = yaw.correlate_shear_tomographic(config, sources)
    (cells, thresholds), = seen
    assert np.array_equal(cells[:, 4], np.minimum(cells[:, 2], cells[:, 3]))
    assert thresholds.shape[0] == 3 and np.all(thresholds[0, -1] > thresholds[1:, -1])  # the nearer bin: the larger angle
    upper = [(i, j) for i in range(3) for j in range(i, 3)]
    expected = by_hand(config, sources, None, upper)
    check_result(result, expected)
    # and not those of the farther bin: the pairs of (0, 2) under row 2 are fewer
    layout = sources.build_trees(ZEDGES, with_shear=True)
    o = shear_auto_oracle.as_catalogue(layout)
    far = shear_pair_oracle.shear_pair_cells(o, o, [(p, q, 0, 2, 2) for p, q, *_ in cells[(cells[:, 2] == 0) & (cells[:, 3] == 2)]], thresholds)
    near = shear_pair_oracle.shear_pair_cells(o, o, [(p, q, 0, 2, 0) for p, q, *_ in cells[(cells[:, 2] == 0) & (cells[:, 3] == 2)]], thresholds)
    assert 0 < far[3].sum() < near[3].sum()


# --------------------------------------------------------------------------- 3. refusals
def test_driver_rejects_what_it_cannot_count(stand_in):
    config, sources = tomo_scenario()
    _, no_shear = tomo_scenario(seed=29, shear=False)
    _, no_z = tomo_scenario(seed=29, redshifts=False)
    with pytest.raises(ValueError, match="catalog has no 'g1'/'g2' attached"):
        yaw.correlate_shear_tomographic(config, no_shear)
    with pytest.raises(ValueError, match="catalog has no 'g1'/'g2' attached"):
        yaw.correlate_shear_tomographic(config, sources, no_shear)
    with pytest.raises(ValueError, match="redshifts"):
        yaw.correlate_shear_tomographic(config, no_z)
    with pytest.raises(ValueError, match="redshifts"):
        yaw.correlate_shear_tomographic(config, sources, no_z)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.correlate_shear_tomographic(config, sources, sources)
    _, moved = tomo_scenario(seed=29, shift=8.0 * ARCMIN)
    with pytest.raises(InconsistentPatchesError):
        yaw.correlate_shear_tomographic(config, sources, moved)
    with pytest.raises(ValueError, match="i <= j"):
        yaw.correlate_shear_tomographic(config, sources, bin_pairs=[(1, 0)])
    for bad in ((0, 3), (-1, 0)):
        with pytest.raises(ValueError, match="outside the 3 redshift bins"):
            yaw.correlate_shear_tomographic(config, sources, bin_pairs=[bad])


def test_several_ranks_are_refused(stand_in, monkeypatch):
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    config, sources = tomo_scenario()
    with pytest.raises(NotImplementedError):
        yaw.correlate_shear_tomographic(config, sources)


# --------------------------------------------------------------------------- 4. ABI
def test_new_symbol_is_declared_and_bound_at_abi_6():
    from yet_another_wizz_amd import _lib

    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "yawhip_shear_pair_count" in _lib.ABI_SYMBOLS
    assert re.search(r"\bint yawhip_shear_pair_count\s*\(", code)
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)
    assert "correlate_shear_tomographic" in yaw.__all__ and callable(engine.count_shear_pair_fine)
    assert hasattr(_lib.load_library(), "yawhip_shear_pair_count")
