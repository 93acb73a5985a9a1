"""GPU: per-patch redshift histograms (yawhip_redshift_histogram, csrc/yawhip_hist.hip) and HistData.from_catalog against
the reference (tests/golden/histdata_*.npz, tools/make_golden_nz.py) and against the reference's per-patch numpy
function on random inputs: edges hit exactly, NaN, empty and single-object patches, 1 .. 10 000 bins (LDS and global
scratch paths), chunk boundaries inside patches and tiles, and 5e7 weighted objects. Then the result files end to end."""
import math
import os

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from conftest import GOLDEN, load_golden
from helpers import twodflens_catalogs
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.config import BinningConfig

pytestmark = pytest.mark.gpu

DEFAULT_CHUNK_LOG2 = 23


def reference_patch_histogram(z, w, edges, closed):
    """The reference's worker function (src/yaw/redshifts.py:44-57) on one patch's columns."""
    mask = z > edges[0] if closed == "right" else z < edges[-1]
    counts, _ = np.histogram(z[mask], edges, weights=None if w is None else w[mask])
    return counts.astype(np.float64)


def reference_counts(z, w, offsets, edges, closed):
    return np.array([reference_patch_histogram(z[lo:hi], None if w is None else w[lo:hi], edges, closed)
                     for lo, hi in zip(offsets[:-1], offsets[1:])]).reshape(len(offsets) - 1, len(edges) - 1)


def bin_keys(z, offsets, edges, closed):
    """(patch * B + bin) of every kept object, -1 for dropped ones: the rule written out with searchsorted."""
    n_bins = len(edges) - 1
    idx = np.searchsorted(edges, z, side="right") - 1
    idx[z == edges[-1]] = n_bins - 1
    keep = (z >= edges[0]) & (z <= edges[-1]) & (z > edges[0] if closed == "right" else z < edges[-1])
    patch = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return np.where(keep, patch * n_bins + idx, -1)


def fsum_counts(z, w, offsets, edges, closed):
    n_bins = len(edges) - 1
    keys = bin_keys(z, offsets, edges, closed)
    out = np.zeros((len(offsets) - 1) * n_bins)
    order = np.argsort(keys, kind="stable")
    keys, w = keys[order], w[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    for lo, hi in zip(starts, np.r_[starts[1:], len(keys)]):
        if keys[lo] >= 0:
            out[keys[lo]] = math.fsum(w[lo:hi])
    return out.reshape(len(offsets) - 1, n_bins)


def device_counts(z, w, offsets, edges, closed, chunk_log2=None):
    ctx = engine.get_context(engine.default_devices()[0])
    if chunk_log2 is None:
        return engine.redshift_histogram(z, w, offsets, edges, closed == "right")
    ctx.set_option("hist_chunk_log2", chunk_log2)
    try:
        return engine.redshift_histogram(z, w, offsets, edges, closed == "right")
    finally:
        ctx.set_option("hist_chunk_log2", DEFAULT_CHUNK_LOG2)


def irregular_edges(rng, n_bins, lo=0.05, hi=2.5):
    while True:
        edges = np.sort(rng.uniform(lo, hi, n_bins + 1))
        if np.all(np.diff(edges) > 0):
            return edges


def random_sample(rng, sizes, edges):
    """Redshifts over and beyond the edges, a share of them exactly on edges, some NaN; positive weights."""
    n = int(np.sum(sizes))
    z = rng.uniform(edges[0] - 0.2, edges[-1] + 0.2, n)
    on = rng.random(n) < 0.2
    z[on] = edges[rng.integers(0, len(edges), int(on.sum()))]
    z[rng.random(n) < 0.01] = np.nan
    w = rng.uniform(0.1, 3.0, n)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return z, w, offsets


def assert_fsum_close(got, want):
    """Weighted sums within 1e-10 (relative) of math.fsum per (patch, bin)."""
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want))


def assert_weighted_close(got, want, w, offsets):
    """rtol 1e-10 plus 1e-12 x the patch's sum of weights: numpy's cumsum-difference rounding lives in the latter."""
    patch_sum = np.add.reduceat(np.r_[w, 0.0], offsets[:-1])[: len(offsets) - 1] if len(w) else np.zeros(len(offsets) - 1)
    patch_sum[np.diff(offsets) == 0] = 0.0
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want) + 1e-12 * patch_sum[:, None])


# --------------------------------------------------------------------------- the reference's fixtures
def edges_cases():
    return [str(c) for c in load_golden("histdata_edges.npz")["cases"]]


@pytest.fixture(scope="module")
def edges_catalogs():
    g = load_golden("histdata_edges.npz")
    kw = dict(redshifts=g["z"], patch_ids=g["patch"].astype(np.int64))
    return g, {False: yaw.Catalog.from_arrays(g["ra"], g["dec"], **kw),
               True: yaw.Catalog.from_arrays(g["ra"], g["dec"], weights=g["w"], **kw)}


def check_hist(hist, data, samples, weighted, total_weight):
    assert type(hist) is yaw.HistData
    if weighted:
        np.testing.assert_allclose(hist.data, data, rtol=1e-10, atol=1e-12 * total_weight)
        np.testing.assert_allclose(hist.samples, samples, rtol=1e-10, atol=1e-12 * total_weight)
    else:
        assert np.array_equal(hist.data, data)
        assert np.array_equal(hist.samples, samples)


@pytest.mark.parametrize("case", edges_cases())
def test_edges_fixture(case, edges_catalogs):
    g, cats = edges_catalogs
    weighted = bool(g[f"{case}.weighted"])
    config = BinningConfig.create(edges=g[f"{case}.edges"], closed=str(g[f"{case}.closed"]))
    hist = yaw.HistData.from_catalog(cats[weighted], config)
    assert np.array_equal(hist.binning.edges, g[f"{case}.edges"])
    check_hist(hist, g[f"{case}.data"], g[f"{case}.samples"], weighted, float(np.sum(g["w"])))


def test_refcache_fixture():
    g = load_golden("histdata_refcache.npz")
    cat = yaw.Catalog(os.path.join(GOLDEN, "refcache"))
    assert cat.has_weights and cat.has_redshifts
    for case in (str(c) for c in g["cases"]):
        config = yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", edges=g[f"{case}.edges"], closed=str(g[f"{case}.closed"]))
        hist = yaw.HistData.from_catalog(cat, config)
        check_hist(hist, g[f"{case}.data"], g[f"{case}.samples"], True, float(np.sum(cat._w)))


def test_twodflens_fixture():
    g = load_golden("histdata_2dflens.npz")
    _, cats, config = twodflens_catalogs()
    for closed in ("right", "left"):
        hist = yaw.HistData.from_catalog(cats["data"], config.modify(closed=closed))
        assert np.array_equal(hist.binning.edges, g["edges"])
        check_hist(hist, g[f"{closed}.data"], g[f"{closed}.samples"], True, float(np.sum(cats["data"]._w)))


# --------------------------------------------------------------------------- random cases against numpy
@pytest.mark.parametrize("n_bins", [1, 30, 2048, 2049, 10000])
@pytest.mark.parametrize("closed", ["right", "left"])
def test_random_bins(n_bins, closed):
    rng = np.random.default_rng(1000 * n_bins + (closed == "right"))
    sizes = rng.integers(0, 9000, 13)
    sizes[[2, 7]] = 0   # empty patches
    sizes[[4, 11]] = 1  # single objects
    edges = irregular_edges(rng, n_bins)
    z, w, offsets = random_sample(rng, sizes, edges)
    got = device_counts(z, None, offsets, edges, closed)
    assert got.shape == (13, n_bins)
    assert np.array_equal(got, reference_counts(z, None, offsets, edges, closed))
    got_w = device_counts(z, w, offsets, edges, closed)
    assert_fsum_close(got_w, fsum_counts(z, w, offsets, edges, closed))
    assert_weighted_close(got_w, reference_counts(z, w, offsets, edges, closed), w, offsets)


@pytest.mark.parametrize("n_patches", [1, 2, 64, 300])
@pytest.mark.parametrize("chunk_log2", [None, 8, 11])
def test_random_patches_and_chunks(n_patches, chunk_log2):
    rng = np.random.default_rng(n_patches * 100 + (chunk_log2 or 0))
    sizes = rng.integers(0, 12000 if n_patches < 64 else 1500, n_patches)
    if n_patches > 2:
        sizes[rng.choice(n_patches, n_patches // 5, replace=False)] = 0
        sizes[rng.choice(n_patches, n_patches // 7, replace=False)] = 1
    edges = irregular_edges(rng, 30, 0.1, 1.2)
    z, w, offsets = random_sample(rng, sizes, edges)
    for closed in ("right", "left"):
        got = device_counts(z, None, offsets, edges, closed, chunk_log2)
        assert np.array_equal(got, reference_counts(z, None, offsets, edges, closed))
        got_w = device_counts(z, w, offsets, edges, closed, chunk_log2)
        assert_fsum_close(got_w, fsum_counts(z, w, offsets, edges, closed))


def test_small_chunks_agree_with_one_chunk():
    """Counts are equal whatever the chunk size; weighted sums agree within the tolerance, since other tile cuts add the
    weights in another order."""
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 40000, 17)
    edges = irregular_edges(rng, 2049)
    z, w, offsets = random_sample(rng, sizes, edges)
    whole_n = device_counts(z, None, offsets, edges, "right")
    whole_w = device_counts(z, w, offsets, edges, "right")
    for chunk_log2 in (8, 12, 15):  # chunk boundaries inside patches and inside tiles of the whole-chunk call
        assert np.array_equal(device_counts(z, None, offsets, edges, "right", chunk_log2), whole_n)
        assert_weighted_close(device_counts(z, w, offsets, edges, "right", chunk_log2), whole_w, w, offsets)


def test_fifty_million_weighted():
    rng = np.random.default_rng(50)
    n, n_patches = 50_000_000, 64
    sizes = np.diff(np.sort(np.r_[0, rng.integers(0, n, n_patches - 1), n]))
    edges = np.linspace(0.07, 1.43, 31)
    z = rng.uniform(0.0, 1.5, n)
    z[: n // 50] = edges[rng.integers(0, 31, n // 50)]
    w = rng.integers(1, 4096, n) / 1024.0  # dyadic weights: every partial sum is exact, in any order
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for closed in ("right", "left"):
        keys = bin_keys(z, offsets, edges, closed)
        keep = keys >= 0
        want_n = np.bincount(keys[keep], minlength=n_patches * 30).reshape(n_patches, 30).astype(np.float64)
        want_w = np.bincount(keys[keep], weights=w[keep], minlength=n_patches * 30).reshape(n_patches, 30)
        assert np.array_equal(device_counts(z, None, offsets, edges, closed), want_n)
        assert np.array_equal(device_counts(z, w, offsets, edges, closed), want_w)


def test_argument_checks():
    ctx = engine.get_context(engine.default_devices()[0])
    z = np.array([0.5, 0.6])
    with pytest.raises(_lib.YawhipError, match="increase"):
        _lib.redshift_histogram(ctx, z, None, np.array([0, 2]), np.array([0.0, 1.0, 1.0]), True)
    with pytest.raises(_lib.YawhipError, match="offsets"):
        _lib.redshift_histogram(ctx, z, None, np.array([0, 1]), np.array([0.0, 1.0]), True)
    with pytest.raises(_lib.YawhipError, match="hist_chunk_log2"):
        ctx.set_option("hist_chunk_log2", 4)
    assert np.array_equal(_lib.redshift_histogram(ctx, np.empty(0), None, np.array([0, 0, 0]), np.array([0.0, 1.0]), True),
                          np.zeros((2, 1)))


# --------------------------------------------------------------------------- end to end
def test_estimate_to_files_and_back_and_histogram(tmp_path):
    _, cats, config = twodflens_catalogs()
    (cross,) = yaw.crosscorrelate(config, cats["data"], cats["unk"], ref_rand=cats["rand"])
    est = yaw.RedshiftData.from_corrfuncs(cross)
    est.to_files(tmp_path / "nz")
    back = yaw.RedshiftData.from_files(tmp_path / "nz")
    # the files hold 10 characters per value: at least 7 decimals for these magnitudes, edges included
    np.testing.assert_allclose(back.binning.edges, est.binning.edges, rtol=0, atol=5.1e-8)
    assert back.binning.closed == est.binning.closed
    np.testing.assert_allclose(back.data, est.data, rtol=0, atol=5.1e-8 * max(1.0, np.nanmax(np.abs(est.data))))
    np.testing.assert_allclose(back.samples, est.samples, rtol=0, atol=5.1e-8 * max(1.0, np.nanmax(np.abs(est.samples))))
    hist = yaw.HistData.from_catalog(cats["data"], config).normalised()
    assert np.isclose(np.nansum(hist.binning.dz * hist.data), 1.0)
    fitted = est.normalised(target=hist)
    assert fitted.data.shape == est.data.shape and np.all(np.isfinite(fitted.data[np.isfinite(est.data)]))
    for cat in cats.values():
        cat.drop_layouts()
