"""Scalar-field ("kappa") correlations, host side: the kappa column in the catalogue and its cache (both directions against
the reference), the result containers and the SC estimator against the reference's tensors, the error behaviour, the new
C-ABI symbols, and the drivers with the CPU oracle standing in for the device. Fixtures: tools/make_golden_scalar.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import helpers
import yet_another_wizz_amd as yaw
from conftest import GOLDEN, ROOT, load_golden
from yet_another_wizz_amd import _lib
from yet_another_wizz_amd.catalog import read_patch_file
from yet_another_wizz_amd.corrfunc import scalar_correlation
from yet_another_wizz_amd.options import CountMode

REFCACHE_KAPPA = os.path.join(GOLDEN, "refcache_kappa")
COLUMNS = ["ra", "dec", "weights", "redshifts", "kappa"]  # the reference's ATTR_ORDER without the never-stored patch ids
KW = dict(ra_name="ra", dec_name="dec", weight_name="w", redshift_name="z", kappa_name="kappa")


def _sorted_rows(rows):
    return rows[np.lexsort(rows.T)]  # the order inside a patch is not part of the format


def _cache_frame():
    g = load_golden("scalar_cache.npz")
    return g, {k: g[f"input.{k}"] for k in ("ra", "dec", "w", "z", "kappa")}, yaw.AngularCoordinates(g["patch_centers"])


# --------------------------------------------------------------------------- catalogue and cache
def test_kappa_column_follows_its_objects():
    g, frame, centers = _cache_frame()
    cat = yaw.Catalog.from_dataframe(None, frame, patch_centers=centers, **KW)
    assert cat.has_kappa and all(cat[pid].has_kappa for pid in cat)
    rows = np.concatenate([np.column_stack([cat[p].coords.ra, cat[p].coords.dec, cat[p].weights, cat[p].redshifts, cat[p].kappa])
                           for p in cat])
    src = np.column_stack([np.deg2rad(frame["ra"]), np.deg2rad(frame["dec"]), frame["w"], frame["z"], frame["kappa"]])
    assert np.array_equal(_sorted_rows(rows), _sorted_rows(src))
    same = yaw.Catalog.from_arrays(frame["ra"], frame["dec"], weights=frame["w"], redshifts=frame["z"], kappa=frame["kappa"],
                                   patch_centers=centers)
    assert all(np.array_equal(same[p].kappa, cat[p].kappa) for p in cat)
    plain = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", patch_centers=centers)
    assert not plain.has_kappa and plain[0].kappa is None and not plain[0].has_kappa
    with pytest.raises(ValueError, match="differ in length"):
        yaw.Catalog.from_arrays(frame["ra"], frame["dec"], kappa=frame["kappa"][:-1], patch_centers=centers)


def test_from_file_reads_kappa(tmp_path):
    g, frame, centers = _cache_frame()
    np.savez(tmp_path / "frame.npz", **frame)
    cat = yaw.Catalog.from_file(None, tmp_path / "frame.npz", patch_centers=centers, **KW)
    ref = yaw.Catalog.from_dataframe(None, frame, patch_centers=centers, **KW)
    assert cat.has_kappa and all(np.array_equal(cat[p].kappa, ref[p].kappa) for p in ref)


def test_objects_outside_the_binning_drop_their_kappa():
    """trees.py:414-419: kappa is binned with the other columns; what is outside the binning is gone from all of them."""
    g, frame, centers = _cache_frame()
    cat = yaw.Catalog.from_dataframe(None, frame, patch_centers=centers, **KW)
    edges = np.array([0.1, 0.3, 0.55, 0.8, 1.0])
    for closed in ("left", "right"):
        layout = cat.build_trees(edges, closed=closed, force=True)
        assert layout.twin is not None and len(layout.kappa) == len(layout.x) < len(frame["ra"])
        for pid in cat:
            z, k, w = cat[pid].redshifts, cat[pid].kappa, cat[pid].weights
            idx = np.digitize(z, edges, right=closed == "right")
            for b in range(4):
                lo, hi = layout.offsets[pid * 4 + b], layout.offsets[pid * 4 + b + 1]
                assert np.array_equal(np.sort(layout.kappa[lo:hi]), np.sort(k[idx == b + 1]))
                assert np.array_equal(np.sort(layout.twin.w[lo:hi]), np.sort(k[idx == b + 1] * w[idx == b + 1]))
    flat = cat.build_trees(None)
    assert np.array_equal(flat.kappa, np.concatenate([cat[p].kappa for p in cat]))
    no_w = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", kappa_name="kappa", patch_centers=centers)
    assert np.array_equal(no_w.build_trees(None).twin.w, no_w.build_trees(None).kappa)


def test_read_reference_kappa_cache():
    """A cache the reference wrote with kappa, read column for column."""
    g, frame, centers = _cache_frame()
    cat = yaw.Catalog(REFCACHE_KAPPA)
    assert cat.num_patches == 3 and cat.has_weights and cat.has_redshifts and cat.has_kappa
    assert g["reference_cache.flags"].tolist() == [True, True, True]
    assert list(cat.get_num_records()) == g["reference_cache.num_records"].tolist()
    for pid in range(3):
        path = os.path.join(REFCACHE_KAPPA, f"patch_{pid}", "data.bin")
        with open(path, "rb") as f:
            assert f.read(1)[0] == 0b101111  # ra, dec, weights, redshifts, kappa (bit 5); no patch ids (bit 4)
        assert list(read_patch_file(path)) == COLUMNS
        p = cat[pid]
        mine = np.column_stack([p.coords.ra, p.coords.dec, p.weights, p.redshifts, p.kappa])
        assert np.array_equal(mine, g[f"reference_cache.patch_{pid}.records"])  # the reference's read-back, row for row


def test_reference_reads_our_kappa_cache(tmp_path):
    """The other direction: scalar_cache.npz holds what the reference read from a cache this package wrote from the same
    frame; a fresh cache parsed by the format alone must hold those records, in the reference's column order."""
    g, frame, centers = _cache_frame()
    out = tmp_path / "mine"
    cat = yaw.Catalog.from_dataframe(out, frame, patch_centers=centers, **KW)
    assert g["our_cache.flags"].tolist() == [True, True, True]
    assert list(cat.get_num_records()) == g["our_cache.num_records"].tolist()
    for pid in range(3):
        with open(out / f"patch_{pid}" / "data.bin", "rb") as f:
            flags = f.read(1)[0]
            raw = np.fromfile(f, dtype=np.float64)
        assert flags == 0b101111
        rows = raw.reshape(-1, len(COLUMNS))  # ra, dec, weights, redshifts, kappa
        assert np.array_equal(_sorted_rows(rows), _sorted_rows(g[f"our_cache.patch_{pid}.records"])), pid
        assert np.array_equal(np.sort(rows[:, 4]), np.sort(cat[pid].kappa))
        theirs = os.path.join(REFCACHE_KAPPA, f"patch_{pid}", "data.bin")
        assert os.path.getsize(out / f"patch_{pid}" / "data.bin") == os.path.getsize(theirs)
    back = yaw.Catalog(out)
    assert back.has_kappa and all(np.array_equal(back[p].kappa, cat[p].kappa) for p in cat)
    # a catalogue without kappa writes the header it always wrote
    plain = tmp_path / "plain"
    yaw.Catalog.from_dataframe(plain, frame, ra_name="ra", dec_name="dec", weight_name="w", redshift_name="z", patch_centers=centers)
    with open(plain / "patch_0" / "data.bin", "rb") as f:
        assert f.read(1)[0] == 0b001111


# --------------------------------------------------------------------------- containers and estimator
def _golden_corrfuncs(prefix):
    g = load_golden("scalar_drivers.npz")
    binning = yaw.Binning(g["zedges"], closed="left" if prefix == "cross_rand" else "right")
    auto = prefix == "auto"
    cfs = []
    for s in range(2):
        counts = {}
        for kind in ("dd", "dr"):
            key = f"{prefix}.s{s}.{kind}"
            if f"{key}.kappa_counts" in g.files:
                counts[kind] = yaw.NormalisedScalarCounts(yaw.PatchedCounts(binning, g[f"{key}.kappa_counts"], auto=auto),
                                                          yaw.PatchedCounts(binning, g[f"{key}.number_counts"], auto=auto))
        cfs.append(yaw.ScalarCorrFunc(**counts))
    return g, cfs


@pytest.mark.parametrize("prefix", ["auto", "cross", "cross_rand"])
def test_containers_reproduce_the_reference(prefix, tmp_path):
    g, cfs = _golden_corrfuncs(prefix)
    for s, cf in enumerate(cfs):
        assert cf.get_estimator() is scalar_correlation and cf.get_estimator().name == "SC"
        assert (cf.dr is None) == (prefix == "auto") and cf.rd is None and cf.rr is None
        for kind, counts in cf.to_dict().items():
            sampled = counts.sample_patch_sum()
            np.testing.assert_allclose(sampled.data, g[f"{prefix}.s{s}.{kind}.sample_data"], rtol=1e-12, atol=0)
            np.testing.assert_allclose(sampled.samples, g[f"{prefix}.s{s}.{kind}.sample_samples"], rtol=1e-12, atol=0)
            total = counts.number_counts.sample_patch_sum().data
            assert np.array_equal(counts.get_array(), counts.kappa_counts.counts / total[:, None, None])
        corr = cf.sample()
        np.testing.assert_allclose(corr.data, g[f"{prefix}.s{s}.corr_data"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(corr.samples, g[f"{prefix}.s{s}.corr_samples"], rtol=1e-12, atol=0)
        dd = cf.dd.sample_patch_sum()
        if cf.dr is None:  # SC without DR is DD itself
            assert np.array_equal(corr.data, dd.data) and np.array_equal(corr.samples, dd.samples)
        else:
            dr = cf.dr.sample_patch_sum()
            assert np.array_equal(corr.data, dd.data - dr.data) and np.array_equal(corr.samples, dd.samples - dr.samples)
        corr.to_files(tmp_path / f"scale{s}")
        back = yaw.CorrData.from_files(tmp_path / f"scale{s}")
        assert back.binning == corr.binning
        # (the file format keeps 10 characters per number: at least six decimals of values below 10)
        assert np.all(np.abs(corr.data) < 10)
        np.testing.assert_allclose(back.data, corr.data, rtol=0, atol=1e-6)
        np.testing.assert_allclose(back.samples, corr.samples, rtol=0, atol=1e-6)


def test_scalar_containers_compare_and_slice():
    g, (cf0, cf1) = _golden_corrfuncs("cross")
    _, (again, _) = _golden_corrfuncs("cross")
    assert cf0 == again and not (cf0 == cf1) and cf0.is_compatible(cf1)
    assert cf0.dd == again.dd and cf0.dd.is_compatible(cf1.dd) and not (cf0.dd == cf1.dd)
    assert yaw.ScalarCorrFunc.from_dict(cf0.to_dict()) == cf0
    bins = cf0.bins_subset([1, 2])
    assert bins.num_bins == 2 and np.array_equal(bins.dd.kappa_counts.counts, cf0.dd.kappa_counts.counts[1:3])
    assert np.array_equal(bins.sample().data, cf0.sample().data[1:3])
    patches = cf0.patches_subset([0, 3, 5])
    assert patches.num_patches == 3
    assert np.array_equal(patches.dr.number_counts.counts, cf0.dr.number_counts.counts[:, [0, 3, 5]][:, :, [0, 3, 5]])
    assert not cf0.is_compatible(bins) and not cf0.dd.is_compatible(patches.dd)
    # scalar and number containers do not mix
    nn = yaw.NormalisedCounts(cf0.dd.number_counts, yaw.PatchedSumWeights(cf0.binning, np.ones((4, 8)), np.ones((4, 8)), auto=False))
    assert not cf0.dd.is_compatible(nn) and not nn.is_compatible(cf0.dd) and not (cf0.dd == nn)
    with pytest.raises(TypeError):
        yaw.ScalarCorrFunc(nn)
    with pytest.raises(TypeError):
        yaw.CorrFunc(cf0.dd, cf0.dr)
    with pytest.raises(TypeError):
        yaw.NormalisedScalarCounts(cf0.dd.kappa_counts, nn.sum_weights)
    with pytest.raises(ValueError, match="not compatible"):
        yaw.ScalarCorrFunc(cf0.dd, bins.dr)


# --------------------------------------------------------------------------- errors
def _driver_catalogs(g, *, weights, kappa_on=("ref",)):
    centers = yaw.AngularCoordinates(g["patch_centers"])
    cats = {}
    for name in ("ref", "unk", "rnd"):
        frame = {k.split(".", 1)[1]: g[k] for k in g.files if k.startswith(name + ".")}
        cats[name] = yaw.Catalog.from_dataframe(
            None, frame, ra_name="ra", dec_name="dec", weight_name="w" if weights and "w" in frame else None,
            redshift_name="z" if "z" in frame else None, kappa_name="kappa" if name in kappa_on and "kappa" in frame else None,
            patch_centers=centers)
    return cats


def _driver_config(g, *, closed="right", rweight=None):
    return yaw.Configuration.create(rmin=g["rmin"], rmax=g["rmax"], unit="arcmin", edges=g["zedges"], closed=closed,
                                    rweight=rweight, resolution=12 if rweight is not None else None)


def test_count_modes_and_their_errors(monkeypatch):
    helpers.use_oracle_engine(monkeypatch)
    assert [str(m) for m in CountMode] == ["nn", "nk", "kn", "kk"] and CountMode.parse("kn") is CountMode.kn == "kn"
    g = load_golden("scalar_drivers.npz")
    config = _driver_config(g)
    cats = _driver_catalogs(g, weights=False)
    ref, unk = cats["ref"], cats["unk"]
    ref.build_trees(config.binning.edges, closed="right")
    unk.build_trees(None)
    links = yaw.PatchLinkage.from_catalogs(config, ref, unk)
    with pytest.raises(ValueError, match=re.escape("missing required 'kappa' for second tree.")):
        links.count_pairs(ref, unk, mode="nk")
    with pytest.raises(ValueError, match=re.escape("missing required 'kappa' for first tree.")):
        links.count_pairs(unk, ref, mode="kn")
    with pytest.raises(ValueError, match=re.escape("missing required 'kappa' for both tree.")):
        links.count_pairs(ref, unk, mode="kk")
    with pytest.raises(ValueError, match=re.escape("missing required 'kappa' for both tree.")):
        links.count_scalar_pairs(unk, mode="kk")
    for bad in ("kappa", "NN", "k", "", "nnk"):
        with pytest.raises(ValueError):
            links.count_pairs(ref, unk, mode=bad)
        with pytest.raises(ValueError):
            links.count_pairs_batch([((ref, unk), "DD", bad), ((ref, unk), "DR")])
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_scalar(config, ref, ref)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_scalar(config, ref, unk, unk_rand=unk)
    with pytest.raises(ValueError, match="no 'kappa'"):
        yaw.compute_scalar_normalisation(unk, config.binning.binning)
    # the modes that are valid here run, and "nn" is what it always was
    nn = links.count_pairs(ref, unk)
    assert all(a.counts == b.counts for a, b in zip(nn, links.count_pairs(ref, unk, mode=CountMode.nn)))
    assert all(a.counts == b.counts for a, b in zip(nn, links.count_pairs(ref, unk, mode="nn")))
    kn = links.count_pairs(ref, unk, mode="kn")
    assert type(kn[0]) is yaw.NormalisedCounts and kn[0].sum_weights == nn[0].sum_weights and not (kn[0].counts == nn[0].counts)


# --------------------------------------------------------------------------- the C ABI
def test_abi_declares_binds_and_exports_the_scalar_entry_points():
    header = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("yawhip_catalog_upload_scalar", "yawhip_catalog_segment_sums"):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
    assert int(re.search(r"#define YAWHIP_ABI_VERSION (\d+)", header).group(1)) == 6
    lib.yawhip_abi_version.restype = ctypes.c_int
    assert lib.yawhip_abi_version() == 6
    loaded = _lib.load_library()
    assert len(loaded.yawhip_catalog_upload_scalar.argtypes) == 13 and len(loaded.yawhip_catalog_upload_axis.argtypes) == 11
    # errors are reported, not thrown, and no handle comes back
    out_n, out_k = ctypes.c_void_p(1), ctypes.c_void_p(1)
    assert loaded.yawhip_catalog_upload_scalar(None, 0, None, None, None, None, None, 1, 1, None, 2, ctypes.byref(out_n),
                                               ctypes.byref(out_k)) == -1
    assert not out_n.value and not out_k.value
    for axis, kappa in ((3, None), (-1, None), (2, None)):  # whichever check fails first (sort axis, kappa of n > 0, context)
        out_n, out_k = ctypes.c_void_p(1), ctypes.c_void_p(1)
        assert loaded.yawhip_catalog_upload_scalar(None, 1 if axis == 2 else 0, None, None, None, None, kappa, 1, 1, None, axis,
                                                   ctypes.byref(out_n), ctypes.byref(out_k)) == -1
        assert not out_n.value and not out_k.value, axis
    assert loaded.yawhip_catalog_segment_sums(None, None) == -1 and b"NULL" in loaded.yawhip_last_error()


# --------------------------------------------------------------------------- drivers on the CPU oracle
def _check_scalar_counts(key, counts, g, *, exact_nn):
    """The rule of the GPU tests: number counts exact (unweighted) or to 1e-10, κ-weighted slots to 1e-10 of the
    cancellation-free magnitude the reference reports for the slot (``abs_counts``), exactly 0 where that is 0."""
    if exact_nn:
        assert np.array_equal(counts.number_counts.counts, g[f"{key}.number_counts"]), key
    else:
        np.testing.assert_allclose(counts.number_counts.counts, g[f"{key}.number_counts"], rtol=helpers.RTOL_W, atol=0, err_msg=key)
    got, exp, mag = counts.kappa_counts.counts, g[f"{key}.kappa_counts"], g[f"{key}.abs_counts"]
    assert np.all(np.abs(got - exp) <= 1e-10 * mag), (key, np.max(np.abs(got - exp) / np.where(mag > 0, mag, 1.0)))
    assert np.all(got[mag == 0] == 0.0), key
    assert np.count_nonzero(mag) > 50, key


def test_drivers_against_the_reference_with_the_oracle_engine(monkeypatch):
    """Host logic of ``autocorrelate_scalar`` and ``crosscorrelate_scalar(unk_rand=...)`` (mode -> twin, two or four requests
    in one batch, containers) with the CPU oracle standing in for the device. The forms that need the device's segment sums
    are GPU tests (tests/test_gpu_scalar.py)."""
    helpers.use_oracle_engine(monkeypatch)
    g = load_golden("scalar_drivers.npz")
    cats = _driver_catalogs(g, weights=True)
    cfs = yaw.autocorrelate_scalar(_driver_config(g), cats["ref"])
    for s, cf in enumerate(cfs):
        assert type(cf) is yaw.ScalarCorrFunc and cf.dr is None and cf.auto
        _check_scalar_counts(f"auto.s{s}.dd", cf.dd, g, exact_nn=False)
        np.testing.assert_allclose(cf.sample().data, g[f"auto.s{s}.corr_data"], rtol=1e-7, atol=1e-12)
    cats = _driver_catalogs(g, weights=False)
    cfs = yaw.crosscorrelate_scalar(_driver_config(g, closed="left", rweight=-1.0), cats["ref"], cats["unk"], unk_rand=cats["rnd"])
    for s, cf in enumerate(cfs):
        _check_scalar_counts(f"cross_rand.s{s}.dd", cf.dd, g, exact_nn=False)  # (separation weights: not integers)
        _check_scalar_counts(f"cross_rand.s{s}.dr", cf.dr, g, exact_nn=False)
        np.testing.assert_allclose(cf.sample().data, g[f"cross_rand.s{s}.corr_data"], rtol=1e-7, atol=1e-12)
