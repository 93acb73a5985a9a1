"""The on-disk input contract (reference src/yaw/catalog/patch.py:164-178, datachunk.py:47-117,
catalog.py:325-331): a cache written by the reference is read back, and a cache written here holds
the same records in the same format. tests/golden/refcache/ was written by the reference (tools/make_golden.py)."""
import filecmp
import os

import numpy as np
import pytest

import helpers
import yet_another_wizz_amd as yaw
from conftest import GOLDEN, load_golden
from yet_another_wizz_amd import engine

REFCACHE = os.path.join(GOLDEN, "refcache")


def test_read_reference_cache():
    exp = load_golden("refcache_expect.npz")
    cat = yaw.Catalog(REFCACHE)
    assert cat.num_patches == 4 and cat.has_weights and cat.has_redshifts
    assert np.array_equal(np.array(cat.get_num_records()), exp["meta.num_records"])
    assert np.array_equal(cat.get_centers().data, exp["meta.centers"])  # read from meta.yml: exact
    assert np.array_equal(cat.get_radii().data, exp["meta.radii"])
    np.testing.assert_allclose(np.array(cat.get_sum_weights()), exp["meta.sum_weights"], rtol=1e-15)
    # same objects as the input frame (the reference stores radian)
    assert np.array_equal(np.sort(np.concatenate([cat[i].redshifts for i in range(4)])), np.sort(exp["input.z"]))
    np.testing.assert_allclose(np.sort(np.concatenate([cat[i].coords.ra for i in range(4)])),
                               np.sort(np.deg2rad(exp["input.ra"])), rtol=0, atol=0)


def test_written_cache_is_format_compatible(tmp_path):
    exp = load_golden("refcache_expect.npz")
    frame = dict(ra=exp["input.ra"], dec=exp["input.dec"], z=exp["input.z"], w=exp["input.w"])
    out = tmp_path / "mine"
    cat = yaw.Catalog.from_dataframe(out, frame, ra_name="ra", dec_name="dec", weight_name="w", redshift_name="z",
                                     patch_centers=yaw.AngularCoordinates(exp["patch_centers"]))
    assert filecmp.cmp(out / "patch_ids.bin", os.path.join(REFCACHE, "patch_ids.bin"), shallow=False)
    from yet_another_wizz_amd.catalog import read_patch_file

    for pid in range(4):
        mine, theirs = out / f"patch_{pid}" / "data.bin", os.path.join(REFCACHE, f"patch_{pid}", "data.bin")
        assert os.path.getsize(mine) == os.path.getsize(theirs)
        with open(mine, "rb") as f, open(theirs, "rb") as g:
            assert f.read(1) == g.read(1)  # header byte: which columns are present
        a, b = read_patch_file(mine), read_patch_file(theirs)
        assert list(a) == list(b) == ["ra", "dec", "weights", "redshifts"]
        # same records bit for bit; the order inside a patch is not defined by the reference
        # (its groupby uses an unstable argsort, utils/misc.py:54-59)
        rows_a = np.column_stack([a[c] for c in a])
        rows_b = np.column_stack([b[c] for c in b])
        assert np.array_equal(rows_a[np.lexsort(rows_a.T)], rows_b[np.lexsort(rows_b.T)]), pid
    back = yaw.Catalog(out)
    assert back.get_num_records() == cat.get_num_records()
    np.testing.assert_allclose(back.get_centers().data, exp["meta.centers"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(back.get_radii().data, exp["meta.radii"], rtol=1e-12)
    with pytest.raises(FileExistsError):
        cat.to_cache(out)
    cat.to_cache(out, overwrite=True)
    with pytest.raises(OSError):
        yaw.Catalog(tmp_path / "missing")


def test_cache_catalog_runs_through_the_driver(monkeypatch):
    """A catalogue restored from a reference cache gives the same counts as one built from the frame."""
    helpers.use_oracle_engine(monkeypatch)
    exp = load_golden("refcache_expect.npz")
    frame = dict(ra=exp["input.ra"], dec=exp["input.dec"], z=exp["input.z"], w=exp["input.w"])
    centers = yaw.AngularCoordinates(exp["patch_centers"])
    kw = dict(ra_name="ra", dec_name="dec", weight_name="w", patch_centers=centers)
    config = yaw.Configuration.create(rmin=0.5, rmax=8.0, unit="arcmin", zmin=0.1, zmax=1.0, num_bins=4)
    unk = yaw.Catalog.from_dataframe(None, frame, **kw)
    rnd = yaw.Catalog.from_dataframe(None, frame, **kw)
    a = yaw.crosscorrelate(config, yaw.Catalog(REFCACHE), unk, unk_rand=rnd)[0]
    b = yaw.crosscorrelate(config, yaw.Catalog.from_dataframe(None, frame, redshift_name="z", **kw), unk, unk_rand=rnd)[0]
    # weighted sums: same pairs, but the cache holds the objects in another order -> last-bit differences
    np.testing.assert_allclose(a.dd.counts.counts, b.dd.counts.counts, rtol=1e-12, atol=0)
    assert a.dd.counts.counts.sum() > 0
    np.testing.assert_allclose(a.dr.sum_weights.sum_weights1, b.dr.sum_weights.sum_weights1, rtol=1e-13)


def test_reference_cache_measurements_match_the_reference(monkeypatch):
    """Host logic (oracle standing in for the device): counts measured from the reference-written cache equal what
    the reference measured from it. The device version is tests/test_gpu_api_parity.py::test_reference_cache_on_gpu."""
    helpers.use_oracle_engine(monkeypatch)
    helpers.run_refcache_case()


def _read_cache_as_the_reference_does(directory):
    """The reference's reader of a cache, restated from its format (catalog.py:325-331, patch.py:149-178,
    datachunk.py:74-117) without this package: patch_ids.bin = int16 ids; patch_<id>/meta.yml = exactly the keys
    Metadata.from_dict takes; patch_<id>/data.bin = one byte of column flags, then float64 records."""
    import yaml

    flag_bits = dict(ra=0, dec=1, weights=2, redshifts=3, patch_ids=4, kappa=5)
    ids = np.fromfile(os.path.join(directory, "patch_ids.bin"), dtype=np.int16).tolist()
    metas, records, columns = [], [], []
    for pid in ids:
        with open(os.path.join(directory, f"patch_{pid}", "meta.yml")) as f:
            meta = yaml.safe_load(f)
        assert set(meta) == {"num_records", "sum_weights", "center", "radius"}, meta
        assert isinstance(meta["num_records"], int) and len(meta["center"]) == 2
        metas.append(meta)
        with open(os.path.join(directory, f"patch_{pid}", "data.bin"), "rb") as f:
            state = f.read(1)[0]
            raw = np.fromfile(f, dtype=np.byte)
        names = [name for name, bit in flag_bits.items() if state & (1 << bit)]
        assert state < (1 << len(flag_bits)) and names[:2] == ["ra", "dec"], state
        assert raw.size % (8 * len(names)) == 0
        records.append(raw.view([(name, "f8") for name in names]))
        columns.append(names)
    return ids, metas, records, columns


def test_reference_reads_our_cache(tmp_path):
    """Other direction: the reference restores a cache written here. tests/golden/ourcache_reference_readback.npz holds
    what the reference read from a cache this package wrote from the same frame (tools/make_golden.py
    --ourcache-readback); a fresh cache, parsed as the reference parses it, must give the same."""
    exp = load_golden("refcache_expect.npz")
    got = load_golden("ourcache_reference_readback.npz")
    frame = dict(ra=exp["input.ra"], dec=exp["input.dec"], z=exp["input.z"], w=exp["input.w"])
    out = tmp_path / "mine"
    cat = yaw.Catalog.from_dataframe(out, frame, ra_name="ra", dec_name="dec", weight_name="w", redshift_name="z",
                                     patch_centers=yaw.AngularCoordinates(exp["patch_centers"]))
    ids, metas, records, columns = _read_cache_as_the_reference_does(out)
    assert ids == list(range(4)) and bool(got["has_weights"]) and bool(got["has_redshifts"])
    assert all(names == ["ra", "dec", "weights", "redshifts"] for names in columns)
    assert [m["num_records"] for m in metas] == got["meta.num_records"].tolist() == list(cat.get_num_records())
    assert [len(r) for r in records] == got["meta.num_records"].tolist()
    np.testing.assert_allclose([m["center"] for m in metas], got["meta.centers"], rtol=0, atol=1e-14)
    np.testing.assert_allclose([m["radius"] for m in metas], got["meta.radii"], rtol=1e-12)
    np.testing.assert_allclose([m["sum_weights"] for m in metas], got["meta.sum_weights"], rtol=1e-13)
    for pid, rec in enumerate(records):
        # the records the reference returned, bit for bit (order inside a patch is not part of the format)
        mine = np.column_stack([rec[name] for name in columns[pid]])
        theirs = got[f"patch_{pid}.records"]
        assert np.array_equal(mine[np.lexsort(mine.T)], theirs[np.lexsort(theirs.T)]), pid
