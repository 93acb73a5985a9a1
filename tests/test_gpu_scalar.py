"""GPU: scalar-field ("kappa") correlations on the device -- the κ-weighted twin catalogue of ``yawhip_catalog_upload_scalar``,
the four counting modes, the drivers and the segment sums, against the tensors the reference produced
(tools/make_golden_scalar.py).

The rule for every κ-weighted slot: ``|ours - reference| <= 1e-10 * abs_counts[slot]`` -- the project's weighted-sum tolerance
taken relative to the cancellation-free magnitude the reference itself reports for the slot (the same count with ``|kappa|``),
not to the signed sum, which cancels; a slot whose ``abs_counts`` is 0 must be exactly 0. Number counts of unweighted input are
bit-exact, weighted ones within 1e-10 relative."""
import numpy as np
import pytest

import helpers
import yet_another_wizz_amd as yaw
from conftest import load_golden
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
RTOL_W = helpers.RTOL_W


def check_kappa_slots(key, got, exp, mag):
    err = np.abs(got - exp)
    worst = float(np.max(err / np.where(mag > 0, mag, 1.0)))
    print(f"{key}: worst |ours - ref| / abs_counts = {worst:.3e} over {np.count_nonzero(mag)} slots")
    assert got.shape == exp.shape == mag.shape
    assert np.all(err <= 1e-10 * mag), (key, worst)  # every slot, none skipped (abs_counts == 0 allows no error at all)
    assert np.all(got[mag == 0] == 0.0), key


def check_number_counts(key, got, exp, *, exact):
    if exact:
        assert np.array_equal(got, exp), key
    else:
        np.testing.assert_allclose(got, exp, rtol=RTOL_W, atol=0, err_msg=key)


# --------------------------------------------------------------------------- the seam: every mode against the reference
def _seam_catalogs(g, weighted):
    centers = yaw.AngularCoordinates(g["patch_centers"])
    cats = []
    for name in ("one", "two"):
        frame = {k.split(".", 1)[1]: g[k] for k in g.files if k.startswith(name + ".")}
        cats.append(yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", weight_name="w" if weighted else None,
                                               redshift_name="z" if "z" in frame else None, kappa_name="kappa",
                                               patch_centers=centers))
    return cats


@pytest.mark.parametrize("weighted", [False, True], ids=["u", "w"])
@pytest.mark.parametrize("closed", ["left", "right"])
def test_seam_modes_match_the_reference(weighted, closed):
    g = load_golden("scalar_seam.npz")
    one, two = _seam_catalogs(g, weighted)
    n_checked = 0
    for rweight in (None, -1.0):
        config = yaw.Configuration.create(rmin=g["rmin"], rmax=g["rmax"], unit="arcmin", rweight=rweight,
                                          resolution=12 if rweight is not None else None, edges=g["zedges"], closed=closed)
        one.build_trees(config.binning.edges, closed=closed)
        two.build_trees(None)
        links = yaw.PatchLinkage(config, {0: {0, 1}, 1: {0, 1}})  # all four patch pairs, as recorded
        for mode in ("nn", "nk", "kn", "kk"):
            case = f"{mode}.{'w' if weighted else 'u'}.{closed}.{'plain' if rweight is None else 'rw-1'}"
            assert case in g["cases"]
            counts = np.stack([c.counts.counts for c in links.count_pairs(one, two, mode=mode)])  # [S, B, 2, 2]
            exp, mag = g[f"{case}.counts"], g[f"{case}.abs_counts"]
            if mode == "nn":
                assert np.array_equal(exp, mag)  # (no kappa in it)
                check_number_counts(case, counts, exp, exact=not weighted)
            else:
                assert np.any(exp < 0) and np.any(exp > 0) and np.all(np.abs(exp) <= mag)  # the cancellation is real
                check_kappa_slots(case, counts, exp, mag)
            n_checked += 1
    assert n_checked == 8
    one.drop_layouts()
    two.drop_layouts()


# --------------------------------------------------------------------------- drivers
def _driver_catalogs(g, *, weights):
    centers = yaw.AngularCoordinates(g["patch_centers"])
    cats = {}
    for name in ("ref", "unk", "rnd"):
        frame = {k.split(".", 1)[1]: g[k] for k in g.files if k.startswith(name + ".")}
        cats[name] = yaw.Catalog.from_dataframe(
            None, frame, ra_name="ra", dec_name="dec", weight_name="w" if weights and "w" in frame else None,
            redshift_name="z" if "z" in frame else None, kappa_name="kappa" if "kappa" in frame else None, patch_centers=centers)
    return cats


def _driver_config(g, *, closed="right", rweight=None):
    return yaw.Configuration.create(rmin=g["rmin"], rmax=g["rmax"], unit="arcmin", edges=g["zedges"], closed=closed,
                                    rweight=rweight, resolution=12 if rweight is not None else None)


def _check_scalar_counts(key, counts, g, *, exact_nn):
    assert type(counts) is yaw.NormalisedScalarCounts
    check_number_counts(key, counts.number_counts.counts, g[f"{key}.number_counts"], exact=exact_nn)
    check_kappa_slots(key, counts.kappa_counts.counts, g[f"{key}.kappa_counts"], g[f"{key}.abs_counts"])
    assert np.count_nonzero(g[f"{key}.abs_counts"]) > 50


def _check_samples(prefix, cfs, g):
    """sample(): the estimator of patch sums that cancel, so its error is measured on the scale of the cancellation-free
    ratio sum(abs_counts) / sum(number_counts). The bound follows from the slot rule: every κ slot is within 1e-10 of its
    abs_counts, so a patch sum is within 1e-10 * sum(abs_counts); the number counts add 1e-10 relative, a DR term (at most
    the mean |kappa|, i.e. of the order of the scale) as much again: below 1e-9 * scale for the data. A jackknife sample
    leaves out a row and a column of both sums, which shifts the scale by a factor near (P - 1) / P: 1e-8 covers it."""
    for s, cf in enumerate(cfs):
        corr = cf.sample()
        scale = g[f"{prefix}.s{s}.dd.abs_counts"].sum(axis=(1, 2)) / g[f"{prefix}.s{s}.dd.number_counts"].sum(axis=(1, 2))
        assert np.all(np.abs(corr.data - g[f"{prefix}.s{s}.corr_data"]) <= 1e-9 * scale)
        assert np.all(np.abs(corr.samples - g[f"{prefix}.s{s}.corr_samples"]) <= 1e-8 * scale)


def test_autocorrelate_scalar_matches_the_reference():
    g = load_golden("scalar_drivers.npz")
    cats = _driver_catalogs(g, weights=True)
    cfs = yaw.autocorrelate_scalar(_driver_config(g), cats["ref"])
    assert len(cfs) == 2
    for s, cf in enumerate(cfs):
        assert type(cf) is yaw.ScalarCorrFunc and cf.dr is None and cf.auto
        _check_scalar_counts(f"auto.s{s}.dd", cf.dd, g, exact_nn=False)
    _check_samples("auto", cfs, g)
    cats["ref"].drop_layouts()


def test_crosscorrelate_scalar_without_randoms_matches_the_reference():
    g = load_golden("scalar_drivers.npz")
    cats = _driver_catalogs(g, weights=True)
    config = _driver_config(g)
    cfs = yaw.crosscorrelate_scalar(config, cats["ref"], cats["unk"])
    for s, cf in enumerate(cfs):
        _check_scalar_counts(f"cross.s{s}.dd", cf.dd, g, exact_nn=False)
        # DR = compute_scalar_normalisation: the sums of kappa * w and of w per (patch, bin), on the diagonal
        np.testing.assert_allclose(cf.dr.kappa_counts.counts, g[f"cross.s{s}.dr.kappa_counts"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(cf.dr.number_counts.counts, g[f"cross.s{s}.dr.number_counts"], rtol=1e-12, atol=0)
        assert cf.dr is cfs[0].dr  # repeated per scale
    norm = yaw.compute_scalar_normalisation(cats["ref"], config.binning.binning)
    assert norm == cfs[0].dr  # the device sums are reproducible, bit for bit
    off = ~np.eye(8, dtype=bool)
    assert np.all(norm.kappa_counts.counts[:, off] == 0) and np.all(norm.number_counts.counts[:, off] == 0)
    assert np.count_nonzero(norm.kappa_counts.counts) == 4 * 8
    _check_samples("cross", cfs, g)
    for cat in cats.values():
        cat.drop_layouts()


def test_crosscorrelate_scalar_with_randoms_matches_the_reference():
    g = load_golden("scalar_drivers.npz")
    cats = _driver_catalogs(g, weights=False)
    cfs = yaw.crosscorrelate_scalar(_driver_config(g, closed="left", rweight=-1.0), cats["ref"], cats["unk"], unk_rand=cats["rnd"])
    for s, cf in enumerate(cfs):
        # unweighted input, but separation weights: the number counts are no integers -> the weighted tolerance
        _check_scalar_counts(f"cross_rand.s{s}.dd", cf.dd, g, exact_nn=False)
        _check_scalar_counts(f"cross_rand.s{s}.dr", cf.dr, g, exact_nn=False)
    _check_samples("cross_rand", cfs, g)
    # unweighted normalisation: object counts, exact
    norm = yaw.compute_scalar_normalisation(cats["ref"], cfs[0].binning)
    layout = cats["ref"]._active_layout
    assert np.array_equal(np.diagonal(norm.number_counts.counts, axis1=1, axis2=2), layout.segment_sizes().T.astype(np.float64))
    for cat in cats.values():
        cat.drop_layouts()


# --------------------------------------------------------------------------- the twin on the device
def _random_layout(rng, n, n_patches, n_bins, weighted):
    ra = np.deg2rad(rng.uniform(100.0, 104.0, n))
    dec = np.arcsin(rng.uniform(np.sin(np.deg2rad(30.0)), np.sin(np.deg2rad(34.0)), n))
    x, y, z = np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)
    seg = np.sort(rng.integers(0, n_patches * n_bins, n))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=n_patches * n_bins))]).astype(np.int64)
    w = rng.uniform(0.5, 1.5, n) if weighted else None
    return x, y, z, w, rng.normal(0.0, 1.0, n), offsets


@pytest.mark.parametrize("weighted", [False, True], ids=["u", "w"])
@pytest.mark.parametrize("sort_axis", [2, 0])
def test_twin_is_the_catalogue_of_the_host_product(weighted, sort_axis):
    """cat_k of yawhip_catalog_upload_scalar against a plain upload of numpy's kappa * w, cat_n against the plain upload of
    w: fine sums of yawhip_count_pairs bit for bit, the same device bytes, the same segment sums."""
    rng = np.random.default_rng(77 + sort_axis)
    P, B, n = 12, 3, 150_000
    x, y, z, w, kappa, offsets = _random_layout(rng, n, P, B, weighted)
    x2, y2, z2, w2, _, off2 = _random_layout(rng, n, P, 1, True)
    ctx = _lib.Context(0)
    try:
        cat_n, cat_k = _lib.DeviceCatalog.upload_scalar(ctx, x, y, z, w, kappa, P, B, offsets, sort_axis=sort_axis)
        product = kappa * w if weighted else kappa.copy()
        host_k = _lib.DeviceCatalog(ctx, x, y, z, product, P, B, offsets, sort_axis=sort_axis)
        host_n = _lib.DeviceCatalog(ctx, x, y, z, w, P, B, offsets, sort_axis=sort_axis)
        other = _lib.DeviceCatalog(ctx, x2, y2, z2, w2, P, 1, off2, sort_axis=sort_axis)
        assert cat_k.weighted and cat_n.weighted == weighted
        assert cat_k.device_bytes == host_k.device_bytes and cat_n.device_bytes == host_n.device_bytes
        jobs = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)
        t = np.tile(np.array([1e-8, 1.5e-7, 6e-7, 2.2e-6]), (B, 1))
        for a, b in ((cat_k, host_k), (cat_n, host_n)):
            for second in (other, None):  # against another catalogue, and against itself
                got = _lib.count_pairs(ctx, a, second or a, jobs, t, want_counts=True, want_sums=True)
                exp = _lib.count_pairs(ctx, b, second or b, jobs, t, want_counts=True, want_sums=True)
                assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
                assert got[0].sum() > 1e5 and got[2].candidate_pairs == exp[2].candidate_pairs
        # the two of one upload against each other (kn of an autocorrelation) = the two host uploads against each other
        got = _lib.count_pairs(ctx, cat_k, cat_n, jobs, t, want_sums=True)
        exp = _lib.count_pairs(ctx, host_k, host_n, jobs, t, want_sums=True)
        assert np.array_equal(got[1], exp[1]) and np.any(got[1] < 0)
        # segment sums: reproducible, equal for twin and host product, numpy's to rounding
        sums_k = cat_k.segment_sums()
        assert np.array_equal(sums_k, host_k.segment_sums()) and np.array_equal(sums_k, cat_k.segment_sums())
        sums_n = cat_n.segment_sums()
        for got_sums, col in ((sums_k, product), (sums_n, w)):
            for s in range(P * B):
                lo, hi = offsets[s], offsets[s + 1]
                if col is None:
                    assert got_sums.ravel()[s] == hi - lo
                else:
                    assert abs(got_sums.ravel()[s] - col[lo:hi].sum()) <= 1e-12 * np.abs(col[lo:hi]).sum()
        # each is freed on its own; the other keeps counting
        cat_n.free()
        again = _lib.count_pairs(ctx, cat_k, other, jobs, t, want_sums=True)
        exp = _lib.count_pairs(ctx, host_k, other, jobs, t, want_sums=True)
        assert np.array_equal(again[1], exp[1])
    finally:
        ctx.close()


def test_catalogue_without_kappa_uploads_as_before():
    """No kappa: one device catalogue per layout, no twin, the bytes a plain upload reports."""
    g = load_golden("scalar_drivers.npz")
    centers = yaw.AngularCoordinates(g["patch_centers"])
    frame = {k.split(".", 1)[1]: g[k] for k in g.files if k.startswith("ref.")}
    kw = dict(ra_name="ra", dec_name="dec", weight_name="w", redshift_name="z", patch_centers=centers)
    plain, with_kappa = yaw.Catalog.from_dataframe(None, frame, **kw), yaw.Catalog.from_dataframe(None, frame, kappa_name="kappa", **kw)
    config = _driver_config(g)
    for cat in (plain, with_kappa):
        cat.build_trees(config.binning.edges, closed="right")
    links = yaw.PatchLinkage.from_catalogs(config, plain)
    a, b = links.count_pairs(plain), links.count_pairs(with_kappa)
    assert all(x == y for x, y in zip(a, b))  # "nn" does not see the kappa column
    ctx = engine.get_context()
    lp, lk = plain._active_layout, with_kappa._active_layout
    assert lp.twin is None and list(lp.device) == [id(ctx)]
    assert lk.device[id(ctx)].device_bytes == lp.device[id(ctx)].device_bytes
    # the twin is a catalogue like any other: the strip layout of the sort axis is built at upload, those of further
    # orientations on first use, so it weighs what the plain (weighted) one does once it has served the same count
    twin = lk.twin.device[id(ctx)]
    links.count_pairs(with_kappa, mode="kk")
    assert twin is lk.twin.device[id(ctx)] and twin.device_bytes == lp.device[id(ctx)].device_bytes
    with_kappa.drop_layouts()
    assert not twin._h and not lk.twin.device  # the twin goes with the layouts
    plain.drop_layouts()


def test_multi_device_context_replicates_both(monkeypatch):
    """A context of several devices (the one GPU listed twice) replicates the plain catalogue and its twin."""
    g = load_golden("scalar_drivers.npz")
    cats = _driver_catalogs(g, weights=True)
    config = _driver_config(g)
    single = yaw.autocorrelate_scalar(config, cats["ref"])
    cats["ref"].drop_layouts()
    monkeypatch.setenv("YAW_AMD_DEVICES", "0,0")  # (restored to what it was when the test ends)
    multi = yaw.autocorrelate_scalar(config, cats["ref"])
    assert all(a == b for a, b in zip(single, multi))
    cats["ref"].drop_layouts()


# --------------------------------------------------------------------------- exact sums through the API
def _dyadic_catalogs():
    """The positions of the count-variant table's ``c1`` (binned, 17 033 objects) and ``c2u`` (27 258, with the partners at
    the bin edges and the clump) in 1.5 x 1.5 deg, cut into four strips of right ascension (the table's own patch 3 holds no
    ``c1`` object, and a catalogue takes no empty patch). Weights ``m / 16`` with m in [1, 64], kappa ``m / 16`` with m in
    [-64, 64]: ``kappa * w`` is a multiple of 2^-8 of magnitude at most 16, a product of two of them a multiple of 2^-16 of at
    most 2^8, and the catalogues hold fewer than 2^29 pairs -- every float64 sum of such products is exact in any order."""
    import test_gpu_count_variants as table
    from oracle import oracle

    cats = table._catalogues()[0]
    rng = np.random.default_rng(20261023)
    zedges = np.linspace(0.1, 0.9, table.B + 1)
    centers = yaw.AngularCoordinates(np.deg2rad([[30.1875, 0.0], [30.5625, 0.0], [30.9375, 0.0], [31.3125, 0.0]]))
    out = []
    for name in ("c1", "c2u"):
        cat = cats[name]
        n = len(cat["x"])
        ra, dec = oracle.from_3d(cat["x"], cat["y"], cat["z"])
        frame = dict(ra=np.rad2deg(ra), dec=np.rad2deg(dec), w=rng.integers(1, 65, n) / 16.0, kappa=rng.integers(-64, 65, n) / 16.0)
        if cat["nb"] > 1:  # the redshift bin of the table's segment, at the middle of the bin
            k = np.repeat(np.arange(len(cat["off"]) - 1) % cat["nb"], np.diff(cat["off"]))
            frame["z"] = 0.5 * (zedges[k] + zedges[k + 1])
        out.append(yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", weight_name="w", kappa_name="kappa",
                                              redshift_name="z" if "z" in frame else None, patch_centers=centers))
    assert 17033 * 27258 < 2 ** 29
    return (*out, zedges)


def test_scalar_modes_are_exact_on_dyadic_input(monkeypatch):
    """``kappa * w`` through the API on catalogues large enough for the kernels production runs (a band or merged-sweep
    variant, not the brute-force ``k_count``): with exactly summable input the counts of every mode equal, bit for bit, the
    same calls made on the CPU oracle -- the kernel's sums, the halving of an autocorrelation's diagonal jobs, the per-scale
    sums and the scatter are all exact."""
    one, two, zedges = _dyadic_catalogs()
    config = yaw.Configuration.create(rmin=[1.0, 2.0], rmax=[3.5, 6.0], unit="arcmin", edges=zedges, closed="right")
    one.build_trees(config.binning.edges, closed="right")
    two.build_trees(None)
    links = yaw.PatchLinkage.from_catalogs(config, one, two)
    calls = {**{mode: ((one, two), mode) for mode in ("kn", "nk", "kk")}, "auto kk": ((one,), "kk")}

    def production_kernel(stats):
        names = stats.variants
        return bool(names) and all(v.startswith(("k_count_band", "k_count_merged")) for v in names)

    def run(check_variants):
        out = {}
        for key, (cats, mode) in calls.items():
            out[key] = np.stack([c.counts.counts for c in links.count_pairs(*cats, mode=mode)])
            if check_variants:
                print(f"{key}: {sorted(links.last_stats.variants)}")
                assert production_kernel(links.last_stats), (key, links.last_stats.variants)
                assert links.last_stats.count_variant == 0  # the sums alone: the weighted instantiation
        dd = links.count_scalar_pairs(one, two, mode="kk", count_type_info="DD")
        out["scalar kk"] = np.stack([c.kappa_counts.counts for c in dd])
        out["scalar nn"] = np.stack([c.number_counts.counts for c in dd])
        if check_variants:
            assert sorted(links.last_batch_stats) == ["DD (kk)", "DD (nn)"]
            assert all(production_kernel(st) for st in links.last_batch_stats.values()), links.last_batch_stats
        return out

    got = run(True)
    with monkeypatch.context() as patch:
        helpers.use_oracle_engine(patch)
        exp = run(False)
    assert sorted(got) == sorted(exp) and len(got) == 6
    for key in got:
        assert got[key].shape == exp[key].shape and np.any(exp[key] != 0), key
        differ = np.count_nonzero(got[key] != exp[key])
        assert np.array_equal(got[key], exp[key]), (key, differ)
        if key != "scalar nn":
            assert np.any(exp[key] < 0) and np.any(exp[key] > 0), key
    assert np.array_equal(got["scalar kk"], got["kk"])
    # the diagonal jobs of the autocorrelation hold pairs, counted once
    assert np.any(np.diagonal(exp["auto kk"], axis1=2, axis2=3) != 0)
    one.drop_layouts()
    two.drop_layouts()


# --------------------------------------------------------------------------- submissions
def test_scalar_counts_are_one_submission_and_equal_single_calls(monkeypatch):
    g = load_golden("scalar_drivers.npz")
    cats = _driver_catalogs(g, weights=True)
    config = _driver_config(g)
    calls = []
    real = _lib.count_pairs_dense_batch

    def counting(ctx, requests, *args, **kwargs):
        calls.append(len(requests))
        return real(ctx, requests, *args, **kwargs)

    monkeypatch.setattr(_lib, "count_pairs_dense_batch", counting)
    ref, unk, rnd = cats["ref"], cats["unk"], cats["rnd"]
    ref.build_trees(config.binning.edges, closed="right")
    unk.build_trees(None)
    rnd.build_trees(None)
    links = yaw.PatchLinkage.from_catalogs(config, ref, unk, rnd)
    # DD of an autocorrelation: one batch call holding two requests
    dd = links.count_scalar_pairs(ref, mode="kk", count_type_info="DD")
    assert calls == [2] and sorted(links.last_batch_stats) == ["DD (kk)", "DD (nn)"]
    assert all(st.n_launches > 0 and st.candidate_pairs > 0 for st in links.last_batch_stats.values())
    assert links.last_batch_stats["DD (kk)"].count_variant_weighted != 0  # the κ side makes it a weighted count
    # ... equal to two single calls, bit for bit
    kk, nn = links.count_pairs(ref, mode="kk"), links.count_pairs(ref, mode="nn")
    assert calls == [2]
    for s in range(2):
        assert np.array_equal(dd[s].kappa_counts.counts, kk[s].counts.counts)
        assert np.array_equal(dd[s].number_counts.counts, nn[s].counts.counts)
        assert dd[s].kappa_counts == kk[s].counts and dd[s].number_counts == nn[s].counts
    # DD + DR of a cross-correlation: one batch call holding four
    del calls[:]
    cfs = yaw.crosscorrelate_scalar(config, ref, unk, unk_rand=rnd)
    assert calls == [4]
    singles = links.count_pairs(ref, rnd, mode="kn")
    assert all(np.array_equal(cf.dr.kappa_counts.counts, one.counts.counts) for cf, one in zip(cfs, singles))
    # a batch request may carry a mode
    del calls[:]
    out = links.count_pairs_batch([((ref, unk), "a", "kn"), ((ref, unk), "b"), ((ref, unk), "c", "nn")])
    assert calls == [3] and all(x.counts == y.counts for x, y in zip(out[1], out[2]))
    assert all(np.array_equal(x.counts.counts, cf.dd.kappa_counts.counts) for x, cf in zip(out[0], cfs))
    for cat in cats.values():
        cat.drop_layouts()
