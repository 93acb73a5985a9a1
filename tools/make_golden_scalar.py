#!/usr/bin/env python3
"""Generate the scalar-field ("kappa") fixtures under ``tests/golden/`` by RUNNING THE REFERENCE.

Runs only where the reference is present (``tools/ref_loader.py``, one worker). The outputs are pure data: inputs and the
reference's results. kappa is drawn with both signs and a mean near zero, so the signed sums cancel for real; next to every
signed tensor the same count with ``|kappa|`` in the place of ``kappa`` is stored (``abs_counts``): the cancellation-free
magnitude the GPU tests measure their error against.

  scalar_seam.npz      two catalogues of two patches each (binned with redshifts on bin edges / unbinned), and for every
                       combination of mode (nn, nk, kn, kk) x weights (on, off) x rweight (None, -1) x closed (left, right),
                       two scales: ``AngularTree.count(mode=...)`` for every redshift bin of all four patch pairs, called
                       as ``process_patch_pair`` calls it but on trees loaded afresh for EVERY count (see
                       ``count_patch_pair``), ``counts[S, B, 2, 2]``, and ``abs_counts`` of the same shape; case names in
                       ``cases``
  scalar_drivers.npz   8-patch ``autocorrelate_scalar`` (weighted), ``crosscorrelate_scalar`` without randoms (weighted) and
                       with ``unk_rand`` (unweighted, closed left, rweight -1): per scale the ``kappa_counts`` /
                       ``number_counts`` tensors of dd (and dr), their ``abs_counts``, ``sample_patch_sum`` of each and
                       ``ScalarCorrFunc.sample()`` data and samples
  scalar_cache.npz     the frame of the cache fixtures, what the reference reads back from ``refcache_kappa/`` and from a
                       cache THIS package wrote from the same frame
  refcache_kappa/      a cache the reference wrote from that frame (weights, redshifts, kappa)

Running it again reproduces every file byte for byte (npz members are written with a fixed time stamp).

Usage:  python tools/make_golden_scalar.py
"""
from __future__ import annotations

import io
import os
import shutil
import sys
import tempfile
import zipfile
from itertools import islice

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_loader import load_reference  # noqa: E402

yaw = load_reference()
import pandas as pd  # noqa: E402
from yaw.coordinates import AngularCoordinates  # noqa: E402
from yaw.catalog.trees import BinnedTrees  # noqa: E402
from yaw.correlation import measurements as rmeas  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
ZEDGES = np.array([0.1, 0.3, 0.55, 0.8, 1.0])


def save(name, **arrays):
    """np.savez_compressed with a fixed member time stamp, so that the file is a function of the arrays alone."""
    path = os.path.join(OUT, name)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


def draw_frame(rng, n, ra0, ra1, dec0, dec1, *, redshifts):
    """ra / dec uniform on the sphere inside a box, weights, kappa ~ N(0, 1) and, if asked, redshifts with a share on edges."""
    ra = rng.uniform(ra0, ra1, n)
    dec = np.rad2deg(np.arcsin(rng.uniform(np.sin(np.deg2rad(dec0)), np.sin(np.deg2rad(dec1)), n)))
    cols = dict(ra=ra, dec=dec, w=rng.uniform(0.5, 1.5, n), kappa=rng.normal(0.0, 1.0, n))
    if redshifts:
        z = rng.uniform(0.05, 1.05, n)  # some objects fall outside the binning
        on_edge = rng.random(n) < 0.15
        z[on_edge] = rng.choice(ZEDGES, on_edge.sum())  # closed-side cases
        cols["z"] = z
    return cols


def grid_centers(ra0, ra1, dec0, dec1, nra, ndec):
    ras = ra0 + (np.arange(nra) + 0.5) * (ra1 - ra0) / nra
    decs = dec0 + (np.arange(ndec) + 0.5) * (dec1 - dec0) / ndec
    rr, dd = np.meshgrid(ras, decs)
    return np.deg2rad(np.column_stack([rr.ravel(), dd.ravel()]))


class Catalogs:
    """Reference catalogues of one frame under a temporary directory, a fresh cache directory for each."""

    def __init__(self, tmp, centers):
        self.tmp, self.centers, self.count = tmp, AngularCoordinates(centers), 0

    def __call__(self, cols, *, weights, kappa, absolute=False):
        self.count += 1
        frame = dict(cols)
        if absolute and kappa:
            frame["kappa"] = np.abs(frame["kappa"])
        return yaw.Catalog.from_dataframe(
            os.path.join(self.tmp, f"cat_{self.count}"), pd.DataFrame(frame), ra_name="ra", dec_name="dec",
            weight_name="w" if weights else None, redshift_name="z" if "z" in frame else None,
            kappa_name="kappa" if kappa else None, patch_centers=self.centers, overwrite=True)


# --------------------------------------------------------------------------- scalar_seam.npz
def count_patch_pair(patch1, patch2, config, mode):
    """The loop of ``process_patch_pair`` (measurements.py:99-122) around ``AngularTree.count``, with the trees of both
    patches loaded afresh from their cache for every count. The reference's ``get_pair_weights`` multiplies ``tree.kappa`` by
    the weights in place (trees.py:278-282), and an unbinned patch hands the SAME tree object to every bin: inside one
    ``process_patch_pair`` a weighted "k" side without redshifts would carry ``kappa * w**(bin + 1)``. A fresh tree per
    count carries ``kappa * w``, the documented weight. -> counts[S, B]"""
    zmids = config.binning.binning.mids
    out = np.empty((config.scales.num_scales, len(zmids)))
    for i, zmid in enumerate(zmids):
        tree1 = next(islice(iter(BinnedTrees(patch1)), i, None))
        tree2 = next(islice(iter(BinnedTrees(patch2)), i, None))
        ang_min, ang_max = config.scales.scales.get_angle_radian(zmid, cosmology=config.cosmology)
        out[:, i] = tree1.count(tree2, ang_min, ang_max, weight_scale=config.scales.rweight,
                                weight_res=config.scales.resolution, mode=mode)
    return out


def make_seam(tmp):
    rng = np.random.default_rng(20261017)
    box = (20.0, 21.2, -10.0, -9.4)
    centers = grid_centers(*box, 2, 1)
    one = draw_frame(rng, 1300, *box, redshifts=True)
    two = draw_frame(rng, 1700, *box, redshifts=False)
    out = {f"one.{k}": v for k, v in one.items()}
    out.update({f"two.{k}": v for k, v in two.items()})
    out["patch_centers"], out["zedges"] = centers, ZEDGES
    out["rmin"], out["rmax"] = np.array([1.0, 4.0]), np.array([8.0, 20.0])  # arcmin
    make = Catalogs(tmp, centers)
    cases = []
    for weighted in (False, True):
        for closed in ("left", "right"):
            for rweight in (None, -1.0):
                config = yaw.Configuration.create(rmin=out["rmin"], rmax=out["rmax"], unit="arcmin", rweight=rweight,
                                                  resolution=12 if rweight is not None else None, edges=ZEDGES, closed=closed)
                for mode in ("nn", "nk", "kn", "kk"):
                    tensors = {}
                    for name, absolute in (("counts", False), ("abs_counts", True)):
                        cat1 = make(one, weights=weighted, kappa=True, absolute=absolute)
                        cat2 = make(two, weights=weighted, kappa=True, absolute=absolute)
                        cat1.build_trees(ZEDGES, closed=closed, max_workers=1)
                        cat2.build_trees(None, max_workers=1)
                        dense = np.zeros((2, len(ZEDGES) - 1, 2, 2))
                        for i in range(2):
                            for j in range(2):
                                dense[:, :, i, j] = count_patch_pair(cat1[i], cat2[j], config, mode)
                                if mode in ("nn", "kn") or not weighted:  # (no repeated in-place product: the caller agrees)
                                    res = rmeas.process_patch_pair(rmeas.PatchPair(i, j, cat1[i], cat2[j]), config, mode=mode)
                                    assert np.array_equal(res.counts, dense[:, :, i, j])
                        tensors[name] = dense
                    case = f"{mode}.{'w' if weighted else 'u'}.{closed}.{'plain' if rweight is None else 'rw-1'}"
                    out[f"{case}.counts"], out[f"{case}.abs_counts"] = tensors["counts"], tensors["abs_counts"]
                    cases.append(case)
    out["cases"] = np.array(cases)
    save("scalar_seam.npz", **out)


# --------------------------------------------------------------------------- scalar_drivers.npz
def dump_scalar(prefix, corrfuncs, abs_corrfuncs, out):
    for s, (cf, cf_abs) in enumerate(zip(corrfuncs, abs_corrfuncs)):
        for kind in ("dd", "dr"):
            counts, counts_abs = getattr(cf, kind), getattr(cf_abs, kind)
            if counts is None:
                continue
            key = f"{prefix}.s{s}.{kind}"
            out[f"{key}.kappa_counts"] = counts.kappa_counts.counts
            out[f"{key}.number_counts"] = counts.number_counts.counts
            out[f"{key}.abs_counts"] = counts_abs.kappa_counts.counts
            sampled = counts.sample_patch_sum()
            out[f"{key}.sample_data"], out[f"{key}.sample_samples"] = sampled.data, sampled.samples
        corr = cf.sample()
        out[f"{prefix}.s{s}.corr_data"], out[f"{prefix}.s{s}.corr_samples"] = corr.data, corr.samples


def make_drivers(tmp):
    rng = np.random.default_rng(20261018)
    box = (30.0, 34.0, 5.0, 7.0)
    centers = grid_centers(*box, 4, 2)
    ref = draw_frame(rng, 1500, *box, redshifts=True)
    unk = draw_frame(rng, 1800, *box, redshifts=False)
    rnd = draw_frame(rng, 2500, *box, redshifts=False)
    del unk["kappa"], rnd["kappa"], rnd["w"]  # (columns no case reads)
    out = {f"{name}.{k}": v for name, cols in (("ref", ref), ("unk", unk), ("rnd", rnd)) for k, v in cols.items()}
    out["patch_centers"], out["zedges"] = centers, ZEDGES
    out["rmin"], out["rmax"] = np.array([2.0, 5.0]), np.array([20.0, 40.0])  # arcmin
    make = Catalogs(tmp, centers)
    kw = dict(rmin=out["rmin"], rmax=out["rmax"], unit="arcmin", edges=ZEDGES)
    plain = yaw.Configuration.create(closed="right", **kw)
    weighted_sep = yaw.Configuration.create(closed="left", rweight=-1.0, resolution=12, **kw)

    def both(run):
        return run(False), run(True)

    auto = both(lambda a: rmeas.autocorrelate_scalar(plain, make(ref, weights=True, kappa=True, absolute=a), max_workers=1))
    dump_scalar("auto", *auto, out)
    cross = both(lambda a: rmeas.crosscorrelate_scalar(plain, make(ref, weights=True, kappa=True, absolute=a),
                                                       make(unk, weights=True, kappa=False), max_workers=1))
    dump_scalar("cross", *cross, out)
    cross_rand = both(lambda a: rmeas.crosscorrelate_scalar(
        weighted_sep, make(ref, weights=False, kappa=True, absolute=a), make(unk, weights=False, kappa=False),
        unk_rand=make(rnd, weights=False, kappa=False), max_workers=1))
    dump_scalar("cross_rand", *cross_rand, out)
    save("scalar_drivers.npz", **out)


# --------------------------------------------------------------------------- scalar_cache.npz, refcache_kappa/
def read_back(cat, prefix, out):
    out[f"{prefix}.flags"] = np.array([cat.has_weights, cat.has_redshifts, cat[0].has_kappa])
    out[f"{prefix}.num_records"] = np.array(cat.get_num_records())
    for pid in range(cat.num_patches):
        patch = cat[pid]
        out[f"{prefix}.patch_{pid}.records"] = np.column_stack(
            [patch.coords.ra, patch.coords.dec, patch.weights, patch.redshifts, patch.kappa])


def make_cache(tmp):
    sys.path.insert(0, os.path.dirname(HERE))
    import yet_another_wizz_amd as ours

    rng = np.random.default_rng(20261019)
    box = (50.0, 52.0, -2.0, -1.0)
    centers = grid_centers(*box, 3, 1)
    frame = draw_frame(rng, 90, *box, redshifts=True)
    out = {f"input.{k}": v for k, v in frame.items()}
    out["patch_centers"] = centers
    kw = dict(ra_name="ra", dec_name="dec", weight_name="w", redshift_name="z", kappa_name="kappa")
    theirs = os.path.join(tmp, "refcache_kappa")
    yaw.Catalog.from_dataframe(theirs, pd.DataFrame(frame), patch_centers=AngularCoordinates(centers), overwrite=True, **kw)
    dest = os.path.join(OUT, "refcache_kappa")
    shutil.rmtree(dest, ignore_errors=True)
    shutil.copytree(theirs, dest)
    read_back(yaw.Catalog(theirs), "reference_cache", out)
    mine = os.path.join(tmp, "ourcache_kappa")
    ours.Catalog.from_dataframe(mine, frame, patch_centers=ours.AngularCoordinates(centers), **kw)
    read_back(yaw.Catalog(mine), "our_cache", out)
    save("scalar_cache.npz", **out)
    print("refcache_kappa files:", sorted(os.listdir(dest)), sorted(os.listdir(os.path.join(dest, "patch_0"))))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        make_cache(tmp)
        make_seam(tmp)
        make_drivers(tmp)


if __name__ == "__main__":
    main()
