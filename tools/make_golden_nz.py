#!/usr/bin/env python3
"""Generate the redshift-histogram and result-file fixtures under ``tests/golden/`` by RUNNING THE REFERENCE.

Runs only where the reference is present (``tools/ref_loader.py``, one worker: the reference's ``iter_unordered`` may
reorder the rows of the per-patch histogram otherwise). The outputs are pure data: inputs and the reference's results.

  histdata_edges.npz     a synthetic catalogue with given patch ids whose redshifts sit on e[0], on interior edges and
                         on e[B] of every binning (and outside them), with the reference's HistData (data, samples and
                         per-patch counts) for closed left / right x linear / irregular / single-bin binnings, with and
                         without weights; case names in ``cases``
  histdata_refcache.npz  HistData of the reference-written cache tests/golden/refcache (weights, redshifts), two binnings
  histdata_2dflens.npz   HistData of the 2dFLenS reference sample held by twodflens.npz, with its patch assignment
  result_files/          the .dat / .smp / .cov files the reference's to_files writes for a CorrData, a RedshiftData and a
                         HistData built from the full-precision arrays in inputs.npz (NaN values, both closed sides),
                         and in expected.npz what its from_files reads back from each and its normalised() outputs

Running it again reproduces every file byte for byte (npz members are written with a fixed time stamp).

Usage:  python tools/make_golden_nz.py
"""
from __future__ import annotations

import io
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_loader import load_reference  # noqa: E402

yaw = load_reference()
import pandas as pd  # noqa: E402
from yaw.redshifts import _redshift_histogram  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


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


def binning_config(edges, closed):
    return yaw.config.BinningConfig.create(edges=np.asarray(edges), closed=closed)


def histogram(cat, edges, closed):
    """The reference's HistData and the per-patch counts its worker function returns, in patch order."""
    hist = yaw.HistData.from_catalog(cat, binning_config(edges, closed), max_workers=1)
    binning = yaw.Binning(np.asarray(edges), closed=closed)
    counts = np.array([_redshift_histogram(cat[pid], binning) for pid in sorted(cat.keys())])
    return hist, counts


# --------------------------------------------------------------------------- histdata_edges.npz
EDGE_BINNINGS = {
    "linear": np.linspace(0.1, 1.0, 10),
    "irregular": np.array([0.05, 0.1, 0.13, 0.3, 0.31, 0.5, 0.9, 1.2]),
    "single": np.array([0.2, 0.8]),
}


def make_edges(tmp):
    rng = np.random.default_rng(20261016)
    n_patches = 6
    on_edges = np.concatenate(list(EDGE_BINNINGS.values()))
    z = np.concatenate([
        np.repeat(on_edges, 7),                    # every edge of every binning, seven times
        rng.uniform(0.0, 1.4, 1500),               # spread over and beyond all binnings
        np.array([-0.5, -0.0, 0.0, 1.5, 2.0, 0.049999999, 1.2000000001]),  # outside every binning
    ])
    n = len(z)
    order = rng.permutation(n)
    z = z[order]
    patch = rng.integers(0, n_patches, n).astype(np.int32)
    patch[:n_patches] = np.arange(n_patches)       # no empty patch (the reference rejects them)
    ra = rng.uniform(0.0, 360.0, n)
    dec = rng.uniform(-30.0, 30.0, n)
    w = rng.uniform(0.25, 2.0, n)
    df = pd.DataFrame(dict(ra=ra, dec=dec, z=z, w=w, patch=patch))
    out = dict(ra=ra, dec=dec, z=z, w=w, patch=patch)
    cases = []
    for weighted in (False, True):
        kw = dict(ra_name="ra", dec_name="dec", redshift_name="z", patch_name="patch")
        if weighted:
            kw["weight_name"] = "w"
        cat = yaw.Catalog.from_dataframe(os.path.join(tmp, f"edges_{int(weighted)}"), df, overwrite=True, **kw)
        for name, edges in EDGE_BINNINGS.items():
            for closed in ("left", "right"):
                case = f"{name}_{closed}_{'w' if weighted else 'n'}"
                hist, counts = histogram(cat, edges, closed)
                out[f"{case}.edges"] = edges
                out[f"{case}.closed"] = np.array(closed)
                out[f"{case}.weighted"] = np.array(weighted)
                out[f"{case}.data"] = hist.data
                out[f"{case}.samples"] = hist.samples
                out[f"{case}.counts"] = counts
                cases.append(case)
    out["cases"] = np.array(cases)
    save("histdata_edges.npz", **out)


# --------------------------------------------------------------------------- histdata_refcache.npz
REFCACHE_BINNINGS = {
    "linear_right": (np.linspace(0.05, 1.05, 21), "right"),
    "irregular_left": (np.array([0.0, 0.15, 0.2, 0.45, 0.5, 0.75, 1.5]), "left"),
}


def make_refcache(tmp):
    cache = os.path.join(tmp, "refcache_copy")
    shutil.copytree(os.path.join(OUT, "refcache"), cache)
    cat = yaw.Catalog(cache)
    out, cases = {}, []
    for case, (edges, closed) in REFCACHE_BINNINGS.items():
        hist, counts = histogram(cat, edges, closed)
        out[f"{case}.edges"] = edges
        out[f"{case}.closed"] = np.array(closed)
        out[f"{case}.data"] = hist.data
        out[f"{case}.samples"] = hist.samples
        out[f"{case}.counts"] = counts
        cases.append(case)
    out["cases"] = np.array(cases)
    save("histdata_refcache.npz", **out)


# --------------------------------------------------------------------------- histdata_2dflens.npz
def make_2dflens(tmp):
    src = np.load(os.path.join(OUT, "twodflens.npz"))
    df = pd.DataFrame({"ra": src["data.RA"], "dec": src["data.Dec"], "z": src["data.redshift"], "w": src["data.wei"],
                       "patch": src["data.patch"]})
    cat = yaw.Catalog.from_dataframe(os.path.join(tmp, "twodflens"), df, ra_name="ra", dec_name="dec", redshift_name="z",
                                     weight_name="w", patch_name="patch", overwrite=True)
    edges = src["zedges"]
    out = {"edges": edges}
    for closed in ("right", "left"):
        hist, counts = histogram(cat, edges, closed)
        out[f"{closed}.data"] = hist.data
        out[f"{closed}.samples"] = hist.samples
        out[f"{closed}.counts"] = counts
    save("histdata_2dflens.npz", **out)


# --------------------------------------------------------------------------- result_files/
def make_result_files():
    rng = np.random.default_rng(7)
    dest = os.path.join(OUT, "result_files")
    os.makedirs(dest, exist_ok=True)
    edges_right = np.linspace(0.07, 1.43, 9)               # CorrData: closed right
    edges_left = np.array([0.0, 0.1, 0.25, 0.3, 0.55, 0.6, 0.95, 1.3, 2.0])  # RedshiftData, HistData: closed left
    n_samples = 5
    corr_data = rng.normal(0.0, 0.05, 8)
    corr_data[3] = np.nan
    corr_samples = corr_data + rng.normal(0.0, 0.01, (n_samples, 8))
    corr_samples[2, 5] = np.nan
    nz_data = np.abs(rng.normal(1.2, 0.8, 8)) * np.array([1.0, 1e3, 1.0, -1.0, 1e-7, 1.0, 12345.678, 1.0])
    nz_data[6] = np.nan
    nz_samples = nz_data * (1.0 + rng.normal(0.0, 0.05, (n_samples, 8)))
    hist_counts = rng.integers(0, 5000, (n_samples, 8)).astype(np.float64) * rng.uniform(0.5, 1.5, (n_samples, 8))
    hist_data = hist_counts.sum(axis=0)
    hist_samples = hist_data - hist_counts
    inputs = dict(edges_right=edges_right, edges_left=edges_left, corr_data=corr_data, corr_samples=corr_samples,
                  nz_data=nz_data, nz_samples=nz_samples, hist_data=hist_data, hist_samples=hist_samples)
    cases = {
        "corrdata": yaw.CorrData(yaw.Binning(edges_right, closed="right"), corr_data, corr_samples),
        "redshiftdata": yaw.RedshiftData(yaw.Binning(edges_left, closed="left"), nz_data, nz_samples),
        "histdata": yaw.HistData(yaw.Binning(edges_left, closed="left"), hist_data, hist_samples),
    }
    expected = {}
    for name, obj in cases.items():
        obj.to_files(os.path.join(dest, name))
        back = type(obj).from_files(os.path.join(dest, name))
        expected[f"{name}.edges"] = back.binning.edges
        expected[f"{name}.closed"] = np.array(str(back.binning.closed))
        expected[f"{name}.data"] = back.data
        expected[f"{name}.samples"] = back.samples
    norm_hist = cases["histdata"].normalised()
    norm_nz = cases["redshiftdata"].normalised()
    norm_nz_target = cases["redshiftdata"].normalised(target=norm_hist)
    for key, obj in (("norm_hist", norm_hist), ("norm_nz", norm_nz), ("norm_nz_target", norm_nz_target)):
        expected[f"{key}.data"] = obj.data
        expected[f"{key}.samples"] = obj.samples
    save(os.path.join("result_files", "inputs.npz"), **inputs)
    save(os.path.join("result_files", "expected.npz"), **expected)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        make_edges(tmp)
        make_refcache(tmp)
        make_2dflens(tmp)
    make_result_files()


if __name__ == "__main__":
    main()
