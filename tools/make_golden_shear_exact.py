#!/usr/bin/env python3
"""Generate ``tests/golden/shear_exact.npz``: an exact reference of the four shear counts (``yawhip_shear_count``,
``yawhip_dsigma_count``, ``yawhip_shear_auto_count``, ``yawhip_shear_pair_count``) at separations of 0.4 to 36 arcseconds.

Runs on the CPU with ``mpmath`` at 50 digits; no GPU, no reference package. Nothing here restates the contract's algebra
(``a = x ly - y lx`` ... of include/yawhip.h): per pair the tool takes the float64 ``(ra, dec)`` the scene was built from and
computes the position angle of the partner by the bearing of spherical trigonometry (the formula of
``tests/shear_oracle.position_angle``), ``cos`` and ``sin`` of twice that angle, the exact chord^2 for membership and the exact
pair terms; ``wg = w * g`` are the rounded float64 products a handle stores, ``f, c, u`` the float64 columns. The sums of a cell
are rounded to float64 once, at the end.

Scenes (a few thousand pairs in all; a site is a patch of its own):
  sites   dec 0, dec 60, dec +89.99, dec -89.99 degrees, and one at ra = 2 pi - 1e-7 whose partners fall on both sides of the
          wrap of the right ascension
  tan     30 lenses inside 1" of every site in two redshift bins, 14 sources per site on rings of 0.5" ... 30" (log-uniform);
          two rows of 6 log-spaced fine bins, 0.4" ... 32" and 0.45" ... 36"; random weights and shears; jobs (p, p) and two
          jobs between sites, which hold nothing
  ds      the same objects with columns f, c, u drawn so that about half the pairs have the source in front
  pat     one lens, 200 sources whose (g1, g2) are the exact tangential pattern of amplitude ``pat.amplitude`` around it,
          rounded to float64: T / W = amplitude, X = 0
  cat     the sites as objects of one catalogue in two redshift bins, the second drawn around a centre 10" away; the site at
          the wrap is two patches, one on either side of it. ``auto``: the jobs of the auto count; ``one``: a cell list of the
          pair count on one handle (same-bin diagonal and cross-patch cells, cross-bin cells, both rows); ``two``: a cell list
          between the catalogue and a twin at the same positions with other weights and shears (``catb``)

Per cell the file holds the exact sums, ``A`` (the cancellation-free magnitude of the oracles) and ``A_theta`` (the same sum with
every pair divided by its separation in radian), and per member pair the exact terms rounded to float64 (``*.pairs``,
``*.pair_*``): tests/test_shear_exact_fixture.py re-derives every 7th of them with the functions below.

Two conditions are asserted; the inputs are redrawn until they hold, so that no pair is left out of any comparison: no pair's
exact chord^2 lies within a relative 1e-6 of any edge, and no pair of ``ds`` has ``|1 - c u| < 1e-6``.

``K`` of the tolerance (tests/shear_exact.py) is measured here: the worst ``|oracle - exact| / (eps A_theta)`` of the four numpy
oracles over the whole file, times four, rounded up to a power of two. It goes into the file and into DESIGN.md (between the
``shear-exact-K`` markers).

Running it again reproduces the file byte for byte (fixed seed; npz members are written with a fixed time stamp).

Usage:  python tools/make_golden_shear_exact.py
"""
from __future__ import annotations

import io
import os
import re
import sys
import zipfile

import mpmath
import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

OUT = os.path.join(ROOT, "tests", "golden", "shear_exact.npz")
DESIGN = os.path.join(ROOT, "DESIGN.md")
mp.dps = 50
SEED = 20261019
ARCSEC = np.pi / 180.0 / 3600.0
DEG = np.pi / 180.0
SITES = [(1.0, 0.0), (2.1, 60.0 * DEG), (3.3, 89.99 * DEG), (4.4, -89.99 * DEG), (2.0 * np.pi - 1e-7, 0.5)]
WRAP_SITE = 4
N_LENS, N_SRC, N_PER_BIN, N_PATTERN = 30, 14, 10, 200
EDGE_MARGIN, CLIP_MARGIN = 1e-6, 1e-6
AMPLITUDE = 0.03


def save(path, arrays):
    """np.savez_compressed with a fixed member time stamp, so that the file is a function of the arrays alone."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


def thresholds():
    rows = np.array([np.geomspace(0.4, 32.0, 7), np.geomspace(0.45, 36.0, 7)]) * ARCSEC
    return (2.0 * np.sin(0.5 * rows)) ** 2


# --------------------------------------------------------------------------- exact arithmetic
class Point:
    """A float64 (ra, dec) with its sines and cosines at the working precision."""

    __slots__ = ("ra", "sd", "cd", "x", "y", "z")

    def __init__(self, ra, dec):
        self.ra = mpf(float(ra))
        dec = mpf(float(dec))
        self.sd, self.cd = mp.sin(dec), mp.cos(dec)
        self.x, self.y, self.z = mp.cos(self.ra) * self.cd, mp.sin(self.ra) * self.cd, self.sd


def double_angle(at, to):
    """``(cos 2 phi, sin 2 phi)`` of the position angle ``phi`` of ``to`` seen from ``at``, from east towards north: the
    bearing of spherical trigonometry (tests/shear_oracle.position_angle)."""
    dra = to.ra - at.ra
    east = to.cd * mp.sin(dra)
    north = at.cd * to.sd - at.sd * to.cd * mp.cos(dra)
    phi = mp.atan2(north, east)
    return mp.cos(2 * phi), mp.sin(2 * phi)


def chord2(a, b):
    return (a.x - b.x) ** 2 + (a.y - b.y) ** 2 + (a.z - b.z) ** 2


def separation(c2):
    return 2 * mp.asin(mp.sqrt(c2) / 2)


def fine_bin(c2, row):
    """``e`` with ``row[e] < c2 <= row[e + 1]`` (the float64 edges taken exactly), or None."""
    if not (c2 > mpf(float(row[0])) and c2 <= mpf(float(row[-1]))):
        return None
    return sum(1 for edge in row if c2 > mpf(float(edge))) - 1


def near_an_edge(c2, t):
    return any(abs(c2 / mpf(float(edge)) - 1) < EDGE_MARGIN for edge in np.unique(t))


def products(w, g1, g2):
    """The rounded float64 products ``w * g`` a handle stores."""
    return np.asarray(w) * np.asarray(g1), np.asarray(w) * np.asarray(g2)


def tangential_terms(w_l, wg1, wg2, cos2, sin2):
    """``(T, X)`` of one pair: ``w_l * -(wg1 cos 2phi + wg2 sin 2phi)`` and ``w_l * (wg1 sin 2phi - wg2 cos 2phi)``."""
    w_l, wg1, wg2 = mpf(float(w_l)), mpf(float(wg1)), mpf(float(wg2))
    return w_l * -(wg1 * cos2 + wg2 * sin2), w_l * (wg1 * sin2 - wg2 * cos2)


def lensing_factor(f, c, u):
    """``(1 - c u, s = f (1 - c u))`` exactly."""
    eff = 1 - mpf(float(c)) * mpf(float(u))
    return eff, mpf(float(f)) * eff


def shear_shear_terms(wg_a, wg_b, angle_a, angle_b):
    """``(P, M, C)`` of one pair from the weighted shears of its two ends and the double angles taken at each end."""
    (a1, a2), (b1, b2) = ((mpf(float(v)) for v in wg) for wg in (wg_a, wg_b))
    (ca, sa), (cb, sb) = angle_a, angle_b
    t_a, x_a = -(a1 * ca + a2 * sa), a1 * sa - a2 * ca
    t_b, x_b = -(b1 * cb + b2 * sb), b1 * sb - b2 * cb
    return t_a * t_b + x_a * x_b, t_a * t_b - x_a * x_b, t_a * x_b + x_a * t_b


class Geometry:
    """Chord^2, separation and the double angles at both ends of the pairs between two lists of points, computed once per
    pair. Pairs far outside every edge are recognised in float64 (a factor 4 in chord^2 against errors of 1e-16)."""

    def __init__(self, first, second, t, symmetric=False):
        self.first = [Point(r, d) for r, d in zip(first["ra"], first["dec"])]
        self.second = self.first if symmetric else [Point(r, d) for r, d in zip(second["ra"], second["dec"])]
        self.symmetric = symmetric
        self.t = t
        self.cache = {}
        xyz_1 = np.array([[float(p.x), float(p.y), float(p.z)] for p in self.first])
        xyz_2 = np.array([[float(p.x), float(p.y), float(p.z)] for p in self.second])
        d2 = ((xyz_1[:, None, :] - xyz_2[None, :, :]) ** 2).sum(axis=2)
        self.far = (d2 > 4.0 * t.max()) | (d2 == 0.0)  # (0: an object and its twin, inside no bin)
        self.edge_violations = 0

    def pair(self, i, j):
        """``(chord^2, theta, double angle at i towards j, double angle at j towards i)`` or None for a far pair."""
        if self.far[i, j]:
            return None
        key = (min(i, j), max(i, j)) if self.symmetric else (i, j)
        if key not in self.cache:
            a, b = self.first[key[0]], self.second[key[1]]
            c2 = chord2(a, b)
            self.edge_violations += near_an_edge(c2, self.t)
            self.cache[key] = (c2, separation(c2), double_angle(a, b), double_angle(b, a))
        c2, theta, at_first, at_second = self.cache[key]
        return (c2, theta, at_first, at_second) if key == (i, j) else (c2, theta, at_second, at_first)


def exact_tangential(lens, src, jobs, t, geometry, dsigma=None):
    """The exact ``(T, X, W, A, A_theta)`` f64[n_jobs, B, E-1] of the tangential count, or of Delta Sigma with ``dsigma =
    (f, c, u)``; the member pairs ``(lens, source)`` with their ``(T, X)``; and the pairs closer than CLIP_MARGIN to the clip."""
    n_bins, nf = t.shape[0], t.shape[1] - 1
    nb = lens["nb"]
    wg1, wg2 = products(src["w"], src["g1"], src["g2"])
    sums = [[[[mpf(0)] * nf for _ in range(n_bins)] for _ in jobs] for _ in range(3)]
    mags = np.zeros((2, len(jobs), n_bins, nf))
    pairs, clip_violations = {}, 0
    for job, (p, q) in enumerate(jobs):
        for k in range(n_bins):
            seg = p * nb + (0 if nb == 1 else k)
            for i in range(int(lens["off"][seg]), int(lens["off"][seg + 1])):
                for j in range(int(src["off"][q]), int(src["off"][q + 1])):
                    geo = geometry.pair(i, j)
                    e = None if geo is None else fine_bin(geo[0], t[k])
                    if e is None:
                        continue
                    _, theta, _, (cos2, sin2) = geo  # the lens seen from the source
                    tv, xv = tangential_terms(lens["w"][i], wg1[j], wg2[j], cos2, sin2)
                    wv = mpf(float(lens["w"][i])) * mpf(float(src["w"][j]))
                    mag = abs(lens["w"][i] * src["w"][j]) * (abs(src["g1"][j]) + abs(src["g2"][j]))
                    if dsigma is not None:
                        eff, s = lensing_factor(dsigma[0][i], dsigma[1][i], dsigma[2][j])
                        clip_violations += abs(eff) < CLIP_MARGIN
                        if s <= 0:
                            pairs.setdefault((i, j), (0.0, 0.0))
                            continue
                        tv, xv, wv, mag = tv * s, xv * s, wv * s * s, mag * float(s)
                    pairs[(i, j)] = (float(tv), float(xv))
                    for plane, v in enumerate((tv, xv, wv)):
                        sums[plane][job][k][e] += v
                    mags[0, job, k, e] += mag
                    mags[1, job, k, e] += mag / float(theta)
    T, X, W = (np.array([[[float(v) for v in row] for row in cell] for cell in plane]) for plane in sums)
    return (T, X, W, mags[0], mags[1]), pairs, clip_violations


def exact_shear_shear(cat_a, cat_b, cells, t, geometry):
    """The exact ``(P, M, C, W, A, A_theta)`` f64[n_cells, E-1] of the pair count's cell list (``cat_b is cat_a``: one handle)
    and the member pairs ``(a, b)`` with their ``(P, M, C)``."""
    nf = t.shape[1] - 1
    one = cat_b is cat_a
    wg_a = np.column_stack(products(cat_a["w"], cat_a["g1"], cat_a["g2"]))
    wg_b = np.column_stack(products(cat_b["w"], cat_b["g1"], cat_b["g2"]))
    mag_a, mag_b = (np.abs(c["g1"]) + np.abs(c["g2"]) for c in (cat_a, cat_b))
    sums = [[[mpf(0)] * nf for _ in cells] for _ in range(4)]
    mags = np.zeros((2, len(cells), nf))
    pairs = {}
    for c, (p, q, ka, kb, row) in enumerate(cells):
        sa, sb = p * cat_a["nb"] + ka, q * cat_b["nb"] + kb
        for i in range(int(cat_a["off"][sa]), int(cat_a["off"][sa + 1])):
            for j in range(int(cat_b["off"][sb]), int(cat_b["off"][sb + 1])):
                if one and sa == sb and j <= i:
                    continue  # a diagonal cell: every unordered pair once
                geo = geometry.pair(i, j)
                e = None if geo is None else fine_bin(geo[0], t[row])
                if e is None:
                    continue
                _, theta, at_a, at_b = geo
                terms = shear_shear_terms(wg_a[i], wg_b[j], at_a, at_b)
                wv = mpf(float(cat_a["w"][i])) * mpf(float(cat_b["w"][j]))
                mag = abs(cat_a["w"][i] * cat_b["w"][j]) * mag_a[i] * mag_b[j]
                pairs[(min(i, j), max(i, j)) if one else (i, j)] = tuple(float(v) for v in terms)
                for plane, v in enumerate((*terms, wv)):
                    sums[plane][c][e] += v
                mags[0, c, e] += mag
                mags[1, c, e] += mag / float(theta)
    P, M, C, W = (np.array([[float(v) for v in cell] for cell in plane]) for plane in sums)
    return (P, M, C, W, mags[0], mags[1]), pairs


# --------------------------------------------------------------------------- scenes
def ring_around(rng, ra_c, dec_c, r):
    """Points (ra in [0, 2 pi), dec) at the separations ``r`` (radian) from (ra_c, dec_c), in any direction."""
    theta = rng.uniform(0.0, 2.0 * np.pi, len(r))
    centre = np.array([np.cos(dec_c) * np.cos(ra_c), np.cos(dec_c) * np.sin(ra_c), np.sin(dec_c)])
    east = np.array([-np.sin(ra_c), np.cos(ra_c), 0.0])
    north = np.cross(centre, east)
    xyz = np.cos(r)[:, None] * centre + np.sin(r)[:, None] * (np.cos(theta)[:, None] * east + np.sin(theta)[:, None] * north)
    return np.arctan2(xyz[:, 1], xyz[:, 0]) % (2.0 * np.pi), np.arcsin(np.clip(xyz[:, 2], -1.0, 1.0))


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def shear_columns(rng, n):
    return dict(w=rng.uniform(0.5, 2.0, n), g1=rng.normal(0.0, 0.3, n), g2=rng.normal(0.0, 0.3, n))


def draw_scenes(rng):
    """The inputs of every scene (float64 columns and offsets)."""
    lens_ra, lens_dec, src_ra, src_dec = [], [], [], []
    for ra_c, dec_c in SITES:
        ra, dec = ring_around(rng, ra_c, dec_c, 1.0 * ARCSEC * np.sqrt(rng.uniform(0.0, 1.0, N_LENS)))
        lens_ra.append(ra), lens_dec.append(dec)
        ra, dec = ring_around(rng, ra_c, dec_c, log_uniform(rng, 0.5, 30.0, N_SRC) * ARCSEC)
        src_ra.append(ra), src_dec.append(dec)
    n_l, n_s = N_LENS * len(SITES), N_SRC * len(SITES)
    lens = dict(ra=np.concatenate(lens_ra), dec=np.concatenate(lens_dec), w=rng.uniform(0.5, 2.0, n_l), nb=2,
                off=np.arange(0, n_l + 1, N_LENS // 2, dtype=np.int64))  # two bins of 15 lenses per site
    src = dict(ra=np.concatenate(src_ra), dec=np.concatenate(src_dec), **shear_columns(rng, n_s),
               off=np.arange(0, n_s + 1, N_SRC, dtype=np.int64))
    # Delta Sigma: c = chi_l and u = 1 / chi_s from one distribution of distances, f below c
    c = rng.uniform(600.0, 2500.0, n_l)
    dsigma = (c / rng.uniform(1.2, 1.9, n_l), c, 1.0 / rng.uniform(600.0, 2500.0, n_s))

    # the pattern scene: one lens at a mid latitude
    ra_l, dec_l = 2.1, 0.9
    ra, dec = ring_around(rng, ra_l, dec_l, log_uniform(rng, 0.5, 30.0, N_PATTERN) * ARCSEC)
    pat_lens = dict(ra=np.array([ra_l]), dec=np.array([dec_l]), w=np.array([1.7]), nb=1, off=np.array([0, 1], dtype=np.int64))
    lens_point = Point(ra_l, dec_l)
    g1, g2 = [], []
    for r, d in zip(ra, dec):
        cos2, sin2 = double_angle(Point(r, d), lens_point)
        g1.append(float(-AMPLITUDE * cos2)), g2.append(float(-AMPLITUDE * sin2))
    pat_src = dict(ra=ra, dec=dec, w=rng.uniform(0.5, 2.0, N_PATTERN), g1=np.array(g1), g2=np.array(g2),
                   off=np.array([0, N_PATTERN], dtype=np.int64))

    # the binned catalogue: per site two bins, the second around a centre 10" away; the wrap site cut at the wrap
    ra_all, dec_all, seg_all = [], [], []
    for site, (ra_c, dec_c) in enumerate(SITES):
        (ra_2,), (dec_2,) = ring_around(rng, ra_c, dec_c, np.array([10.0 * ARCSEC]))
        for k, (ra_k, dec_k) in enumerate(((ra_c, dec_c), (ra_2, dec_2))):
            ra, dec = ring_around(rng, ra_k, dec_k, log_uniform(rng, 0.5, 30.0, N_PER_BIN) * ARCSEC)
            patch = np.full(N_PER_BIN, site) + ((site == WRAP_SITE) & (ra < np.pi))
            ra_all.append(ra), dec_all.append(dec), seg_all.append(patch * 2 + k)
    ra_all, dec_all, seg_all = (np.concatenate(v) for v in (ra_all, dec_all, seg_all))
    order = np.argsort(seg_all, kind="stable")
    n_c = len(order)
    n_patches = len(SITES) + 1
    cat = dict(ra=ra_all[order], dec=dec_all[order], **shear_columns(rng, n_c), nb=2,
               off=np.concatenate([[0], np.cumsum(np.bincount(seg_all, minlength=2 * n_patches))]).astype(np.int64))
    twin = dict(cat, **shear_columns(rng, n_c))
    return lens, src, dsigma, pat_lens, pat_src, cat, twin


def job_lists():
    sites = range(len(SITES))
    tan_jobs = np.array([(p, p) for p in sites] + [(0, 1), (4, 3)], dtype=np.int32)
    west, east = WRAP_SITE, WRAP_SITE + 1  # the two patches of the wrap site
    patches = range(len(SITES) + 1)
    auto_jobs = np.array([(p, p) for p in patches] + [(west, east), (0, 1)], dtype=np.int32)
    one = [(p, p, k, k, k) for p in patches for k in (0, 1)] + [(west, east, k, k, k) for k in (0, 1)] + [(0, 1, 0, 0, 0)]
    one += [(p, p, 0, 1, row) for p in patches for row in (0, 1)] + [(p, p, 1, 0, 0) for p in (1, west)]
    one += [(west, east, 0, 1, 0), (east, west, 0, 1, 1), (west, east, 1, 0, 1), (2, 3, 0, 1, 0)]
    two = [(p, p, ka, kb, ka) for p in patches for ka in (0, 1) for kb in (0, 1)]
    two += [(p, q, ka, kb, kb) for p, q in ((west, east), (east, west)) for ka in (0, 1) for kb in (0, 1)] + [(1, 0, 1, 1, 0)]
    return tan_jobs, auto_jobs, np.array(one, dtype=np.int32), np.array(two, dtype=np.int32)


def auto_cells(jobs):
    return np.array([(p, q, k, k, k) for p, q in jobs for k in (0, 1)], dtype=np.int32)


def pair_arrays(prefix, pairs, names):
    keys = sorted(pairs)
    out = {f"{prefix}.pairs": np.array(keys, dtype=np.int32).reshape(-1, 2)}
    for c, name in enumerate(names):
        out[f"{prefix}.pair_{name}"] = np.array([pairs[k][c] for k in keys], dtype=np.float64)
    return out


def compute(rng):
    """One draw of the inputs and everything derived from it -> (arrays, number of pairs that break a condition)."""
    lens, src, dsigma, pat_lens, pat_src, cat, twin = draw_scenes(rng)
    t = thresholds()
    tan_jobs, auto_jobs, one_cells, two_cells = job_lists()
    arrays = {"t": t, "eps": np.float64(2.0**-52)}
    violations = 0

    geometry = Geometry(lens, src, t)
    tan, tan_pairs, _ = exact_tangential(lens, src, tan_jobs, t, geometry)
    ds, ds_pairs, clipped = exact_tangential(lens, src, tan_jobs, t, geometry, dsigma)
    violations += geometry.edge_violations + clipped
    assert sorted(tan_pairs) == sorted(ds_pairs)
    for side, cols in (("lens", lens), ("src", src)):
        arrays.update({f"tan.{side}.{c}": v for c, v in cols.items() if c != "nb"})
    arrays.update({"tan.n_patches": np.int32(len(SITES)), "tan.jobs": tan_jobs, "ds.f": dsigma[0], "ds.c": dsigma[1], "ds.u": dsigma[2]})
    for prefix, planes in (("tan", tan), ("ds", ds)):
        arrays.update({f"{prefix}.{n}": v for n, v in zip(("T", "X", "W", "A", "Ath"), planes)})
    arrays.update(pair_arrays("tan", tan_pairs, ("T", "X")))
    arrays.update({k.replace("tan.", "ds."): v for k, v in pair_arrays("tan", ds_pairs, ("T", "X")).items() if "pair_" in k})

    geometry = Geometry(pat_lens, pat_src, t[:1])
    pat, pat_pairs, _ = exact_tangential(pat_lens, pat_src, np.array([[0, 0]]), t[:1], geometry)
    violations += geometry.edge_violations
    for side, cols in (("lens", pat_lens), ("src", pat_src)):
        arrays.update({f"pat.{side}.{c}": v for c, v in cols.items() if c != "nb"})
    arrays.update({"pat.n_patches": np.int32(1), "pat.jobs": np.array([[0, 0]], dtype=np.int32), "pat.amplitude": np.float64(AMPLITUDE)})
    arrays.update({f"pat.{n}": v for n, v in zip(("T", "X", "W", "A", "Ath"), pat)})
    arrays.update(pair_arrays("pat", pat_pairs, ("T", "X")))

    geometry = Geometry(cat, cat, t, symmetric=True)
    auto, auto_pairs = exact_shear_shear(cat, cat, auto_cells(auto_jobs), t, geometry)
    one, one_pairs = exact_shear_shear(cat, cat, one_cells, t, geometry)
    violations += geometry.edge_violations
    geometry = Geometry(cat, twin, t)
    two, two_pairs = exact_shear_shear(cat, twin, two_cells, t, geometry)
    violations += geometry.edge_violations
    arrays.update({f"cat.{c}": v for c, v in cat.items() if c != "nb"})
    arrays.update({f"catb.{c}": twin[c] for c in ("w", "g1", "g2")})
    arrays.update({"auto.jobs": auto_jobs, "one.cells": one_cells, "two.cells": two_cells})
    names = ("P", "M", "C", "W", "A", "Ath")
    arrays.update({f"auto.{n}": v.reshape(len(auto_jobs), 2, -1) for n, v in zip(names, auto)})
    arrays.update({f"one.{n}": v for n, v in zip(names, one)})
    arrays.update({f"two.{n}": v for n, v in zip(names, two)})
    arrays.update(pair_arrays("one", {**auto_pairs, **one_pairs}, ("P", "M", "C")))
    arrays.update(pair_arrays("two", two_pairs, ("P", "M", "C")))
    return arrays, int(violations)


# --------------------------------------------------------------------------- the oracles against the file: K
def oracle_ratios(fx):
    """Worst ``|oracle - exact| / (eps A_theta)`` of the four numpy oracles per scene (tests/shear_exact.worst_ratio)."""
    import dsigma_oracle
    import shear_auto_oracle
    import shear_exact as se
    import shear_oracle
    import shear_pair_oracle

    t = fx["t"]
    out = {}
    lens, src = se.lenses(fx, "tan"), se.sources(fx, "tan")
    got = shear_oracle.shear_jobs(lens, src, fx["tan.jobs"], t)
    out["tan"] = max(se.worst_ratio(got[c], fx[f"tan.{n}"], fx["tan.A"], fx["tan.Ath"]) for c, n in enumerate("TX"))
    got = dsigma_oracle.dsigma_jobs(dict(lens, f=fx["ds.f"], c=fx["ds.c"]), dict(src, u=fx["ds.u"]), fx["tan.jobs"], t)
    out["ds"] = max(se.worst_ratio(got[c], fx[f"ds.{n}"], fx["ds.A"], fx["ds.Ath"]) for c, n in enumerate("TX"))
    got = shear_oracle.shear_jobs(se.lenses(fx, "pat"), se.sources(fx, "pat"), fx["pat.jobs"], t[:1])
    out["pat"] = max(se.worst_ratio(got[c], fx[f"pat.{n}"], fx["pat.A"], fx["pat.Ath"]) for c, n in enumerate("TX"))
    cat = se.catalogue(fx, "cat")
    twin = dict(cat, w=fx["catb.w"], g1=fx["catb.g1"], g2=fx["catb.g2"])
    got = shear_auto_oracle.shear_auto_jobs(cat, fx["auto.jobs"], t)
    out["auto"] = max(se.worst_ratio(got[c], fx[f"auto.{n}"], fx["auto.A"], fx["auto.Ath"]) for c, n in enumerate("PMC"))
    got = shear_pair_oracle.shear_pair_cells(cat, cat, fx["one.cells"], t)
    out["one"] = max(se.worst_ratio(got[c], fx[f"one.{n}"], fx["one.A"], fx["one.Ath"]) for c, n in enumerate("PMC"))
    got = shear_pair_oracle.shear_pair_cells(cat, twin, fx["two.cells"], t)
    out["two"] = max(se.worst_ratio(got[c], fx[f"two.{n}"], fx["two.A"], fx["two.Ath"]) for c, n in enumerate("PMC"))
    return out


def write_design(K, worst):
    with open(DESIGN, encoding="utf-8") as fh:
        text = fh.read()
    marked = re.compile(r"(<!-- shear-exact-K -->).*?(<!-- /shear-exact-K -->)", re.S)
    if not marked.search(text):
        print("DESIGN.md has no shear-exact-K markers: not updated")
        return
    new = marked.sub(lambda m: f"{m.group(1)}`K` = {K:g} (worst measured ratio of the numpy oracles {worst:.2f}){m.group(2)}", text)
    if new != text:
        with open(DESIGN, "w", encoding="utf-8") as fh:
            fh.write(new)
    print(f"DESIGN.md: K = {K:g}")


def main():
    rng = np.random.default_rng(SEED)
    draws = 0
    while True:
        draws += 1
        arrays, violations = compute(rng)
        if violations == 0:
            break
        print(f"draw {draws}: {violations} pairs within {EDGE_MARGIN:g} of an edge or of the clip: drawing again")
    n_pairs = sum(len(arrays[f"{p}.pairs"]) for p in ("tan", "pat", "one", "two"))
    print(f"draw {draws}: both conditions hold, 0 pairs excluded; {n_pairs} member pairs "
          f"(tan/ds {len(arrays['tan.pairs'])}, pat {len(arrays['pat.pairs'])}, one handle {len(arrays['one.pairs'])}, "
          f"two handles {len(arrays['two.pairs'])}); mpmath {mpmath.__version__} at {mp.dps} digits")
    behind = arrays["ds.pair_T"] != 0.0
    print(f"Delta Sigma: {behind.mean():.2f} of the member pairs have the source behind the lens")
    ratios = oracle_ratios(arrays)
    worst = max(ratios.values())
    K = 2.0 ** int(np.ceil(np.log2(4.0 * worst)))
    print("worst |oracle - exact| / (eps A_theta): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    print(f"measured worst {worst:.3f} -> K = {K:g}")
    assert worst <= 10.0, "a worst ratio above ~10 says the reference is wrong, not the tolerance"
    arrays.update({"K": np.float64(K), "K_measured": np.float64(worst)})
    save(OUT, arrays)
    write_design(K, worst)


if __name__ == "__main__":
    main()
