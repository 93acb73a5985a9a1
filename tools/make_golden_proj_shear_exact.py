#!/usr/bin/env python3
"""Generate ``tests/golden/proj_shear_exact.npz``: an exact reference of the projected position-shape count
(``yawhip_proj_count_shear``) from arcseconds up to the cap of its reach, 5.73 degrees.

Runs on the CPU with ``mpmath`` at 50 digits; no GPU, no reference package. The arithmetic of a pair is that of
tools/make_golden_shear_exact.py and tools/make_golden_proj_exact.py, imported from there (``Point``, ``chord2``,
``separation``, ``double_angle``, ``tangential_terms``, ``products``; ``bin_of``, ``pi_plane``; the file is written by ``save``).
Per pair of a density object and a shape the tool takes the float64 ``(ra, dec)`` of both and the float64 columns, computes
``theta = 2 asin(chord / 2)``, ``R2 = ((d_a + d_b) / 2)^2 theta^2`` and ``p = |c_a - c_b|`` exactly and tests them against the
float64 edges taken exactly, and rotates the shape's rounded products ``w g1, w g2`` by the exact bearing of the density
object seen from the shape (spherical trigonometry). NOTHING here evaluates the contract's series of the squared angle or its
algebra of the double angle.

Scenes: a density catalogue ``dens`` and a shape catalogue ``shapes``; every site has two patches over the same area and two
redshift bins per patch; the cells are ``proj_scenes.cells_two_handles`` and two between different sites, which hold nothing
(``proj_exact.cell_lists``); row = bin.
  as     the ``as`` scene of tools/make_golden_proj_exact.py (five sites: dec 0, 60, +-89.99 degrees, the wrap of the right
         ascension; 14 objects per segment on rings of 0.5" ... 30"; ``d`` 600 ... 2500), its catalogue ``b`` with ``g1``, ``g2``
  wide   sites at dec 0 and 60 degrees, one at 86 degrees whose rings pass over the pole, one whose partners straddle the wrap:
         14 objects per segment, log-uniform from 3' to 5.6 degrees around the site; in every (catalogue, bin) the least ``d``
         has ``r2max / least^2`` between 0.0095 and 0.00999 and the others are up to 4 times farther
Three sets of pi edges (``one``: ``[0, 40]``; ``four``: four equal bins; ``uneven``: the five of tests/proj_pi_oracle.py).

Condition, asserted at 50 digits; the inputs are redrawn until it holds, so that no pair is left out: no pair of any cell has
its exact ``R2`` within a relative 1e-6 of an edge of either row, or its ``p`` within a relative 1e-6 of a pi edge of any set.

Per scene and edge set the file holds ``N`` (integer member pairs), the exact ``T``, ``X``, ``W`` for the stored weights, ``A =
sum |w_a w_b| (|g1| + |g2|)`` and ``Ath``, the same sum with every pair divided by its angle, f64[n_pi, n_cells, nf] each, rounded
once. The numpy oracle with unit weights must give ``N`` cell for cell: a mismatch is a finding about the contract, and the
tool stops. ``K`` of the rule ``|ours - exact| <= K 2^-52 Ath + 1e-13 A`` is four times the oracle's worst ``|oracle - exact| /
(2^-52 Ath)`` over the file, rounded up to a power of two; it goes into the file.

Running it again reproduces the file byte for byte.

Usage:  python tools/make_golden_proj_shear_exact.py
"""
from __future__ import annotations

import collections
import os
import sys

import mpmath
import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (HERE, ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

from make_golden_dsigma_radial_exact import WIDE_SITES, bin_of  # noqa: E402
from make_golden_proj_exact import catalogue, draw_as, far_apart, pi_plane, radii2  # noqa: E402
from make_golden_shear_exact import (ARCSEC, DEG, SITES, Point, chord2, double_angle, log_uniform, products, ring_around, save,  # noqa: E402
                                     separation, tangential_terms)

OUT = os.path.join(ROOT, "tests", "golden", "proj_shear_exact.npz")
mp.dps = 50
SEED = 20261024
MARGIN = 1e-6
PMAX = 40.0
PER_SEGMENT_WIDE = 14
PI_SETS = {"one": np.array([0.0, PMAX]), "four": np.linspace(0.0, PMAX, 5), "uneven": np.array([0.0, 0.7, 3.1, 9.3, 22.9, PMAX])}
SITES_OF = {"as": SITES, "wide": WIDE_SITES}


def draw_wide(rng):
    r2 = radii2("wide")
    cats = {}
    for cat in ("dens", "shapes"):
        least = [np.sqrt(r2[k, -1] / rng.uniform(0.0095, 0.00999)) for k in range(2)]
        segments = []
        for site, (ra_c, dec_c) in enumerate(WIDE_SITES):
            for patch in range(2):
                for k in range(2):
                    n = PER_SEGMENT_WIDE
                    ra, dec = ring_around(rng, ra_c, dec_c, log_uniform(rng, 3.0 * 60.0 * ARCSEC, 5.6 * DEG, n))
                    d = least[k] * log_uniform(rng, 1.0, 4.0, n)
                    if site == 0 and patch == 0:
                        d[0] = least[k]  # the nearest object of the bin: the reach is next to the cap
                    segments.append((ra, dec, d, rng.uniform(0.0, 120.0, n)))
        cats[cat] = catalogue(segments)
        cats[cat]["w"] = rng.uniform(0.5, 2.0, len(cats[cat]["ra"]))
    return cats["dens"], cats["shapes"]


def draw(scene, rng):
    dens, shapes = draw_as(rng) if scene == "as" else draw_wide(rng)
    n = len(shapes["ra"])
    shapes["g1"], shapes["g2"] = rng.normal(0.0, 0.3, n), rng.normal(0.0, 0.3, n)
    return dens, shapes


def exact_scene(scene, dens, shapes, r2):
    """Every pair of the cells -> (arrays of the scene, number of pairs that break the condition, nearest margins)."""
    import proj_exact

    n_sites = len(SITES_OF[scene])
    nf = r2.shape[1] - 1
    cells = proj_exact.cell_lists(n_sites, False, True)
    points = [[Point(r, d) for r, d in zip(cat["ra"], cat["dec"])] for cat in (dens, shapes)]
    edges = [[mpf(float(e)) for e in row] for row in r2]
    every_edge = [e for row in edges for e in row]
    pi_edges = {name: [mpf(float(e)) for e in pe] for name, pe in PI_SETS.items()}
    every_pi_edge = sorted({e for pe in pi_edges.values() for e in pe if e > 0})
    wg1, wg2 = products(shapes["w"], shapes["g1"], shapes["g2"])
    sums = collections.defaultdict(lambda: [mpf(0)] * 5)  # (set, plane, cell, bin) -> T, X, W, A, Ath
    N = {name: np.zeros((len(pe) - 1, len(cells), nf)) for name, pe in PI_SETS.items()}
    violations, margin, pi_margin = 0, np.inf, np.inf
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        assert not diagonal
        if n >= len(cells) - 2:
            assert far_apart(dens, shapes, sa, sb, dens["off"], shapes["off"], r2), "a cell between sites holds a pair"
            continue
        for i in range(int(dens["off"][sa]), int(dens["off"][sa + 1])):
            for j in range(int(shapes["off"][sb]), int(shapes["off"][sb + 1])):
                c2 = chord2(points[0][i], points[1][j])
                theta = separation(c2)
                DD = ((mpf(float(dens["d"][i])) + mpf(float(shapes["d"][j]))) / 2) ** 2
                R2 = DD * theta * theta
                p = abs(mpf(float(dens["c"][i])) - mpf(float(shapes["c"][j])))
                near, pi_near = float(min(abs(R2 / e - 1) for e in every_edge)), float(min(abs(p / e - 1) for e in every_pi_edge))
                margin, pi_margin = min(margin, near), min(pi_margin, pi_near)
                violations += (near < MARGIN) + (pi_near < MARGIN)
                e = bin_of(R2, edges[row])
                if e is None:
                    continue
                tv, xv = tangential_terms(dens["w"][i], wg1[j], wg2[j], *double_angle(points[1][j], points[0][i]))
                ww = mpf(float(dens["w"][i])) * mpf(float(shapes["w"][j]))
                size = abs(ww) * (abs(mpf(float(shapes["g1"][j]))) + abs(mpf(float(shapes["g2"][j]))))
                for name, pe in pi_edges.items():
                    plane = pi_plane(p, pe)
                    if plane is None:
                        continue
                    N[name][plane, n, e] += 1
                    key = (name, plane, n, e)
                    sums[key] = [s + t for s, t in zip(sums[key], (tv, xv, ww, size, size / theta))]
    out = {"r2": r2, "n_sites": np.int32(n_sites), "cells": cells}
    for cat, cols in (("dens", dens), ("shapes", shapes)):
        out.update({f"{cat}.{c}": v for c, v in cols.items()})
    for name, pe in PI_SETS.items():
        out[f"{name}.N"] = N[name]
        for c, plane in enumerate(("T", "X", "W", "A", "Ath")):
            out[f"{name}.{plane}"] = np.array([[[float(sums[(name, j, n, e)][c]) for e in range(nf)] for n in range(len(cells))]
                                               for j in range(len(pe) - 1)])
    out.update(margin=np.float64(margin), pi_margin=np.float64(pi_margin))
    return {f"{scene}.{k}": v for k, v in out.items()}, int(violations)


def oracle_planes(arrays, scene, name, weighted, variant=None):
    import proj_shear_exact
    import proj_shear_oracle

    dens, shapes = (proj_shear_exact.catalogue(arrays, scene, cat, weighted) for cat in ("dens", "shapes"))
    return proj_shear_oracle.proj_shear_cells(dens, shapes, arrays[f"{scene}.cells"], arrays[f"{scene}.r2"], PI_SETS[name], variant)


def main():
    import proj_shear_exact

    rng = np.random.default_rng(SEED)
    arrays = {"eps": np.float64(proj_shear_exact.EPS), "pmax": np.float64(PMAX), "margin": np.float64(MARGIN)}
    arrays.update({f"pi.{name}": pe for name, pe in PI_SETS.items()})
    for scene in ("as", "wide"):
        draws = 0
        while True:
            draws += 1
            dens, shapes = draw(scene, rng)
            part, violations = exact_scene(scene, dens, shapes, radii2(scene))
            members = part[f"{scene}.one.N"].sum()
            if violations == 0 and members > 1000:
                break
            print(f"{scene} draw {draws}: {violations} pairs within {MARGIN:g} of an edge, {members:.0f} member pairs: drawing again")
        arrays.update(part)
        arrays[f"{scene}.draws"] = np.int32(draws)
        print(f"{scene} draw {draws}: the condition holds, 0 pairs excluded; {members:.0f} member pairs inside the cut, nearest radius edge "
              f"{part[f'{scene}.margin']:.2e} away, nearest edge in p {part[f'{scene}.pi_margin']:.2e}")
        for name in PI_SETS:
            got = oracle_planes(arrays, scene, name, False)
            if not (np.array_equal(got[4], arrays[f"{scene}.{name}.N"]) and np.array_equal(got[2], got[4])):
                sys.exit(f"{scene} {name}: the numpy oracle does not count the pairs of the exact reference: a finding about the contract")
    worst = 0.0
    for scene in ("as", "wide"):
        for name in PI_SETS:
            got, exp = oracle_planes(arrays, scene, name, True), proj_shear_exact.expected(arrays, scene, name)
            np.testing.assert_allclose(got[3], exp["A"], rtol=1e-12, atol=0)
            ratios = [proj_shear_exact.worst_ratio(got[c], exp[plane], exp["Ath"]) for c, plane in enumerate("TX")]
            print(f"{scene} {name}: worst |oracle - exact| / (2^-52 Ath): T {ratios[0]:.3f}, X {ratios[1]:.3f}")
            worst = max(worst, *ratios)
    K = 2.0 ** int(np.ceil(np.log2(4.0 * worst)))
    print(f"mpmath {mpmath.__version__} at {mp.dps} digits; measured worst {worst:.3f} -> K = {K:g}")
    assert worst <= 10.0, "a worst ratio above ~10 says the reference is wrong, not the tolerance"
    arrays.update({"K": np.float64(K), "K_measured": np.float64(worst)})
    save(OUT, arrays)


if __name__ == "__main__":
    main()
