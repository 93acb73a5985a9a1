#!/usr/bin/env python3
"""Generate ``tests/golden/proj_shape_exact.npz``: an exact reference of the projected shape-shape count
(``yawhip_proj_count_shapes``) from arcseconds up to the cap of its reach, 5.73 degrees.

Runs on the CPU with ``mpmath`` at 50 digits; no GPU, no reference package. The arithmetic of a pair is that of
tools/make_golden_shear_exact.py and the projected tools, imported from there (``Point``, ``chord2``, ``separation``,
``double_angle``, ``products``, ``shear_shear_terms``; ``bin_of``, ``pi_plane``; the file is written by ``save``). Per pair of
two shapes the tool takes the float64 ``(ra, dec)`` of both and the float64 columns, computes ``theta = 2 asin(chord / 2)``,
``R2 = ((d_a + d_b) / 2)^2 theta^2`` and ``p = |c_a - c_b|`` exactly and tests them against the float64 edges taken exactly, and
rotates the rounded products ``w g1, w g2`` of EACH end by the exact bearing of the other end seen from it (spherical
trigonometry: ``double_angle(at=a, to=b)`` and ``double_angle(at=b, to=a)``). With ``(P, M, C)`` of ``shear_shear_terms``,

    PP = (P + M) / 2 = tA tB     XX = (P - M) / 2 = xA xB     PX = C = tA xB + xA tB     W = w_a w_b

exactly. NOTHING here evaluates the contract's series of the squared angle or its ``pa / pb / den`` algebra.

Scenes ``as`` and ``wide``: two shape catalogues ``a`` and ``b`` (weights 0.5 ... 2, ``g1, g2 ~ N(0, 0.3)``); every site has two
patches over the same area and two redshift bins per patch; two cell lists, ``two`` (``a`` with ``b``:
``proj_exact.cell_lists(n_sites, False, True)``) and ``one`` (``a`` with itself: diagonal cells, which hold every unordered pair
once, and the two patches of a site against each other), each with two cells between different sites, which hold nothing;
row = bin.
  as     the ``as`` scene of tools/make_golden_proj_exact.py (five sites: dec 0, 60, +-89.99 degrees, the wrap of the right
         ascension; 14 objects per segment on rings of 0.5" ... 30"; ``d`` 600 ... 2500)
  wide   the ``wide`` scene of tools/make_golden_proj_shear_exact.py (sites at dec 0 and 60 degrees, one at 86 degrees whose
         rings pass over the pole, one whose partners straddle the wrap; 14 objects per segment, 3' ... 5.6 degrees); in every
         (catalogue, bin) the least ``d`` has ``r2max / least^2`` between 0.0095 and 0.00999: the reach is at the cap
  pairs  the known answer, independent of every oracle: one catalogue of one patch and two bins, 6 isolated pairs per bin
         (objects 2 k and 2 k + 1 of a segment), the partners 0.5 ... 5.5 degrees apart at ``d`` 1000 ... 1010, different pairs
         farther apart than the largest radius; pairs at dec 0 and 60 degrees, one whose great circle passes within 0.1
         degree of the pole, one that straddles the wrap. The cells are the two diagonal ones. Three sets of shears:
           along  every shape has amplitude ``e = 0.1`` along the exact bearing of its partner, ``(g1, g2) = e (cos 2 phi,
                  sin 2 phi)`` rounded once: ``PP = sum w_a w_b e^2``, ``XX`` and ``PX`` zero to rounding
           both   both ends turned by 45 degrees, ``(g1, g2) -> (-g2, g1)``: ``XX = sum w_a w_b e^2``, ``PP`` and ``PX`` zero
           one    the first shape of each pair turned: ``PP`` and ``XX`` zero, ``PX = + sum w_a w_b e^2``

The sign of ``PX`` in ``one``, from the definitions ("The sign of +x"): with ``phi`` the position angle of
the partner from east towards north, ``(t, x) = (-(g1 cos 2 phi + g2 sin 2 phi), g1 sin 2 phi - g2 cos 2 phi)``. A shape along
``phi`` has ``(t, x) = (-e, 0)``, that is ``e+ = -t = +e``. Turned by +45 degrees (towards north; the double angle by 90
degrees, ``(g1, g2) -> (-g2, g1)``) it has ``(t, x) = (0, -e)``. For ``a`` turned and ``b`` not, ``PX = tA xB + xA tB =
(-e w_a) (-e w_b) = + w_a w_b e^2``, and the ``+x`` product in ``e+ = -t`` and ``ex = x`` is ``e+_a ex_b + ex_a e+_b = - w_a w_b
e^2``: ``PX`` is POSITIVE and ``ShapeShapeCorrFunc.sample("plus_cross")``, which flips it once, is NEGATIVE. Both are symmetric
in which end is turned.

Three sets of pi edges (``one``: ``[0, 40]``; ``four``: four equal bins; ``uneven``: the five of tests/proj_pi_oracle.py).

Condition, asserted at 50 digits; the inputs are redrawn until it holds, so that no pair is left out: no pair of any cell has
its exact ``R2`` within a relative 1e-6 of an edge of either row, or its ``p`` within a relative 1e-6 of a pi edge of any set.
``as`` and ``wide`` hold more than 1000 member pairs in either cell list, every pi bin of every set holds pairs, and in ``one``
diagonal and off-diagonal cells both do.

Per scene, cell list (``pairs``: set of shears) and pi set the file holds ``<scene>.<list>.<set>.<plane>`` f64[n_pi, n_cells, nf],
each rounded once: ``N`` (integer member pairs), the exact ``PP``, ``XX``, ``PX``, ``W`` for the stored weights, ``A = sum |w_a w_b|
(|g1_a| + |g2_a|) (|g1_b| + |g2_b|)`` and ``Ath``, the same sum with every pair divided by its angle. The numpy oracle with unit
weights must give ``N`` element for element: a mismatch is a finding about the contract, and the tool stops. ``K`` of the rule
``|ours - exact| <= K 2^-52 Ath + 1e-13 A`` is four times the oracle's worst ``|oracle - exact| / (2^-52 Ath)`` over the file and
its three signed planes, rounded up to a power of two; it goes into the file and into DESIGN.md (between the
``proj-shape-exact-K`` markers). Above a worst ratio of 20 the tool stops: then the reference or the oracle is wrong.

Running it again reproduces the file byte for byte.

Usage:  python tools/make_golden_proj_shape_exact.py
"""
from __future__ import annotations

import os
import re
import sys
import time

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
from make_golden_proj_shear_exact import PI_SETS, PMAX, draw_wide  # noqa: E402
from make_golden_shear_exact import (DEG, SITES, Point, chord2, double_angle, log_uniform, products, ring_around, save,  # noqa: E402
                                     separation, shear_shear_terms)

OUT = os.path.join(ROOT, "tests", "golden", "proj_shape_exact.npz")
DESIGN = os.path.join(ROOT, "DESIGN.md")
mp.dps = 50
SEED = 20261027
MARGIN = 1e-6
WORST_ALLOWED = 20.0  # one rotated end: 10 (the siblings); two bearings enter every term here
SITES_OF = {"as": SITES, "wide": WIDE_SITES}
PLANES = ("PP", "XX", "PX", "W", "A", "Ath")
SIGNED = ("PP", "XX", "PX")
VARIANTS = ("along", "both", "one")

# the known answer
AMPLITUDE = 0.1
PAIR_SITES = (  # the first shape of a pair (ra, dec), or both shapes; six pairs per bin
    ((1.0, 0.0), (2.1, 60.0 * DEG), ((1.0, 88.0 * DEG), (1.0 + np.pi - 0.03, 87.5 * DEG)), ((2.0 * np.pi - 0.01, 0.3), (0.02, 0.31)),
     (3.0, -0.7), (4.5, 0.4)),
    ((0.3, 0.0), (5.2, 60.0 * DEG), (1.7, -1.2), (3.8, 1.0), (2.6, 0.2), (0.9, -0.4)))
POLE_PAIR, WRAP_PAIR = 2, 3  # of bin 0
PAIR_CELLS = np.array([(0, 0, 0, 1), (1, 1, 1, 1)], dtype=np.int32)
PAIR_R2 = np.array([np.geomspace(8.5, 99.0, 4), np.geomspace(8.6, 99.5, 4)]) ** 2


# --------------------------------------------------------------------------- scenes
def draw(scene, rng):
    a, b = draw_as(rng) if scene == "as" else draw_wide(rng)
    for cat in (a, b):
        n = len(cat["ra"])
        cat["g1"], cat["g2"] = rng.normal(0.0, 0.3, n), rng.normal(0.0, 0.3, n)
    return a, b


def along_partner(ra, dec):
    """``(g1, g2)`` of amplitude AMPLITUDE along the exact bearing of the partner (objects 2 k and 2 k + 1), rounded once."""
    points = [Point(r, d) for r, d in zip(ra, dec)]
    g1, g2 = np.empty(len(ra)), np.empty(len(ra))
    for i, here in enumerate(points):
        cos2, sin2 = double_angle(here, points[i ^ 1])
        g1[i], g2[i] = float(mpf(AMPLITUDE) * cos2), float(mpf(AMPLITUDE) * sin2)
    return g1, g2


def draw_pairs(rng):
    """The catalogue of the known answer and its three sets of shears ``{variant: (g1, g2)}``."""
    segments = []
    for sites in PAIR_SITES:
        ra, dec = [], []
        for site in sites:
            if np.ndim(site[0]):
                (ra_0, dec_0), (ra_1, dec_1) = site
            else:
                ra_0, dec_0 = site
                (ra_1,), (dec_1,) = ring_around(rng, ra_0, dec_0, log_uniform(rng, 0.5 * DEG, 5.5 * DEG, 1))
            ra += [ra_0, ra_1]
            dec += [dec_0, dec_1]
        n = len(ra)
        c = np.repeat(rng.uniform(40.0, 80.0, n // 2), 2)
        c[1::2] += rng.uniform(-38.0, 38.0, n // 2)
        segments.append((np.array(ra), np.array(dec), rng.uniform(1000.0, 1010.0, n), c))
    cat = catalogue(segments)
    cat["w"] = rng.uniform(0.5, 2.0, len(cat["ra"]))
    g1, g2 = along_partner(cat["ra"], cat["dec"])
    first = np.arange(len(g1)) % 2 == 0
    shears = {"along": (g1, g2), "both": (-g2, g1), "one": (np.where(first, -g2, g1), np.where(first, g1, g2))}
    return cat, shears


def pole_distance(ra, dec):
    """The least angle between the great circle through two points and the pole, radian, in float64."""
    xyz = np.array([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)]).T
    normal = np.cross(xyz[0], xyz[1])
    return float(np.arcsin(abs(normal[2]) / np.linalg.norm(normal)))


# --------------------------------------------------------------------------- exact arithmetic
def mp_points(cat):
    return [Point(r, d) for r, d in zip(cat["ra"], cat["dec"])]


def exact_cells(a, b, points_a, points_b, cells, r2, empty_tail):
    """Every pair of the cells of ``a`` with ``b`` (``b is a``: one handle, a diagonal cell takes ``i < j``) ->
    ``({(set, plane): f64[n_pi, n_cells, nf]}, pairs that break the condition, nearest radius edge, nearest pi edge)``; the
    last ``empty_tail`` cells lie between sites and must hold nothing."""
    same = b is a
    nf = r2.shape[1] - 1
    edges = [[mpf(float(e)) for e in row] for row in r2]
    every_edge = [e for row in edges for e in row]
    pi_edges = {name: [mpf(float(e)) for e in pe] for name, pe in PI_SETS.items()}
    every_pi_edge = sorted({e for pe in pi_edges.values() for e in pe if e > 0})
    wg_a = np.column_stack(products(a["w"], a["g1"], a["g2"]))
    wg_b = np.column_stack(products(b["w"], b["g1"], b["g2"]))
    mag_a, mag_b = ([abs(mpf(float(u))) + abs(mpf(float(v))) for u, v in zip(cat["g1"], cat["g2"])] for cat in (a, b))
    sums = {}  # (set, plane of pi, cell, bin) -> [PP, XX, PX, W, A, Ath]
    N = {name: np.zeros((len(pe) - 1, len(cells), nf)) for name, pe in PI_SETS.items()}
    violations, margin, pi_margin = 0, np.inf, np.inf
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        assert bool(diagonal) == (same and sa == sb)
        if n >= len(cells) - empty_tail:
            assert far_apart(a, b, sa, sb, a["off"], b["off"], r2), "a cell between sites holds a pair"
            continue
        for i in range(int(a["off"][sa]), int(a["off"][sa + 1])):
            for j in range(int(b["off"][sb]), int(b["off"][sb + 1])):
                if diagonal and j <= i:
                    continue  # a diagonal cell: every unordered pair once
                theta = separation(chord2(points_a[i], points_b[j]))
                DD = ((mpf(float(a["d"][i])) + mpf(float(b["d"][j]))) / 2) ** 2
                R2 = DD * theta * theta
                p = abs(mpf(float(a["c"][i])) - mpf(float(b["c"][j])))
                near, pi_near = float(min(abs(R2 / e - 1) for e in every_edge)), float(min(abs(p / e - 1) for e in every_pi_edge))
                margin, pi_margin = min(margin, near), min(pi_margin, pi_near)
                violations += (near < MARGIN) + (pi_near < MARGIN)
                e = bin_of(R2, edges[row])
                if e is None or p > every_pi_edge[-1]:
                    continue
                P, M, C = shear_shear_terms(wg_a[i], wg_b[j], double_angle(points_a[i], points_b[j]), double_angle(points_b[j], points_a[i]))
                ww = mpf(float(a["w"][i])) * mpf(float(b["w"][j]))
                size = abs(ww) * mag_a[i] * mag_b[j]
                terms = ((P + M) / 2, (P - M) / 2, C, ww, size, size / theta)
                for name, pe in pi_edges.items():
                    plane = pi_plane(p, pe)
                    if plane is None:
                        continue
                    N[name][plane, n, e] += 1
                    key = (name, plane, n, e)
                    sums[key] = [s + t for s, t in zip(sums.get(key, [mpf(0)] * 6), terms)]
    out = {}
    for name, pe in PI_SETS.items():
        out[(name, "N")] = N[name]
        for c, plane in enumerate(PLANES):
            out[(name, plane)] = np.array([[[float(sums.get((name, j, n, e), [mpf(0)] * 6)[c]) for e in range(nf)] for n in range(len(cells))]
                                           for j in range(len(pe) - 1)])
    return out, int(violations), margin, pi_margin


def exact_scene(scene, a, b, r2):
    """Both cell lists of ``as`` or ``wide`` -> (arrays of the scene, pairs that break the condition, complaints)."""
    import proj_exact

    n_sites = len(SITES_OF[scene])
    out = {"r2": r2, "n_sites": np.int32(n_sites)}
    for cat, cols in (("a", a), ("b", b)):
        out.update({f"{cat}.{c}": v for c, v in cols.items()})
    points = {"a": mp_points(a), "b": mp_points(b)}
    violations, margin, pi_margin, complaints = 0, np.inf, np.inf, []
    for which, two in (("two", True), ("one", False)):
        cells = proj_exact.cell_lists(n_sites, False, two)
        planes, bad, near, pi_near = exact_cells(a, b if two else a, points["a"], points["b" if two else "a"], cells, r2, 2)
        violations, margin, pi_margin = violations + bad, min(margin, near), min(pi_margin, pi_near)
        out[f"cells.{which}"] = cells
        out.update({f"{which}.{name}.{plane}": v for (name, plane), v in planes.items()})
        members = planes[("one", "N")].sum()
        if members <= 1000:
            complaints.append(f"only {members:.0f} member pairs in the list {which}")
        for name in PI_SETS:
            if np.any(planes[(name, "N")].sum(axis=(1, 2)) == 0):
                complaints.append(f"a pi bin of the set {name} holds no pair in the list {which}")
        diagonal = cells[:, 3] != 0
        if not two and (planes[("one", "N")][:, diagonal].sum() == 0 or planes[("one", "N")][:, ~diagonal].sum() == 0):
            complaints.append("the diagonal or the off-diagonal cells hold no pair")
    if scene == "wide":
        for cat in (a, b):
            for k in range(2):
                least = min(cat["d"][int(cat["off"][s]):int(cat["off"][s + 1])].min() for s in range(k, len(cat["off"]) - 1, 2))
                assert 0.0095 <= r2[k, -1] / least**2 <= 0.00999, "the reach is not at the cap"
    out.update(margin=np.float64(margin), pi_margin=np.float64(pi_margin))
    return {f"{scene}.{k}": v for k, v in out.items()}, violations, complaints


def exact_pairs(cat, shears):
    """The known answer -> (arrays, pairs that break the condition, complaints)."""
    out = {"r2": PAIR_R2, "cells": PAIR_CELLS, "amplitude": np.float64(AMPLITUDE)}
    out.update({c: v for c, v in cat.items()})
    points = mp_points(cat)
    complaints = []
    for variant in VARIANTS:
        shaped = dict(cat, g1=shears[variant][0], g2=shears[variant][1])
        planes, violations, margin, pi_margin = exact_cells(shaped, shaped, points, points, PAIR_CELLS, PAIR_R2, 0)
        out.update({f"{variant}.g1": shaped["g1"], f"{variant}.g2": shaped["g2"]})
        out.update({f"{variant}.{name}.{plane}": v for (name, plane), v in planes.items()})
    per_cell = planes[("one", "N")].sum(axis=(0, 2))
    if not np.array_equal(per_cell, [len(sites) for sites in PAIR_SITES]):
        complaints.append(f"the cells hold {per_cell} member pairs")  # a partner outside the cut or the radii, or two pairs that meet
    # the known answer from the weights alone, e^2 W per element: the plane of each set of shears that holds it, the others zero
    for name in PI_SETS:
        known = AMPLITUDE**2 * out[f"along.{name}.W"]
        for variant, plane in zip(VARIANTS, SIGNED):
            for other in SIGNED:
                exact = out[f"{variant}.{name}.{other}"]
                assert np.all(np.abs(exact - (known if other == plane else 0.0)) <= 1e-15 * known), f"{variant} {name}: {other} is not the known answer"
    out.update(margin=np.float64(margin), pi_margin=np.float64(pi_margin))
    ra, dec = cat["ra"], cat["dec"]
    lo = 2 * POLE_PAIR
    assert pole_distance(ra[lo:lo + 2], dec[lo:lo + 2]) < 0.1 * DEG, "the pole pair's great circle misses the pole"
    lo = 2 * WRAP_PAIR
    assert ra[lo] > 6.0 and ra[lo + 1] < 0.1, "the wrap pair does not straddle the wrap"
    return {f"pairs.{k}": v for k, v in out.items()}, violations, complaints


# --------------------------------------------------------------------------- the oracle against the file: K
def oracle_planes(arrays, scene, which, name, weighted):
    """``proj_shape_oracle.proj_shape_cells`` on a scene of the file: (PP, XX, PX, W, A, N)."""
    import proj_shape_exact
    import proj_shape_oracle

    if scene == "pairs":
        a = b = proj_shape_exact.catalogue(arrays, scene, which, weighted)
    else:
        a = proj_shape_exact.catalogue(arrays, scene, "a", weighted)
        b = proj_shape_exact.catalogue(arrays, scene, "b", weighted) if which == "two" else a
    return proj_shape_oracle.proj_shape_cells(a, b, proj_shape_exact.cells(arrays, scene, which), arrays[f"{scene}.r2"], PI_SETS[name])


def write_design(K, worst):
    with open(DESIGN, encoding="utf-8") as fh:
        text = fh.read()
    marked = re.compile(r"(<!-- proj-shape-exact-K -->).*?(<!-- /proj-shape-exact-K -->)", re.S)
    if not marked.search(text):
        print("DESIGN.md has no proj-shape-exact-K markers: not updated")
        return
    new = marked.sub(lambda m: f"{m.group(1)}`K` = {K:g} (`K_measured`, the worst ratio of the numpy oracle, {worst:.3f}){m.group(2)}", text)
    if new != text:
        with open(DESIGN, "w", encoding="utf-8") as fh:
            fh.write(new)
    print(f"DESIGN.md: K = {K:g}")


def main():
    import proj_shape_exact

    started = time.time()
    rng = np.random.default_rng(SEED)
    arrays = {"eps": np.float64(proj_shape_exact.EPS), "pmax": np.float64(PMAX), "margin": np.float64(MARGIN)}
    arrays.update({f"pi.{name}": pe for name, pe in PI_SETS.items()})
    lists = {}
    for scene in ("as", "wide", "pairs"):
        draws = 0
        while True:
            draws += 1
            if scene == "pairs":
                part, violations, complaints = exact_pairs(*draw_pairs(rng))
            else:
                part, violations, complaints = exact_scene(scene, *draw(scene, rng), radii2(scene))
            if violations == 0 and not complaints:
                break
            print(f"{scene} draw {draws}: {violations} pairs within {MARGIN:g} of an edge" + "".join("; " + c for c in complaints) + ": drawing again")
        arrays.update(part)
        arrays[f"{scene}.draws"] = np.int32(draws)
        lists[scene] = VARIANTS if scene == "pairs" else ("two", "one")
        members = ", ".join(f"{which} {part[f'{scene}.{which}.one.N'].sum():.0f}" for which in lists[scene])
        print(f"{scene} draw {draws}: the condition holds, 0 pairs excluded; member pairs inside the cut: {members}; nearest radius edge "
              f"{part[f'{scene}.margin']:.2e} away, nearest edge in p {part[f'{scene}.pi_margin']:.2e}")
        for which in lists[scene]:
            for name in PI_SETS:
                got = oracle_planes(arrays, scene, which, name, False)
                if not (np.array_equal(got[5], arrays[f"{scene}.{which}.{name}.N"]) and np.array_equal(got[3], got[5])):
                    sys.exit(f"{scene} {which} {name}: the numpy oracle does not count the pairs of the exact reference: a finding about the contract")
    worst = 0.0
    for scene in ("as", "wide", "pairs"):
        for which in lists[scene]:
            for name in PI_SETS:
                got, exp = oracle_planes(arrays, scene, which, name, True), proj_shape_exact.expected(arrays, scene, which, name)
                np.testing.assert_allclose(got[4], exp["A"], rtol=1e-12, atol=0)
                ratios = [proj_shape_exact.worst_ratio(got[c], exp[plane], exp["Ath"]) for c, plane in enumerate(SIGNED)]
                print(f"{scene} {which} {name}: worst |oracle - exact| / (2^-52 Ath): " + ", ".join(f"{p} {r:.3f}" for p, r in zip(SIGNED, ratios)))
                worst = max(worst, *ratios)
    if worst > WORST_ALLOWED:
        sys.exit(f"the oracle's worst ratio is {worst:.3f} > {WORST_ALLOWED:g}: the reference or the oracle is wrong, not the tolerance")
    K = 2.0 ** int(np.ceil(np.log2(4.0 * worst)))
    print(f"mpmath {mpmath.__version__} at {mp.dps} digits; K_measured = {worst:.3f} -> K = {K:g}; {time.time() - started:.0f} s")
    arrays.update({"K": np.float64(K), "K_measured": np.float64(worst)})
    save(OUT, arrays)
    write_design(K, worst)


if __name__ == "__main__":
    main()
