#!/usr/bin/env python3
"""Generate ``tests/golden/dsigma_radial_exact.npz``: an exact reference of the excess-surface-density count binned in each
lens's own radius (``yawhip_dsigma_count_radial``) from arcseconds up to the cap of its reach, 5.73 degrees.

Runs on the CPU with ``mpmath`` at 50 digits; no GPU, no reference package. The arithmetic of a pair is that of
tools/make_golden_shear_exact.py, imported from there (``Point``, ``chord2``, ``separation``, ``double_angle``,
``tangential_terms``, ``lensing_factor``; the scenes are drawn with its ``ring_around`` and ``log_uniform`` and the file is
written by its ``save``). Per pair the tool takes the float64 ``(ra, dec)`` of both ends and the float64 columns ``m, w, f, c,
u, g1, g2``, computes ``theta = 2 asin(chord / 2)`` and ``R2 = m_l theta^2`` exactly, and tests ``r2[k][e] < R2 <= r2[k][e+1]``
against the float64 edges taken exactly. NOTHING here evaluates the contract's series of the squared angle: what the file says
about a pair's bin is what ``D(z_l) theta`` says. (The two deliberately WRONG squared angles below -- the chord itself, and the
chord with the one term ``s2 / 12`` -- are there to count the pairs that tell them from the right one.)

Scenes (a site is a patch of its own; jobs (p, p) and two jobs between sites, which hold nothing):
  as     the five sites of the shear file (dec 0, 60, +-89.99 degrees, the wrap of the right ascension): 30 lenses inside 1" of
         every site in two redshift bins, 14 sources per site on rings of 0.5" ... 30"; ``m = D^2`` with ``D`` drawn per lens
         from 600 ... 2500, so that neighbours in any sort order differ by up to a factor 17 in ``m``; two rows of 6 log-spaced
         radius bins, 0.004 ... 0.12 and 0.005 ... 0.15, whose end edges both cut through the pairs of every site
  wide   sites at dec 0 and 60 degrees, one at 86 degrees whose rings pass over the pole, one whose partners straddle the wrap:
         10 lenses inside 2" of every site in two bins, 60 sources per site log-uniform from 3' to 5.6 degrees and 14 placed
         ones (below); rows of 6 log-spaced bins 0.2 ... 2 and 0.25 ... 2; the first lens of every segment has ``r2max / m``
         between 0.0095 and 0.00999 -- the call is accepted AT the cap of 0.01 -- and the others reach 1.3 to 4 times less far
         in angle

Per cell the file holds ``N`` (the integer number of pairs), the exact ``T, X, W`` rounded once, ``A`` and ``A_theta``
(tests/shear_exact.py), for the columns ``f, c, u`` of the file and for those of the shear driver (``f = 1, c = 0, u = 0``:
prefix ``sh.``), with the lenses in their two bins and folded into one bin under both rows (prefix ``fold.``: every lens is then
binned by both rows); and per member pair (two bins) its terms, its ``R2``, its bin and its distance from the nearest edge.

Conditions, asserted; the inputs are redrawn until they hold, so that no pair is left out of any comparison:
  * no pair's exact ``R2`` within a relative 1e-6 (as) / 1e-9 (wide) of ANY edge of either row, no ``|1 - c u| < 1e-6``
  * wide: at least 8 member pairs whose bin changes when ``theta^2`` is replaced by the chord ``s2`` (``wide.by_chord``) and 8
    when the series stops after ``s2 / 12`` (``wide.by_cut``) -- sources placed at ``theta^2 = r2[5] / m_l (1 + half the
    term)`` around the first lens of every segment (both wrong angles are too small, so only that side of an edge tells) --
    and per row at least 8 pairs with ``m s2 <= r2max < R2`` (``wide.not_capped``: they pass the kernel's outer test and have
    no bin), placed at ``theta^2 = r2max / m_l (1 + s2 / 24)``
  * in both scenes at least a quarter of the member pairs change their bin, or leave the row, when the ``m`` of their lens is
    replaced by the median ``m`` of its segment
  * the pair counts of the mirror oracle (tests/dsigma_radial_oracle.py) with unit columns are ``N``, cell for cell. A
    mismatch is a finding about the contract: the tool prints the pairs and stops; it does not draw again.

``K`` of the tolerance is measured as in the shear file: four times the worst ``|numpy radial oracle - exact| / (eps A_theta)``
over the file, rounded up to a power of two; it goes into the file and into DESIGN.md (between the ``radial-exact-K`` markers).

Running it again reproduces the file byte for byte.

Usage:  python tools/make_golden_dsigma_radial_exact.py
"""
from __future__ import annotations

import collections
import os
import re
import sys

import mpmath
import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (HERE, ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

from make_golden_shear_exact import (ARCSEC, DEG, SITES, Point, chord2, double_angle, lensing_factor, log_uniform,  # noqa: E402
                                     ring_around, save, separation, tangential_terms)

OUT = os.path.join(ROOT, "tests", "golden", "dsigma_radial_exact.npz")
DESIGN = os.path.join(ROOT, "DESIGN.md")
mp.dps = 50
SEED = 20261020
ARCMIN = 60.0 * ARCSEC
WIDE_SITES = [(1.0, 0.0), (2.1, 60.0 * DEG), (3.3, 86.0 * DEG), (2.0 * np.pi - 1e-7, 0.5)]
EDGE_MARGIN = {"as": 1e-6, "wide": 1e-9}
CLIP_MARGIN = 1e-6
S2_CAP = 0.01
N_SENTINELS = 8
PLACED = (("chord", 2), ("cut", 2), ("cap", 3))  # placed sources per first lens of a segment
PLANES = ("T", "X", "W")


def radii2(scene):
    rows = {"as": ((0.004, 0.12), (0.005, 0.15)), "wide": ((0.2, 2.0), (0.25, 2.0))}[scene]
    return np.array([np.geomspace(lo, hi, 7) for lo, hi in rows]) ** 2


def jobs_of(n_sites):
    return np.array([(p, p) for p in range(n_sites)] + [(0, 1), (n_sites - 1, n_sites - 2)], dtype=np.int32)


# --------------------------------------------------------------------------- scenes
def columns(rng, n_l, n_s):
    """Weights, shears and the lensing columns of tools/make_golden_shear_exact.py: about half the pairs have the source in front."""
    c = rng.uniform(600.0, 2500.0, n_l)
    lens = dict(w=rng.uniform(0.5, 2.0, n_l), f=c / rng.uniform(1.2, 1.9, n_l), c=c)
    src = dict(w=rng.uniform(0.5, 2.0, n_s), g1=rng.normal(0.0, 0.3, n_s), g2=rng.normal(0.0, 0.3, n_s), u=1.0 / rng.uniform(600.0, 2500.0, n_s))
    return lens, src


def draw_as(rng):
    n_lens, n_src = 30, 14
    lens_pos, src_pos = [], []
    for ra_c, dec_c in SITES:
        lens_pos.append(ring_around(rng, ra_c, dec_c, 1.0 * ARCSEC * np.sqrt(rng.uniform(0.0, 1.0, n_lens))))
        src_pos.append(ring_around(rng, ra_c, dec_c, log_uniform(rng, 0.5, 30.0, n_src) * ARCSEC))
    n_l, n_s = n_lens * len(SITES), n_src * len(SITES)
    lens, src = columns(rng, n_l, n_s)
    lens.update(ra=np.concatenate([p[0] for p in lens_pos]), dec=np.concatenate([p[1] for p in lens_pos]),
                m=rng.uniform(600.0, 2500.0, n_l) ** 2, off=np.arange(0, n_l + 1, n_lens // 2, dtype=np.int64))
    src.update(ra=np.concatenate([p[0] for p in src_pos]), dec=np.concatenate([p[1] for p in src_pos]),
               off=np.arange(0, n_s + 1, n_src, dtype=np.int64))
    return lens, src


def draw_wide(rng):
    """The first lens of every segment reaches the cap; around it sources are placed just beyond the edge ``r2[k][5]`` (by half
    the first, and by half the second term of ``theta^2 / s2 - 1 = s2 / 12 + s2^2 / 90 + ...``) and just beyond the last edge."""
    n_lens, n_src = 10, 60
    per_bin = n_lens // 2
    r2 = radii2("wide")
    lens_ra, lens_dec, lens_m, src_ra, src_dec = [], [], [], [], []
    for ra_c, dec_c in WIDE_SITES:
        ra_l, dec_l = ring_around(rng, ra_c, dec_c, 2.0 * ARCSEC * np.sqrt(rng.uniform(0.0, 1.0, n_lens)))
        m = np.empty(n_lens)
        for k in range(2):
            first = r2[k, -1] / rng.uniform(0.0095, 0.00999)
            m[k * per_bin:(k + 1) * per_bin] = first * np.concatenate([[1.0], log_uniform(rng, 1.3, 4.0, per_bin - 1) ** 2])
        ra, dec = ring_around(rng, ra_c, dec_c, log_uniform(rng, 3.0 * ARCMIN, 5.6 * DEG, n_src))
        placed_ra, placed_dec = [ra], [dec]
        for k in range(2):
            i = k * per_bin
            at_edge, at_end = r2[k, 5] / m[i], r2[k, 6] / m[i]
            theta2 = {"chord": at_edge * (1.0 + at_edge / 24.0), "cut": at_edge * (1.0 + at_edge * at_edge / 180.0),
                      "cap": at_end * (1.0 + at_end / 24.0)}
            for kind, count in PLACED:
                ra, dec = ring_around(rng, ra_l[i], dec_l[i], np.full(count, np.sqrt(theta2[kind])))
                placed_ra.append(ra), placed_dec.append(dec)
        lens_ra.append(ra_l), lens_dec.append(dec_l), lens_m.append(m)
        src_ra.append(np.concatenate(placed_ra)), src_dec.append(np.concatenate(placed_dec))
    n_l = n_lens * len(WIDE_SITES)
    sizes = [len(a) for a in src_ra]
    lens, src = columns(rng, n_l, sum(sizes))
    lens.update(ra=np.concatenate(lens_ra), dec=np.concatenate(lens_dec), m=np.concatenate(lens_m),
                off=np.arange(0, n_l + 1, per_bin, dtype=np.int64))
    src.update(ra=np.concatenate(src_ra), dec=np.concatenate(src_dec), off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    return lens, src


# --------------------------------------------------------------------------- exact arithmetic
def bin_of(R2, edges):
    """``e`` with ``edges[e] < R2 <= edges[e + 1]`` (exact numbers), or None."""
    if not (R2 > edges[0] and R2 <= edges[-1]):
        return None
    return sum(1 for edge in edges if R2 > edge) - 1


def exact_scene(scene, lens, src, r2):
    """Every pair of the jobs -> (arrays of the scene, number of pairs that break a condition)."""
    n_sites = len(src["off"]) - 1
    jobs = jobs_of(n_sites)
    n_rows, nf = r2.shape[0], r2.shape[1] - 1
    edges = [[mpf(float(e)) for e in row] for row in r2]
    every_edge = [e for row in edges for e in row]
    lens_points = [Point(r, d) for r, d in zip(lens["ra"], lens["dec"])]
    src_points = [Point(r, d) for r, d in zip(src["ra"], src["dec"])]
    wg1, wg2 = src["w"] * src["g1"], src["w"] * src["g2"]  # the rounded float64 products a handle stores
    xyz_l = np.array([[float(p.x), float(p.y), float(p.z)] for p in lens_points])
    xyz_s = np.array([[float(p.x), float(p.y), float(p.z)] for p in src_points])
    segment = np.searchsorted(lens["off"], np.arange(len(lens["ra"])), side="right") - 1
    median = np.array([np.median(lens["m"][lens["off"][s]:lens["off"][s + 1]]) for s in range(len(lens["off"]) - 1)])

    sums = collections.defaultdict(lambda: mpf(0))  # (fold, columns, plane, job, row, bin)
    shape = (len(jobs), n_rows, nf)
    N = {fold: np.zeros(shape) for fold in (False, True)}
    mags = {(fold, cols, which): np.zeros(shape) for fold in (False, True) for cols in ("ds", "sh") for which in ("A", "Ath")}
    pairs, by_chord, by_cut, not_capped = [], [], [], []
    outside = np.zeros((n_sites, n_rows, 2), dtype=np.int64)  # pairs below the first / above the last edge of the lens's row
    violations, worst_margin = 0, np.inf
    for job, (p, q) in enumerate(jobs):
        for i in range(int(lens["off"][2 * p]), int(lens["off"][2 * p + 2])):
            k_own = int(segment[i]) % 2
            m = mpf(float(lens["m"][i]))
            m_median = mpf(float(median[segment[i]]))
            for j in range(int(src["off"][q]), int(src["off"][q + 1])):
                if p != q:  # two sites: recognised in float64 (a factor 4 in the squared chord against errors of 1e-16)
                    assert ((xyz_l[i] - xyz_s[j]) ** 2).sum() * lens["m"][i] > 4.0 * r2.max()
                    continue
                a, b = lens_points[i], src_points[j]
                c2 = chord2(a, b)
                theta = separation(c2)
                R2 = m * theta * theta
                margin = min(abs(R2 / e - 1) for e in every_edge)
                worst_margin = min(worst_margin, float(margin))
                violations += margin < EDGE_MARGIN[scene]
                bins = [bin_of(R2, edges[k]) for k in range(n_rows)]
                outside[p, k_own] += (R2 <= edges[k_own][0], R2 > edges[k_own][-1])
                for k in range(n_rows):
                    if m * c2 <= edges[k][-1] < R2:
                        not_capped.append((i, j, k))
                if all(e is None for e in bins):
                    continue
                cos2, sin2 = double_angle(b, a)  # the lens seen from the source
                tv, xv = tangential_terms(lens["w"][i], wg1[j], wg2[j], cos2, sin2)
                wv = mpf(float(lens["w"][i])) * mpf(float(src["w"][j]))
                mag = abs(lens["w"][i] * src["w"][j]) * (abs(src["g1"][j]) + abs(src["g2"][j]))
                eff, s = lensing_factor(lens["f"][i], lens["c"][i], src["u"][j])
                violations += abs(eff) < CLIP_MARGIN
                terms = {"sh": (tv, xv, wv, mag), "ds": (tv * s, xv * s, wv * s * s, mag * float(s)) if s > 0 else None}
                for k, e in enumerate(bins):
                    if e is None:
                        continue
                    for fold in ((False, True) if k == k_own else (True,)):
                        N[fold][job, k, e] += 1
                        for cols, values in terms.items():
                            if values is None:
                                continue
                            for plane, v in zip(PLANES, values[:3]):
                                sums[(fold, cols, plane, job, k, e)] += v
                            mags[(fold, cols, "A")][job, k, e] += values[3]
                            mags[(fold, cols, "Ath")][job, k, e] += values[3] / float(theta)
                e = bins[k_own]
                if e is None:
                    continue
                moved = bin_of(m_median * theta * theta, edges[k_own]) != e
                ds = terms["ds"]
                pairs.append((i, j, float(ds[0]) if ds else 0.0, float(ds[1]) if ds else 0.0, float(R2), e, float(margin), moved))
                if bin_of(m * c2, edges[k_own]) != e:
                    by_chord.append((i, j))
                if bin_of(m * (c2 * (1 + c2 / 12)), edges[k_own]) != e:
                    by_cut.append((i, j))
    out = {"r2": r2, "n_patches": np.int32(n_sites), "jobs": jobs, "margin": np.float64(worst_margin)}
    out.update({f"lens.{c}": v for c, v in lens.items()})
    out.update({f"src.{c}": v for c, v in src.items()})
    for fold in (False, True):
        head = "fold." if fold else ""
        out[head + "N"] = N[fold]
        for cols in ("ds", "sh"):
            mid = head + ("sh." if cols == "sh" else "")
            for plane in PLANES:
                out[mid + plane] = np.array([[[float(sums[(fold, cols, plane, job, k, e)]) for e in range(nf)] for k in range(n_rows)]
                                             for job in range(len(jobs))])
            out[mid + "A"], out[mid + "Ath"] = mags[(fold, cols, "A")], mags[(fold, cols, "Ath")]
    out["pairs"] = np.array([(i, j) for i, j, *_ in pairs], dtype=np.int32).reshape(-1, 2)
    for c, (name, dtype) in enumerate((("T", np.float64), ("X", np.float64), ("R2", np.float64), ("bin", np.int8),
                                       ("margin", np.float32), ("moved", np.bool_)), start=2):
        out[f"pair_{name}"] = np.array([row[c] for row in pairs], dtype=dtype)
    out["by_chord"] = np.array(by_chord, dtype=np.int32).reshape(-1, 2)
    out["by_cut"] = np.array(by_cut, dtype=np.int32).reshape(-1, 2)
    out["not_capped"] = np.array(not_capped, dtype=np.int32).reshape(-1, 3)
    out["outside"] = outside
    return {f"{scene}.{k}": v for k, v in out.items()}, int(violations)


def conditions(scene, arrays):
    """The conditions a draw can miss besides the margins -> list of complaints (empty: the draw is good)."""
    get = lambda name: arrays[f"{scene}.{name}"]  # noqa: E731
    complaints = []
    if get("pair_moved").mean() < 0.25:
        complaints.append(f"the median m moves only {get('pair_moved').mean():.2f} of the member pairs")
    if np.any(get("N")[:get("n_patches")].sum(axis=2) == 0):
        complaints.append("a row of a site holds no pair")
    if scene == "as" and np.any(get("outside") == 0):
        complaints.append("an end edge does not cut through the pairs of a site")
    if scene == "wide":
        per_row = np.bincount(get("not_capped")[:, 2], minlength=2)
        if len(get("by_chord")) < N_SENTINELS or len(get("by_cut")) < N_SENTINELS or per_row.min() < N_SENTINELS:
            complaints.append(f"sentinels: {len(get('by_chord'))} by chord, {len(get('by_cut'))} by cut, {per_row} not capped")
        m, off, r2 = get("lens.m"), get("lens.off"), get("r2")
        for k in range(2):
            reach = r2[k, -1] / min(m[off[s]:off[s + 1]].min() for s in range(k, len(off) - 1, 2))
            if not (0.0095 <= reach and reach * (1.0 + 1e-12) <= S2_CAP):
                complaints.append(f"row {k}: the nearest lens reaches {reach}")
        if r2[:, -1].max() / m.min() * (1.0 + 1e-12) > S2_CAP:
            complaints.append("folded into one bin the call is refused")
        ra_s, dec_s = get("src.ra"), get("src.dec")
        pole, wrap = slice(*get("src.off")[2:4]), slice(*get("src.off")[3:5])
        if not np.any(np.cos(ra_s[pole] - WIDE_SITES[2][0]) < 0.0) or min(np.sum(ra_s[wrap] < 1.0), np.sum(ra_s[wrap] > 5.0)) < 10:
            complaints.append("no ring over the pole, or no partners on both sides of the wrap")
        assert dec_s.max() < np.pi / 2
    return complaints


# --------------------------------------------------------------------------- the mirror oracle against the file
def oracle_inputs(arrays, scene, cols, fold=False):
    import dsigma_radial_exact as dre

    return dre.scene(arrays, scene, cols, fold)


def compare_counts(arrays, scene):
    """The mirror oracle's pair counts against ``N``; a mismatch prints the pairs whose float64 bin is not the exact one."""
    import dsigma_radial_oracle as oracle

    ok = True
    for fold in (False, True):
        lens, src = oracle_inputs(arrays, scene, "unit", fold)
        W = oracle.radial_jobs(lens, src, arrays[f"{scene}.jobs"], arrays[f"{scene}.r2"])[2]
        ok &= bool(np.array_equal(W, arrays[f"{scene}.{'fold.' if fold else ''}N"]))
    if ok:
        return True
    lens, src = oracle_inputs(arrays, scene, "unit")
    r2 = arrays[f"{scene}.r2"]
    member = {(int(i), int(j)): int(e) for (i, j), e in zip(arrays[f"{scene}.pairs"], arrays[f"{scene}.pair_bin"])}
    for p in range(int(arrays[f"{scene}.n_patches"])):
        for i in range(int(lens["off"][2 * p]), int(lens["off"][2 * p + 2])):
            k = int(np.searchsorted(lens["off"], i, side="right") - 1) % 2
            for j in range(int(src["off"][p]), int(src["off"][p + 1])):
                d = [src[c][j] - lens[c][i] for c in "xyz"]
                R2 = lens["m"][i] * oracle.squared_angle((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                e = int((R2 > r2[k]).sum()) - 1 if r2[k, 0] < R2 <= r2[k, -1] else -1
                if e != member.get((i, j), -1):
                    print(f"{scene}: lens {i} source {j} row {k}: the contract's R2 = {R2!r} falls into bin {e}, the exact one into {member.get((i, j), -1)}")
    return False


def oracle_ratios(arrays):
    """Worst ``|oracle - exact| / (eps A_theta)`` of the numpy radial oracle per scene and set of columns."""
    import dsigma_radial_exact as dre
    import dsigma_radial_oracle as oracle
    import shear_exact as se

    out = {}
    for scene in ("as", "wide"):
        for cols in ("real", "shear"):
            for fold in (False, True):
                lens, src = dre.scene(arrays, scene, cols, fold)
                got = oracle.radial_jobs(lens, src, arrays[f"{scene}.jobs"], arrays[f"{scene}.r2"])
                prefix = dre.prefix(scene, cols, fold)
                out[prefix] = max(se.worst_ratio(got[c], arrays[f"{prefix}.{n}"], arrays[f"{prefix}.A"], arrays[f"{prefix}.Ath"])
                                  for c, n in enumerate("TX"))
                np.testing.assert_allclose(got[2], arrays[f"{prefix}.W"], rtol=se.RTOL_W, atol=0)
    return out


def write_design(K, worst):
    with open(DESIGN, encoding="utf-8") as fh:
        text = fh.read()
    marked = re.compile(r"(<!-- radial-exact-K -->).*?(<!-- /radial-exact-K -->)", re.S)
    if not marked.search(text):
        print("DESIGN.md has no radial-exact-K markers: not updated")
        return
    new = marked.sub(lambda m: f"{m.group(1)}`K` = {K:g} (worst measured ratio of the numpy radial oracle {worst:.3f}){m.group(2)}", text)
    if new != text:
        with open(DESIGN, "w", encoding="utf-8") as fh:
            fh.write(new)
    print(f"DESIGN.md: K = {K:g}")


def main():
    rng = np.random.default_rng(SEED)
    arrays = {"eps": np.float64(2.0**-52)}
    for scene, draw in (("as", draw_as), ("wide", draw_wide)):
        draws = 0
        while True:
            draws += 1
            lens, src = draw(rng)
            part, violations = exact_scene(scene, lens, src, radii2(scene))
            complaints = conditions(scene, part)
            if violations == 0 and not complaints:
                break
            print(f"{scene} draw {draws}: {violations} pairs within {EDGE_MARGIN[scene]:g} of an edge or {CLIP_MARGIN:g} of the clip"
                  + "".join("; " + c for c in complaints) + ": drawing again")
        arrays.update(part)
        arrays[f"{scene}.draws"] = np.int32(draws)
        print(f"{scene} draw {draws}: every condition holds, 0 pairs excluded; {len(part[f'{scene}.pairs'])} member pairs, nearest edge "
              f"{part[f'{scene}.margin']:.2e} away; the median m of its segment would move {part[f'{scene}.pair_moved'].mean():.3f} of them")
        if scene == "wide":
            per_row = np.bincount(part["wide.not_capped"][:, 2], minlength=2)
            print(f"wide sentinels: {len(part['wide.by_chord'])} member pairs change their bin by the chord, {len(part['wide.by_cut'])} by the series "
                  f"cut after s2 / 12, {per_row[0]} + {per_row[1]} pairs pass m s2 <= r2max with R2 beyond it")
        if not compare_counts(arrays, scene):
            sys.exit(f"{scene}: the mirror oracle does not count the pairs of the exact reference: a finding about the contract")
    print(f"mpmath {mpmath.__version__} at {mp.dps} digits; the mirror oracle counts N in every cell, in two bins and folded")
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
