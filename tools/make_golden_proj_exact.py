#!/usr/bin/env python3
"""Generate ``tests/golden/proj_exact.npz``: an exact reference of the two projected pair counts (``yawhip_proj_count`` and
``yawhip_proj_count_pi``, DESIGN.md sections 20 and 22) from arcseconds up to the cap of their reach, 5.73 degrees.

Runs on the CPU with ``mpmath`` at 50 digits; no GPU, no reference package. The arithmetic of a pair is that of
tools/make_golden_shear_exact.py, imported from there (``Point``, ``chord2``, ``separation``; the scenes are drawn with its
``ring_around`` and ``log_uniform`` and the file is written by its ``save``). Per pair the tool takes the float64 ``(ra, dec)``
of both ends and the float64 columns ``d, c, w``, computes ``theta = 2 asin(chord / 2)``, ``R2 = ((d_a + d_b) / 2)^2 theta^2`` and
``p = |c_a - c_b|`` exactly, and tests ``r2[row][e] < R2 <= r2[row][e + 1]``, ``p <= pmax`` and ``pe[j] < p <= pe[j + 1]`` against
the float64 edges taken exactly. NOTHING here evaluates the contract's series of the squared angle: what the file says about
a pair's bin is what ``D theta`` says. (The two deliberately WRONG squared angles below -- the chord itself, and the chord with
the one term ``s2 / 12`` -- and the wrong distance ``d_a`` are there to count the pairs that tell them from the right ones.)

Scenes: two catalogues ``a`` and ``b``; every site has two patches over the same area and two redshift bins per patch; the
cells of tests/proj_scenes.py (``cells_one_handle``: every diagonal cell and the two patches of a site against each other;
``cells_two_handles``: ``a`` against ``b``) and two cells between different sites, which hold nothing; row = bin.
  as     the five sites of the shear file (dec 0, 60, +-89.99 degrees, the wrap of the right ascension): 14 objects per segment
         on rings of 0.5" ... 30" around the site, ``d`` drawn per object from 600 ... 2500, so that neighbours in any sort
         order differ by up to a factor 4 in ``d``; ``c`` 0 ... 120, ``pmax`` 40; two rows of 6 log-spaced radius bins,
         0.004 ... 0.12 and 0.005 ... 0.15, whose end edges both cut through the pairs of every site
  wide   sites at dec 0 and 60 degrees, one at 86 degrees whose rings pass over the pole, one whose partners straddle the wrap:
         20 objects per segment, log-uniform from 3' to 5.6 degrees around the site; rows of 6 log-spaced bins 0.2 ... 2 and
         0.25 ... 2; in every (catalogue, bin) the least ``d`` has ``r2max / least^2`` between 0.0095 and 0.00999 -- the call is
         accepted AT the cap of 0.01 -- a few "near" objects lie within 2 % of it (an anchor next to every site in ``a``, and
         the partners placed around it, below) and the others are 1.3 to 4 times farther
In every segment one pair of objects lies 1e-4 ... 4e-4 apart in ``c``, one inside the narrow pi bin and one at the same ``c``.

Three sets of pi edges are stored (``pi.one``: ``[0, 40]``; ``pi.four``: four equal bins; ``pi.uneven``: 8 bins, the first edge
5e-4, one bin 0.03 wide). Per scene, cell list (``one``, ``two``) and for the bins as uploaded and folded into one bin under
both rows (prefix ``fold.``: the cells of ``nb = 1`` once per row) the file holds ``N`` (the integer member pairs inside the
cut), ``N_pi.<set>`` f64[n_pi, cells, nf], and for the stored weights the exact ``W``, ``A = sum |w_a w_b|`` and ``W_pi.<set>``,
each rounded once (every weight is > 0, so the ``A`` of a plane is its ``W_pi``). Per-pair records exist only for the sentinels.

Conditions, asserted; the inputs are redrawn until they hold, so that no pair is left out of any comparison:
  * no pair's exact ``R2`` within a relative 1e-6 (as) / 1e-9 (wide) of ANY edge of either row; no ``p`` within a relative
    1e-9 of ``pmax`` or of any pi edge of any set
  * wide: at least 8 member pairs whose bin changes when ``theta^2`` is replaced by the chord ``s2`` (``wide.by_chord``) and 8
    when the series stops after ``s2 / 12`` (``wide.by_cut``) -- partners placed at ``theta^2 = r2[5] / DD (1 + half the
    term)`` around the anchors (both wrong angles are too small, so only that side of an edge tells) -- and per row at least
    8 pairs with ``DD s2 <= r2max < R2`` (``wide.not_capped``: they pass the kernel's outer test and have no bin), placed at
    ``theta^2 = r2max / DD (1 + s2 / 24)``, at least 4 of them inside the cut in ``p`` and 4 beyond it
  * in both scenes at least a quarter of the member pairs change their bin, or leave the row, when the pair's ``D`` is
    replaced by the ``d`` of its first object alone
  * every pi plane of the uneven set holds a pair in some scene; over each set the planes sum to ``N``; more than 1000 member
    pairs per scene and cell list
  * the mirror oracles with unit weights give the file's counts cell for cell (tests/proj_oracle.py ``N``,
    tests/proj_pi_oracle.py ``N_pi``). A mismatch is a finding about the contract: the tool prints the pairs and stops; it
    does not draw again.

``K`` of the tolerance is four times the worst ``|mirror oracle - exact| / (2^-53 A)`` over all weighted planes of the file,
rounded up to a power of two; it goes into the file and into DESIGN.md (between the ``proj-exact-K`` markers).

Running it again reproduces the file byte for byte.

Usage:  python tools/make_golden_proj_exact.py
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

from make_golden_dsigma_radial_exact import WIDE_SITES, bin_of  # noqa: E402
from make_golden_shear_exact import ARCSEC, DEG, SITES, Point, chord2, log_uniform, ring_around, save, separation  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "proj_exact.npz")
DESIGN = os.path.join(ROOT, "DESIGN.md")
mp.dps = 50
SEED = 20261021
ARCMIN = 60.0 * ARCSEC
EDGE_MARGIN = {"as": 1e-6, "wide": 1e-9}
PI_MARGIN = 1e-9
S2_CAP = 0.01
PMAX = 40.0
N_SENTINELS = 8
PER_SEGMENT = {"as": 14, "wide": 20}
PLACED = (("chord", 2), ("cut", 2), ("cap", 3))  # placed partners per anchor and target segment
PI_SETS = {"one": np.array([0.0, PMAX]), "four": np.linspace(0.0, PMAX, 5),
           "uneven": np.array([0.0, 5e-4, 0.3, 0.33, 2.0, 7.0, 15.0, 26.0, PMAX])}
SITES_OF = {"as": SITES, "wide": WIDE_SITES}


def radii2(scene):
    rows = {"as": ((0.004, 0.12), (0.005, 0.15)), "wide": ((0.2, 2.0), (0.25, 2.0))}[scene]
    return np.array([np.geomspace(lo, hi, 7) for lo, hi in rows]) ** 2


# --------------------------------------------------------------------------- scenes
def engineer_c(rng, c, start):
    """Objects ``start .. start + 5`` of a segment: one pair below the first pi edge of the uneven set, one inside its narrow
    bin, one at the same ``c``."""
    c[start + 1] = c[start] + rng.uniform(1e-4, 4e-4)
    c[start + 3] = c[start + 2] + rng.uniform(0.305, 0.325)
    c[start + 5] = c[start + 4]


def catalogue(segments):
    """Segments [(ra, dec, d, c)] in the order patch * 2 + bin -> the columns of a catalogue without its weights."""
    sizes = [len(seg[0]) for seg in segments]
    out = {name: np.concatenate([seg[n] for seg in segments]) for n, name in enumerate(("ra", "dec", "d", "c"))}
    out["off"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return out


def draw_as(rng):
    per = PER_SEGMENT["as"]
    cats = {}
    for cat in "ab":
        segments = []
        for ra_c, dec_c in SITES:
            for _ in range(4):  # two patches over the same area, two bins each
                ra, dec = ring_around(rng, ra_c, dec_c, log_uniform(rng, 0.5, 30.0, per) * ARCSEC)
                c = rng.uniform(0.0, 120.0, per)
                engineer_c(rng, c, 0)
                segments.append((ra, dec, rng.uniform(600.0, 2500.0, per), c))
        cats[cat] = catalogue(segments)
        cats[cat]["w"] = rng.uniform(0.5, 2.0, len(cats[cat]["ra"]))
    return cats["a"], cats["b"]


def draw_wide(rng):
    """In ``a`` the first object of the segments (patch 2 s, bin k) is an anchor within 2" of its site, as near as the bin's
    least ``d`` allows; around it partners are placed in (patch 2 s + 1, bin k) of ``a`` and in (patch 2 s, bin k) of ``b``,
    as near themselves: just beyond the edge ``r2[k][5]`` (by half the first, and by half the second term of ``theta^2 / s2 -
    1 = s2 / 12 + s2^2 / 90 + ...``) and just beyond the last edge, alternately inside the cut in ``p`` and beyond it."""
    per = PER_SEGMENT["wide"]
    n_placed = sum(count for _, count in PLACED)
    r2 = radii2("wide")
    least = {(cat, k): np.sqrt(r2[k, -1] / rng.uniform(0.0095, 0.00999)) for cat in "ab" for k in range(2)}
    segments = {cat: [None] * (4 * len(WIDE_SITES)) for cat in "ab"}
    beyond_cut = 0
    for site, (ra_c, dec_c) in enumerate(WIDE_SITES):
        for k in range(2):
            (ra_0,), (dec_0,) = ring_around(rng, ra_c, dec_c, 2.0 * ARCSEC * np.sqrt(rng.uniform(0.0, 1.0, 1)))
            d_0 = least["a", k] * (1.0 if site == 0 else rng.uniform(1.0, 1.02))
            c_0 = rng.uniform(30.0, 90.0)
            for cat, patch in (("a", 2 * site), ("a", 2 * site + 1), ("b", 2 * site), ("b", 2 * site + 1)):
                head = [(ra_0, dec_0, d_0, c_0)] if (cat, patch) == ("a", 2 * site) else []
                if (cat, patch) in (("a", 2 * site + 1), ("b", 2 * site)):
                    for kind, count in PLACED:
                        for _ in range(count):
                            d = least[cat, k] * (1.0 if (site == 0 and not head) else rng.uniform(1.0, 1.02))
                            DD = (0.5 * (d_0 + d)) ** 2
                            at_edge, at_end = r2[k, 5] / DD, r2[k, 6] / DD
                            theta2 = {"chord": at_edge * (1.0 + at_edge / 24.0), "cut": at_edge * (1.0 + at_edge * at_edge / 180.0),
                                      "cap": at_end * (1.0 + at_end / 24.0)}[kind]
                            (ra,), (dec,) = ring_around(rng, ra_0, dec_0, np.array([np.sqrt(theta2)]))
                            far = kind == "cap" and beyond_cut % 2 == 1
                            beyond_cut += kind == "cap"
                            delta = rng.uniform(45.0, 70.0) if far else rng.uniform(5.0, 35.0)
                            head.append((ra, dec, d, c_0 + delta if c_0 + delta <= 120.0 else c_0 - delta))
                n = per - len(head)
                ra, dec = ring_around(rng, ra_c, dec_c, log_uniform(rng, 3.0 * ARCMIN, 5.6 * DEG, n))
                c = rng.uniform(0.0, 120.0, n)
                engineer_c(rng, c, 0)
                d = least[cat, k] * log_uniform(rng, 1.3, 4.0, n)
                cols = [np.concatenate([[h[col] for h in head], rest]) for col, rest in enumerate((ra, dec, d, c))]
                segments[cat][patch * 2 + k] = tuple(cols)
    assert n_placed + 6 <= per
    cats = {cat: catalogue(segments[cat]) for cat in "ab"}
    for cat in "ab":
        cats[cat]["w"] = rng.uniform(0.5, 2.0, len(cats[cat]["ra"]))
    return cats["a"], cats["b"]


# --------------------------------------------------------------------------- exact arithmetic
def pi_plane(p, edges):
    """``j`` with ``p`` in plane j of the exact edges (plane 0 is ``[0, pe[1]]``, plane j ``(pe[j], pe[j + 1]]``), or None."""
    j = sum(1 for edge in edges[1:] if p > edge)
    return j if j < len(edges) - 1 else None


class Pairs:
    """Everything exact about a pair of objects, computed once: ``(R2, c2, DD, DD of the first object alone, p, bins per row,
    plane per set, inside the cut, w_a w_b)``. ``two``: object ``i`` of ``a`` with ``j`` of ``b``; else both of ``a``, ``i > j``."""

    def __init__(self, scene, a, b, r2):
        self.scene = scene
        self.cats = (a, b)
        self.points = [[Point(r, d) for r, d in zip(cat["ra"], cat["dec"])] for cat in (a, b)]
        self.edges = [[mpf(float(e)) for e in row] for row in r2]
        self.every_edge = [e for row in self.edges for e in row]
        self.pi_edges = {name: [mpf(float(e)) for e in pe] for name, pe in PI_SETS.items()}
        self.every_pi_edge = sorted({e for pe in self.pi_edges.values() for e in pe if e > 0})
        self.pmax = mpf(PMAX)
        self.records = {}
        self.violations = 0
        self.margin, self.pi_margin = np.inf, np.inf

    def get(self, two, i, j):
        key = (two, i, j)
        rec = self.records.get(key)
        if rec is not None:
            return rec
        first, second = self.cats[0], self.cats[1 if two else 0]
        c2 = chord2(self.points[0][i], self.points[1 if two else 0][j])
        theta = separation(c2)
        d_i, d_j = mpf(float(first["d"][i])), mpf(float(second["d"][j]))
        DD = ((d_i + d_j) / 2) ** 2
        R2 = DD * theta * theta
        p = abs(mpf(float(first["c"][i])) - mpf(float(second["c"][j])))
        margin = float(min(abs(R2 / e - 1) for e in self.every_edge))
        pi_margin = float(min(abs(p / e - 1) for e in self.every_pi_edge))
        self.margin, self.pi_margin = min(self.margin, margin), min(self.pi_margin, pi_margin)
        self.violations += (margin < EDGE_MARGIN[self.scene]) + (pi_margin < PI_MARGIN)
        bins = tuple(bin_of(R2, row) for row in self.edges)
        planes = {name: pi_plane(p, pe) for name, pe in self.pi_edges.items()}
        ww = mpf(float(first["w"][i])) * mpf(float(second["w"][j]))
        rec = self.records[key] = (R2, c2, DD, d_i * d_i, p, bins, planes, p <= self.pmax, ww)
        return rec


def far_apart(a, b, sa, sb, off_a, off_b, r2):
    """A cell between two sites, recognised in float64 (a factor 4 in the squared radius against errors of 1e-16)."""
    xyz = [np.array([[float(p.x), float(p.y), float(p.z)] for p in (Point(r, d) for r, d in zip(cat["ra"][lo:hi], cat["dec"][lo:hi]))])
           for cat, lo, hi in ((a, off_a[sa], off_a[sa + 1]), (b, off_b[sb], off_b[sb + 1]))]
    s2 = ((xyz[0][:, None, :] - xyz[1][None, :, :]) ** 2).sum(axis=2)
    return bool(np.all(s2 * min(a["d"].min(), b["d"].min()) ** 2 > 4.0 * r2.max()))


def exact_scene(scene, a, b, r2):
    """Every pair of the cells -> (arrays of the scene, number of pairs that break a condition, the pairs)."""
    import proj_exact

    n_sites = len(SITES_OF[scene])
    nf = r2.shape[1] - 1
    pairs = Pairs(scene, a, b, r2)
    out = {"r2": r2, "n_sites": np.int32(n_sites)}
    for cat, cols in (("a", a), ("b", b)):
        out.update({f"{cat}.{c}": v for c, v in cols.items()})
    by_chord, by_cut, not_capped = [], [], []
    outside = np.zeros((n_sites, 2, 2), dtype=np.int64)  # member-in-p pairs below the first / above the last edge of their row
    n_member, n_moved = 0, 0
    for fold in (False, True):
        for two in (False, True):
            cells = proj_exact.cell_lists(n_sites, fold, two)
            off_a, off_b = (cat["off"][::2] if fold else cat["off"] for cat in (a, b if two else a))
            N = np.zeros((len(cells), nf))
            N_pi = {name: np.zeros((len(pe) - 1, len(cells), nf)) for name, pe in PI_SETS.items()}
            sums = collections.defaultdict(lambda: [mpf(0), mpf(0)])  # (set or None, plane, cell, bin) -> [W, A]
            for n, (sa, sb, row, diagonal) in enumerate(cells):
                assert bool(diagonal) == (not two and sa == sb)
                if n >= len(cells) - 2:
                    assert far_apart(a, b if two else a, sa, sb, off_a, off_b, r2), "a cell between sites holds a pair"
                    continue
                for i in range(int(off_a[sa]), int(off_a[sa + 1])):
                    for j in range(int(off_b[sb]), int(off_b[sb + 1])):
                        if diagonal and j >= i:
                            continue  # a diagonal cell: every unordered pair once
                        key = (two, i, j) if two else (two, max(i, j), min(i, j))
                        R2, c2, DD, DD_first, p, bins, planes, inside, ww = pairs.get(*key)
                        e = bins[row]
                        if not fold:
                            if scene == "wide" and DD * c2 <= pairs.edges[row][-1] < R2:
                                not_capped.append((two, key[1], key[2], row, inside))
                            if inside:
                                outside[sa // 4, row] += (R2 <= pairs.edges[row][0], R2 > pairs.edges[row][-1])
                        if e is None or not inside:
                            continue
                        N[n, e] += 1
                        both = sums[(None, 0, n, e)]
                        both[0] += ww
                        both[1] += abs(ww)
                        for name, plane in planes.items():
                            N_pi[name][plane, n, e] += 1
                            both = sums[(name, plane, n, e)]
                            both[0] += ww
                            both[1] += abs(ww)
                        if fold:
                            continue
                        n_member += 1
                        n_moved += bin_of(DD_first * (R2 / DD), pairs.edges[row]) != e
                        if scene == "wide":
                            wrong = bin_of(DD * c2, pairs.edges[row])
                            if wrong != e:
                                by_chord.append((two, key[1], key[2], row, e, -1 if wrong is None else wrong))
                            wrong = bin_of(DD * (c2 * (1 + c2 / 12)), pairs.edges[row])
                            if wrong != e:
                                by_cut.append((two, key[1], key[2], row, e, -1 if wrong is None else wrong))
            head = ("fold." if fold else "") + ("two" if two else "one")
            out[("fold." if fold else "") + "cells." + ("two" if two else "one")] = cells
            out[f"{head}.N"] = N
            for c, plane in enumerate(("W", "A")):
                out[f"{head}.{plane}"] = np.array([[float(sums[(None, 0, n, e)][c]) for e in range(nf)] for n in range(len(cells))])
            for name, pe in PI_SETS.items():
                assert np.array_equal(N_pi[name].sum(axis=0), N), "the planes of a set do not sum to N"
                out[f"{head}.N_pi.{name}"] = N_pi[name]
                W_pi, A_pi = (np.array([[[float(sums[(name, j, n, e)][c]) for e in range(nf)] for n in range(len(cells))]
                                        for j in range(len(pe) - 1)]) for c in range(2))
                assert np.array_equal(W_pi, A_pi)  # every weight is > 0: a plane's sum of |w_a w_b| is its W, and is not stored twice
                out[f"{head}.W_pi.{name}"] = W_pi
    out.update(margin=np.float64(pairs.margin), pi_margin=np.float64(pairs.pi_margin), moved=np.float64(n_moved / max(n_member, 1)),
               outside=outside)
    if scene == "wide":
        out["by_chord"] = np.array(by_chord, dtype=np.int32).reshape(-1, 6)
        out["by_cut"] = np.array(by_cut, dtype=np.int32).reshape(-1, 6)
        out["not_capped"] = np.array(not_capped, dtype=np.int32).reshape(-1, 5)
    return {f"{scene}.{k}": v for k, v in out.items()}, int(pairs.violations), pairs


def conditions(scene, arrays):
    """The conditions a draw can miss besides the margins -> list of complaints (empty: the draw is good)."""
    import proj_exact
    import proj_oracle

    get = lambda name: arrays[f"{scene}.{name}"]  # noqa: E731
    complaints = []
    if get("moved") < 0.25:
        complaints.append(f"d_a alone moves only {get('moved'):.2f} of the member pairs")
    for which in ("one", "two"):
        if get(f"{which}.N").sum() <= 1000:
            complaints.append(f"only {get(f'{which}.N').sum():.0f} member pairs in the list {which}")
    if scene == "as" and np.any(get("outside") == 0):
        complaints.append("an end edge does not cut through the pairs of a site")
    if scene == "wide":
        beyond = get("not_capped")
        per_row = [np.bincount(beyond[beyond[:, 4] == inside, 3], minlength=2) for inside in (0, 1)]
        if len(get("by_chord")) < N_SENTINELS or len(get("by_cut")) < N_SENTINELS or min(r.min() for r in per_row) < N_SENTINELS // 2:
            complaints.append(f"sentinels: {len(get('by_chord'))} by chord, {len(get('by_cut'))} by cut, not capped {per_row}")
        for fold in (False, True):
            a, b = (proj_exact.scene(arrays, scene, cat, fold, False) for cat in "ab")
            for two in (False, True):
                smax = proj_oracle.reach(a, b if two else a, proj_exact.cells(arrays, scene, fold, two), get("r2"))
                if not np.all((smax >= 0.0095) & (smax <= S2_CAP)):
                    complaints.append(f"fold={fold} two={two}: the rows reach {smax}")
        for cat in "ab":
            ra, off = get(f"{cat}.ra"), get(f"{cat}.off")
            pole, wrap = slice(off[8], off[12]), slice(off[12], off[16])  # the four segments of the third and of the fourth site
            if not np.any(np.cos(ra[pole] - WIDE_SITES[2][0]) < 0.0) or min(np.sum(ra[wrap] < 1.0), np.sum(ra[wrap] > 5.0)) < 10:
                complaints.append("no ring over the pole, or no partners on both sides of the wrap")
            assert get(f"{cat}.dec").max() < np.pi / 2
    return complaints


# --------------------------------------------------------------------------- the mirror oracles against the file
def compare_counts(arrays, scene, pairs):
    """The mirror oracles' pair counts against ``N`` and ``N_pi``; a mismatch prints the pairs whose float64 bin or plane is
    not the exact one."""
    import proj_exact
    import proj_oracle
    import proj_pi_oracle

    ok = True
    for fold in (False, True):
        a, b = (proj_exact.scene(arrays, scene, cat, fold, False) for cat in "ab")
        for two in (False, True):
            cells, r2 = proj_exact.cells(arrays, scene, fold, two), arrays[f"{scene}.r2"]
            W, _, N = proj_oracle.proj_cells(a, b if two else a, cells, r2, PMAX)
            ok &= bool(np.array_equal(N, proj_exact.counts(arrays, scene, fold, two)) and np.array_equal(W, N))
            for name, pe in PI_SETS.items():
                N = proj_pi_oracle.proj_pi_cells(a, b if two else a, cells, r2, pe)[2]
                ok &= bool(np.array_equal(N, proj_exact.counts_pi(arrays, scene, fold, two, name)))
    if ok:
        return True
    r2 = arrays[f"{scene}.r2"]
    a, b = (proj_exact.scene(arrays, scene, cat, False, False) for cat in "ab")
    for (two, i, j), (_, _, _, _, _, bins, planes, _, _) in sorted(pairs.records.items()):
        R2, p, _ = proj_oracle.pair_terms(a, b if two else a, np.array([i]), np.array([j]))
        for row in range(len(r2)):
            e = int((R2[0] > r2[row]).sum()) - 1 if r2[row, 0] < R2[0] <= r2[row, -1] else None
            if e != bins[row]:
                print(f"{scene}: pair ({'a, b' if two else 'a, a'}) {i}, {j} row {row}: the contract's R2 = {R2[0]!r} falls into bin {e}, the exact one into {bins[row]}")
        for name, pe in PI_SETS.items():
            plane = int(proj_pi_oracle.pi_bin(p, pe)[0])
            if (plane if plane < len(pe) - 1 else None) != planes[name]:
                print(f"{scene}: pair ({'a, b' if two else 'a, a'}) {i}, {j}: the contract's p = {p[0]!r} falls into plane {plane} of {name}, the exact one into {planes[name]}")
    return False


def oracle_ratios(arrays):
    """Worst ``|mirror oracle - exact| / (2^-53 A)`` per scene, folding and cell list, over ``W`` and every ``W_pi``."""
    import proj_exact
    import proj_oracle
    import proj_pi_oracle

    out = {}
    for scene in ("as", "wide"):
        for fold in (False, True):
            a, b = (proj_exact.scene(arrays, scene, cat, fold, True) for cat in "ab")
            for two in (False, True):
                cells, r2 = proj_exact.cells(arrays, scene, fold, two), arrays[f"{scene}.r2"]
                W, A, _ = proj_oracle.proj_cells(a, b if two else a, cells, r2, PMAX)
                exp_w, exp_a = proj_exact.expected(arrays, scene, fold, two)
                np.testing.assert_allclose(A, exp_a, rtol=1e-12, atol=0)
                worst = proj_exact.worst_ratio(W, exp_w, exp_a)
                for name, pe in PI_SETS.items():
                    W, A, _ = proj_pi_oracle.proj_pi_cells(a, b if two else a, cells, r2, pe)
                    exp_w, exp_a = proj_exact.expected(arrays, scene, fold, two, name)
                    np.testing.assert_allclose(A, exp_a, rtol=1e-12, atol=0)
                    worst = max(worst, proj_exact.worst_ratio(W, exp_w, exp_a))
                out[proj_exact.prefix(scene, fold, two)] = worst
    return out


def write_design(K, worst):
    with open(DESIGN, encoding="utf-8") as fh:
        text = fh.read()
    marked = re.compile(r"(<!-- proj-exact-K -->).*?(<!-- /proj-exact-K -->)", re.S)
    if not marked.search(text):
        print("DESIGN.md has no proj-exact-K markers: not updated")
        return
    new = marked.sub(lambda m: f"{m.group(1)}`K` = {K:g} (worst measured ratio of the mirror oracles {worst:.3f}){m.group(2)}", text)
    if new != text:
        with open(DESIGN, "w", encoding="utf-8") as fh:
            fh.write(new)
    print(f"DESIGN.md: K = {K:g}")


def main():
    rng = np.random.default_rng(SEED)
    arrays = {"eps": np.float64(2.0**-53), "pmax": np.float64(PMAX)}
    arrays.update({f"pi.{name}": pe for name, pe in PI_SETS.items()})
    uneven = PI_SETS["uneven"]
    assert len(uneven) - 1 >= 8 and uneven[1] < 1e-3 and np.diff(uneven).min() < 1e-3 * PMAX and all(pe[-1] == PMAX for pe in PI_SETS.values())
    for scene, draw in (("as", draw_as), ("wide", draw_wide)):
        draws = 0
        while True:
            draws += 1
            a, b = draw(rng)
            part, violations, pairs = exact_scene(scene, a, b, radii2(scene))
            complaints = conditions(scene, part)
            if violations == 0 and not complaints:
                break
            print(f"{scene} draw {draws}: {violations} pairs within {EDGE_MARGIN[scene]:g} of a radius edge or {PI_MARGIN:g} of an edge in p"
                  + "".join("; " + c for c in complaints) + ": drawing again")
        arrays.update(part)
        arrays[f"{scene}.draws"] = np.int32(draws)
        n_one, n_two = (part[f"{scene}.{which}.N"].sum() for which in ("one", "two"))
        print(f"{scene} draw {draws} ({draws - 1} redraws): every condition holds, 0 pairs excluded; {n_one:.0f} + {n_two:.0f} member pairs (one handle + two), "
              f"nearest radius edge {part[f'{scene}.margin']:.2e} away, nearest edge in p {part[f'{scene}.pi_margin']:.2e}; d_a alone would move "
              f"{part[f'{scene}.moved']:.3f} of them")
        if scene == "wide":
            beyond = part["wide.not_capped"]
            print(f"wide sentinels: {len(part['wide.by_chord'])} member pairs change their bin by the chord, {len(part['wide.by_cut'])} by the series "
                  f"cut after s2 / 12; pairs that pass DD s2 <= r2max with R2 beyond it, per row: {np.bincount(beyond[beyond[:, 4] == 1, 3], minlength=2)} "
                  f"inside the cut, {np.bincount(beyond[beyond[:, 4] == 0, 3], minlength=2)} beyond it")
        if not compare_counts(arrays, scene, pairs):
            sys.exit(f"{scene}: the mirror oracles do not count the pairs of the exact reference: a finding about the contract")
    held = sum(arrays[f"{scene}.{which}.N_pi.uneven"].sum(axis=(1, 2)) for scene in ("as", "wide") for which in ("one", "two"))
    assert np.all(held > 0), f"a plane of the uneven set holds no pair: {held}"
    print(f"mpmath {mpmath.__version__} at {mp.dps} digits; the mirror oracles count N and N_pi in every cell, in two bins and folded; "
          f"pairs per plane of the uneven set: {held.astype(int)}")
    ratios = oracle_ratios(arrays)
    worst = max(ratios.values())
    K = 2.0 ** int(np.ceil(np.log2(4.0 * worst)))
    print("worst |oracle - exact| / (2^-53 A): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    print(f"measured worst {worst:.3f} -> K = {K:g}")
    assert worst <= 10.0, "a worst ratio above ~10 says the reference is wrong, not the tolerance"
    arrays.update({"K": np.float64(K), "K_measured": np.float64(worst)})
    save(OUT, arrays)
    write_design(K, worst)


if __name__ == "__main__":
    main()
