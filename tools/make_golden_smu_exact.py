#!/usr/bin/env python3
"""Generate ``tests/golden/smu_exact.npz``: an exact reference of the two redshift-space pair counts (``yawhip_proj_count_smu``
and ``yawhip_proj_count_smu_signed``, DESIGN.md sections 23 and 27) from arcseconds up to the cap of their reach, 5.73 degrees.

Runs on the CPU with ``mpmath`` at 50 digits; no GPU, no reference package. The arithmetic of a pair is that of
tools/make_golden_shear_exact.py, imported from there (``Point``, ``chord2``, ``separation``; the scenes are drawn with its
``ring_around`` and ``log_uniform`` and the file is written by its ``save``); sites, radius rows, segment sizes and
``catalogue`` are those of tools/make_golden_proj_exact.py and the cells those of tests/proj_exact.py. Per pair the tool takes
the float64 ``(ra, dec)`` of both ends and the float64 columns ``d, c, w`` and computes, exactly,

    theta = 2 asin(chord / 2),   R2 = ((d_a + d_b) / 2)^2 theta^2,   ps = c_b - c_a (second object of the call minus first),
    P2 = ps^2,   S2 = R2 + P2,   the fine bin  s2[row][e] < S2 <= s2[row][e + 1],
    the unsigned plane = the number of inner edges with  m2[k] S2 < P2,
    the signed plane   = the number of inner edges with sm2[k] S2 < sign(ps) P2

against the float64 edges and the float64 squares of the mu edges (``mu * mu``, signed ``copysign(mu * mu, mu)``) taken exactly.
NOTHING here evaluates the contract's series of the squared angle. (The two deliberately WRONG squared angles -- the chord
itself, and the chord with the one term ``s2 / 12`` -- and the wrong distance ``d`` of the first object are there to count the
pairs that tell them from the right ones.)

Scenes ``as`` and ``wide``: sites, two patches per site, two bins per patch, objects per segment, ``d`` and the two rows of six
log-spaced edges (read as edges of ``s``) as in the proj file; ``c`` is its 0 ... 120 draw times 2^-10 (``as``) and 2^-6
(``wide``), so that mu runs from 0 to 1. Placed besides, per site and bin (objects counted from the end of a segment):
  far      the last object of (second patch, ``a``) and (first patch, ``b``) lies beyond the last edge of either row in ``c``
           alone: pairs with ``R2 <= s2max < P2``, which an outer test on ``DD s2`` alone would let through
  zero_ps  four objects of both ``b`` segments carry the ``c`` of one object of (first patch, ``a``), bit for bit
  one_sky  an object of (second patch, ``a``) and one of (first patch, ``b``) at the sky position of one of (first patch,
           ``a``), bit for bit, their ``c`` apart by a separation inside the row
and in ``wide`` partners around an anchor (the first object of (first patch, ``a``), as near as the bin's least ``d`` allows), in
(second patch, ``a``) and (first patch, ``b``), as near themselves:
  chord    ``S2`` beyond the edge ``s2[k][5]`` by half of ``DD s2 / 12 * s2``: the chord puts the pair into the bin below
  cut      ... by half of ``DD s2^3 / 90``: a series cut after ``s2 / 12`` does
  mu       ``S2`` in the middle of the last bin and ``P2 = m2 (R2_mid + P2)`` at an edge of the 30-bin set, ``R2_mid`` half way
           between ``DD s2`` and ``DD theta^2``: the chord keeps the s bin and moves the pair one plane up
  cap      ``DD s2 + P2 <= s2max < S2``: past the kernel's outer test and in no bin; one with ``P2 == 0``, one with
           ``P2 = 0.6 s2max``, one between

Stored, per scene, cell list (``one``, ``two``) and for the bins as uploaded and folded (``fold.``): ``N_mu.<set>``
int32[n_mu, cells, nf] for the unsigned sets ``one`` (``[0, 1]``) and the three of tests/smu_scenes.py, and for the list ``two``
``N_smu.<set>`` for the mirrors of those three and ``asymmetric``. The exact weighted sums ``W_mu.<set>`` / ``W_smu.<set>``,
rounded once, are stored for the sets of ``STORED_W`` (the unsigned ``one``, ``uniform4`` and ``uneven`` and the signed
``asymmetric``): all that fits under the 300 KiB of the sibling fixtures. For the others (the 30-bin set, whose planes hold
about one pair per element and would be 8 bytes a pair, and the three mirrors; with the mirrors of ``uniform4`` and
``uneven`` alone the file is 367 KiB) tests/smu_exact.py sums the exact products ``w_a w_b`` over the mirror oracle's member
pairs, whose count per element is the file's: the tool asserts that this gives its own exact sums bit for bit, for EVERY set,
stored or not. Every weight is > 0, so ``A`` is ``W``. Per-pair records exist only for the sentinels.

Conditions, asserted; the inputs are redrawn until they hold (DESIGN.md section 28 lists them). A mismatch of the mirror
oracles' integers is a finding about the contract: the tool prints the pairs and stops; it does not draw again.

``K`` of the tolerance is four times the worst ``|mirror oracle - exact| / (2^-53 A)`` over ALL weighted planes (stored or
not), rounded up to a power of two; it goes into the file and into DESIGN.md (between the ``smu-exact-K`` markers).

Running it again reproduces the file byte for byte.

Usage:  python tools/make_golden_smu_exact.py
"""
from __future__ import annotations

import bisect
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
from make_golden_proj_exact import ARCMIN, EDGE_MARGIN, N_SENTINELS, PER_SEGMENT, SITES_OF, catalogue, far_apart, radii2  # noqa: E402
from make_golden_shear_exact import ARCSEC, DEG, SITES, Point, chord2, log_uniform, ring_around, save, separation  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smu_exact.npz")
DESIGN = os.path.join(ROOT, "DESIGN.md")
mp.dps = 50
SEED = 20261021
S2_CAP = 0.01
C_SCALE = {"as": 2.0**-10, "wide": 2.0**-6}
FAR_C = {"as": (0.3, 0.4), "wide": (4.0, 5.0)}  # beyond c <= 120 * scale by more than the last edge of either row
PLACED = (("chord", 2), ("cut", 2), ("mu", 2), ("cap", 3))  # placed partners per anchor and target segment
MU_PLACED = (6, 10, 14, 18, 22)  # edges of the 30-bin set that the "mu" partners are placed at
N_TIED = 4
STORED_W = (("mu", "one"), ("mu", "uniform4"), ("mu", "uneven"), ("smu", "asymmetric"))  # the others: summed by tests/smu_exact.py


def mu_sets():
    """``(unsigned, signed)``: name -> mu edges. The unsigned ``one`` and the three of tests/smu_scenes.py; their mirrors and
    ``asymmetric``."""
    import smu_exact
    import smu_scenes
    from proj_signed_oracle import mirrored

    unsigned = {"one": np.array([0.0, 1.0]), **smu_scenes.MU_SETS}
    signed = {**{name: mirrored(mu) for name, mu in smu_scenes.MU_SETS.items()}, "asymmetric": smu_exact.MU_ASYMMETRIC}
    return unsigned, signed


# --------------------------------------------------------------------------- scenes
def place_shared(rng, scene, segs, n_sites, r2):
    """``far``, ``zero_ps`` and ``one_sky`` of the docstring, on ``segs[cat][patch * 2 + k] = [ra, dec, d, c]``."""
    for site in range(n_sites):
        for k in range(2):
            first, second = segs["a"][4 * site + k], segs["a"][4 * site + 2 + k]
            b_first, b_second = segs["b"][4 * site + k], segs["b"][4 * site + 2 + k]
            second[3][-1], b_first[3][-1] = rng.uniform(*FAR_C[scene], 2)
            for seg in (b_first, b_second):
                seg[3][-1 - N_TIED:-1] = first[3][-2]
            lo, hi = 1.5 * np.sqrt(r2[k, 0]), 0.8 * np.sqrt(r2[k, -1])
            for n, seg in enumerate((second, b_first)):
                seg[0][-2 - N_TIED], seg[1][-2 - N_TIED] = first[0][-2 - N_TIED], first[1][-2 - N_TIED]
                apart = rng.uniform(lo, hi)
                below = (site + k + n) % 2 == 1 and first[3][-2 - N_TIED] - apart >= 0.0
                seg[3][-2 - N_TIED] = first[3][-2 - N_TIED] + (-apart if below else apart)


def finish(rng, segs):
    cats = {cat: catalogue([tuple(seg) for seg in segs[cat]]) for cat in "ab"}
    for cat in "ab":
        cats[cat]["w"] = rng.uniform(0.5, 2.0, len(cats[cat]["ra"]))
    return cats["a"], cats["b"]


def draw_as(rng):
    per, r2 = PER_SEGMENT["as"], radii2("as")
    segs = {cat: [] for cat in "ab"}
    for cat in "ab":
        for ra_c, dec_c in SITES:
            for _ in range(4):  # two patches over the same area, two bins each
                ra, dec = ring_around(rng, ra_c, dec_c, log_uniform(rng, 0.5, 30.0, per) * ARCSEC)
                c = rng.uniform(0.0, 120.0, per) * C_SCALE["as"]
                segs[cat].append([ra, dec, rng.uniform(600.0, 2500.0, per), c])
    place_shared(rng, "as", segs, len(SITES), r2)
    return finish(rng, segs)


def placed_partner(rng, kind, n, r2_row, DD):
    """``(theta^2, p)`` of the n-th placed partner of a kind, at the pair's ``DD``."""
    edge, end = r2_row[5], r2_row[6]
    if kind in ("chord", "cut"):
        p = 0.0 if n % 2 else rng.uniform(0.1, 0.5) * np.sqrt(edge)
        x = (edge - p * p) / DD
        return x * (1.0 + (x / 24.0 if kind == "chord" else x * x / 180.0)), p
    if kind == "cap":
        p = (0.0, np.sqrt(0.6 * end), rng.uniform(0.2, 0.6) * np.sqrt(end))[n % 3]
        x = (end - p * p) / DD
        return x * (1.0 + x / 24.0), p
    mu = np.linspace(0.0, 1.0, 31)[MU_PLACED[rng.integers(len(MU_PLACED))]]
    m2 = mu * mu
    theta2 = np.sqrt(edge * end) * (1.0 - m2) / DD
    return theta2, np.sqrt(m2 * DD * theta2 * (1.0 - theta2 / 24.0) / (1.0 - m2))


def draw_wide(rng):
    per, r2 = PER_SEGMENT["wide"], radii2("wide")
    least = {(cat, k): np.sqrt(r2[k, -1] / rng.uniform(0.0095, 0.00999)) for cat in "ab" for k in range(2)}
    segs = {cat: [None] * (4 * len(WIDE_SITES)) for cat in "ab"}
    n_placed = 0
    for site, (ra_c, dec_c) in enumerate(WIDE_SITES):
        for k in range(2):
            (ra_0,), (dec_0,) = ring_around(rng, ra_c, dec_c, 2.0 * ARCSEC * np.sqrt(rng.uniform(0.0, 1.0, 1)))
            d_0 = least["a", k] * (1.0 if site == 0 else rng.uniform(1.0, 1.02))
            c_0 = rng.uniform(30.0, 90.0) * C_SCALE["wide"]
            for cat, patch in (("a", 2 * site), ("a", 2 * site + 1), ("b", 2 * site), ("b", 2 * site + 1)):
                head = [(ra_0, dec_0, d_0, c_0)] if (cat, patch) == ("a", 2 * site) else []
                if (cat, patch) in (("a", 2 * site + 1), ("b", 2 * site)):
                    for kind, count in PLACED:
                        for n in range(count):
                            d = least[cat, k] * (1.0 if (site == 0 and not head) else rng.uniform(1.0, 1.02))
                            theta2, p = placed_partner(rng, kind, n, r2[k], (0.5 * (d_0 + d)) ** 2)
                            (ra,), (dec,) = ring_around(rng, ra_0, dec_0, np.array([np.sqrt(theta2)]))
                            n_placed += 1
                            head.append((ra, dec, d, c_0 - p if (n_placed % 2 and c_0 - p >= 0.0) else c_0 + p))
                n = per - len(head)
                assert n >= N_TIED + 2
                ra, dec = ring_around(rng, ra_c, dec_c, log_uniform(rng, 3.0 * ARCMIN, 5.6 * DEG, n))
                rest = (ra, dec, least[cat, k] * log_uniform(rng, 1.3, 4.0, n), rng.uniform(0.0, 120.0, n) * C_SCALE["wide"])
                segs[cat][patch * 2 + k] = [np.concatenate([[h[col] for h in head], rest[col]]) for col in range(4)]
    place_shared(rng, "wide", segs, len(WIDE_SITES), r2)
    return finish(rng, segs)


# --------------------------------------------------------------------------- exact arithmetic
Record = collections.namedtuple("Record", "S2 R2 P2 sign c2 DD DD_first bins planes splanes ww")


class Redraw(Exception):
    pass


def exact_int(w):
    """A float64 in [2^-10, 2^10) as an integer multiple of 2^-62."""
    scaled = float(w) * 2.0**62
    assert scaled == int(scaled)
    return int(scaled)


class Pairs:
    """Everything exact about a pair of objects, computed once. ``two``: object ``i`` of ``a`` with ``j`` of ``b``; else both of
    ``a``, ``i > j``; ``i`` is the first object of the pair and ``ps = c_j - c_i``."""

    def __init__(self, scene, a, b, r2):
        unsigned, signed = mu_sets()
        self.scene = scene
        self.cats = (a, b)
        self.points = [[Point(r, d) for r, d in zip(cat["ra"], cat["dec"])] for cat in (a, b)]
        self.edges = [[mpf(float(e)) for e in row] for row in r2]
        self.every_edge = sorted({e for row in self.edges for e in row})
        self.inner = {name: [mpf(float(v)) for v in (mu * mu)[1:-1]] for name, mu in unsigned.items()}
        self.signed_inner = {name: [mpf(float(v)) for v in np.copysign(mu * mu, mu)[1:-1]] for name, mu in signed.items()}
        every = {abs(e) for inner in list(self.inner.values()) + list(self.signed_inner.values()) for e in inner}
        self.every_mu_edge = sorted(e for e in every if e > 0)
        self.records = {}
        self.margin, self.mu_margin = np.inf, np.inf

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
        ps = mpf(float(second["c"][j])) - mpf(float(first["c"][i]))
        P2 = ps * ps
        S2 = R2 + P2
        assert S2 > 0, "two objects at one place in (ra, dec, c)"
        at = bisect.bisect_left(self.every_edge, S2)
        margin = float(min(abs(S2 / e - 1) for e in self.every_edge[max(at - 1, 0):at + 1]))
        self.margin = min(self.margin, margin)
        ratio = P2 / S2
        if P2 > 0:
            at = bisect.bisect_left(self.every_mu_edge, ratio)
            mu_margin = float(min(abs(e / ratio - 1) for e in self.every_mu_edge[max(at - 1, 0):at + 1]))
            self.mu_margin = min(self.mu_margin, mu_margin)
            margin = min(margin, mu_margin)
        if margin < EDGE_MARGIN[self.scene]:
            raise Redraw(f"pair {key} within {margin:.2e} of an edge")
        # m2[k] S2 < P2 iff m2[k] < P2 / S2, S2 > 0, and the quotient is off every edge by the margin: 50 digits decide it
        sign = int(ps > 0) - int(ps < 0)
        planes = {name: bisect.bisect_left(inner, ratio) for name, inner in self.inner.items()}
        splanes = {name: bisect.bisect_left(inner, sign * ratio) for name, inner in self.signed_inner.items()}
        bins = tuple(bin_of(S2, row) for row in self.edges)
        ww = exact_int(first["w"][i]) * exact_int(second["w"][j])
        rec = self.records[key] = Record(S2, R2, P2, sign, c2, DD, d_i * d_i, bins, planes, splanes, ww)
        return rec


def rounded(total):
    """An integer multiple of 2^-124 rounded once to float64."""
    return float(total) * 2.0**-124


def exact_scene(scene, a, b, r2):
    """Every pair of the cells -> (arrays of the scene, the exact weighted planes {key: W}, the pairs)."""
    import proj_exact

    unsigned, signed = mu_sets()
    n_sites = len(SITES_OF[scene])
    nf = r2.shape[1] - 1
    pairs = Pairs(scene, a, b, r2)
    out = {"s2": r2, "n_sites": np.int32(n_sites)}
    for cat, cols in (("a", a), ("b", b)):
        out.update({f"{cat}.{c}": v for c, v in cols.items()})
    listed = collections.defaultdict(list)
    weighted = {}
    n_member, n_moved = 0, 0
    for fold in (False, True):
        for two in (False, True):
            cells = proj_exact.cell_lists(n_sites, fold, two)
            off_a, off_b = (cat["off"][::2] if fold else cat["off"] for cat in (a, b if two else a))
            sets = [("mu", name, len(mu) - 1) for name, mu in unsigned.items()]
            sets += [("smu", name, len(mu) - 1) for name, mu in signed.items()] if two else []
            N = {(kind, name): np.zeros((n, len(cells), nf), dtype=np.int32) for kind, name, n in sets}
            sums = {(kind, name): collections.defaultdict(int) for kind, name, _ in sets}
            for n, (sa, sb, row, diagonal) in enumerate(cells):
                assert bool(diagonal) == (not two and sa == sb)
                if n >= len(cells) - 2:
                    assert far_apart(a, b if two else a, sa, sb, off_a, off_b, r2), "a cell between sites holds a pair"
                    continue
                last = pairs.edges[row][-1]
                for i in range(int(off_a[sa]), int(off_a[sa + 1])):
                    for j in range(int(off_b[sb]), int(off_b[sb + 1])):
                        if diagonal and j >= i:
                            continue  # a diagonal cell: every unordered pair once
                        key = (two, i, j) if two else (two, max(i, j), min(i, j))
                        rec = pairs.get(*key)
                        e = rec.bins[row]
                        if not fold:
                            head = (int(two), key[1], key[2], row)
                            if rec.DD * rec.c2 + rec.P2 <= last < rec.S2:
                                listed["not_capped"].append(head + (0 if rec.P2 == 0 else 2 if 2 * rec.P2 > rec.S2 else 1,))
                            if rec.R2 <= last < rec.P2:
                                listed["far"].append(head)
                        if e is None:
                            continue
                        for kind, name, _ in sets:
                            slot = ((rec.planes if kind == "mu" else rec.splanes)[name], n, e)
                            N[kind, name][slot] += 1
                            sums[kind, name][slot] += rec.ww
                        if fold:
                            continue
                        n_member += 1
                        theta2 = rec.R2 / rec.DD
                        wrong_d = rec.DD_first * theta2 + rec.P2
                        n_moved += bin_of(wrong_d, pairs.edges[row]) != e or bisect.bisect_left(pairs.inner["uniform30"], rec.P2 / wrong_d) != rec.planes["uniform30"]
                        if two and rec.sign == 0:
                            listed["zero_ps"].append(head + (e,))
                        if rec.c2 == 0:
                            listed["one_sky"].append(head + (e, rec.sign))
                        if scene == "wide":
                            chord = rec.DD * rec.c2 + rec.P2
                            wrong = bin_of(chord, pairs.edges[row])
                            if wrong != e:
                                listed["by_chord"].append(head + (e, -1 if wrong is None else wrong, int(rec.P2 > 0)))
                            elif bisect.bisect_left(pairs.inner["uniform30"], rec.P2 / chord) != rec.planes["uniform30"]:
                                listed["by_chord_mu"].append(head + (e, rec.planes["uniform30"], bisect.bisect_left(pairs.inner["uniform30"], rec.P2 / chord)))
                            wrong = bin_of(rec.DD * (rec.c2 * (1 + rec.c2 / 12)) + rec.P2, pairs.edges[row])
                            if wrong != e:
                                listed["by_cut"].append(head + (e, -1 if wrong is None else wrong, int(rec.P2 > 0)))
            head = ("fold." if fold else "") + ("two" if two else "one")
            out[("fold." if fold else "") + "cells." + ("two" if two else "one")] = cells
            for kind, name, n_mu in sets:
                assert np.array_equal(N[kind, name].sum(axis=0), N["mu", "one"][0]), "the planes of a set do not sum to those of one plane"
                out[f"{head}.N_{kind}.{name}"] = N[kind, name]
                W = np.zeros(N[kind, name].shape)
                for slot, total in sums[kind, name].items():
                    W[slot] = rounded(total)
                weighted[f"{scene}.{head}.W_{kind}.{name}"] = W
                if (kind, name) in STORED_W:
                    out[f"{head}.W_{kind}.{name}"] = W
    out.update(margin=np.float64(pairs.margin), mu_margin=np.float64(pairs.mu_margin), moved=np.float64(n_moved / max(n_member, 1)))
    widths = dict(not_capped=5, far=4, zero_ps=5, one_sky=6, by_chord=7, by_chord_mu=7, by_cut=7)
    for key in ("not_capped", "by_chord", "by_chord_mu", "by_cut") if scene == "wide" else ():
        out[key] = np.array(listed[key], dtype=np.int32).reshape(-1, widths[key])
    for key in ("far", "zero_ps", "one_sky"):
        out[key] = np.array(listed[key], dtype=np.int32).reshape(-1, widths[key])
    return {f"{scene}.{k}": v for k, v in out.items()}, weighted, pairs


def conditions(scene, arrays):
    """The conditions a draw can miss besides the margins -> list of complaints (empty: the draw is good)."""
    import proj_oracle
    import smu_exact

    unsigned, signed = mu_sets()
    get = lambda name: arrays[f"{scene}.{name}"]  # noqa: E731
    complaints = []
    if get("moved") < 0.25:
        complaints.append(f"d of the first object alone moves only {get('moved'):.2f} of the member pairs")
    for which in ("one", "two"):
        if get(f"{which}.N_mu.one").sum() <= 1000:
            complaints.append(f"only {get(f'{which}.N_mu.one').sum()} member pairs in the list {which}")
        for fold in ("", "fold."):
            for kind, names in (("mu", unsigned), ("smu", signed if which == "two" else {})):
                for name in names:
                    N = get(f"{fold}{which}.N_{kind}.{name}")
                    if N.sum(axis=(1, 2)).min() == 0:
                        complaints.append(f"{fold}{which}.N_{kind}.{name}: an empty plane")
                    if kind == "smu" and name != "asymmetric" and N[:len(N) // 2].sum() == N[len(N) // 2:].sum():
                        complaints.append(f"{fold}{which}.N_smu.{name}: both halves hold the same total")
    if get("one.N_mu.one").sum(axis=(0, 1)).min() == 0 or get("two.N_mu.one").sum(axis=(0, 1)).min() == 0:
        complaints.append("an empty s bin")
    if len(get("far")) < N_SENTINELS:
        complaints.append(f"only {len(get('far'))} pairs far along the line of sight")
    tied = get("zero_ps")
    if np.bincount(tied[:, 3], minlength=2).min() < N_SENTINELS:
        complaints.append(f"pairs with ps == 0 inside the s range, per row: {np.bincount(tied[:, 3], minlength=2)}")
    sky = get("one_sky")
    if len(sky) < 4 or not (np.any(sky[:, 5] < 0) and np.any(sky[:, 5] > 0) and np.any(sky[:, 0] == 0) and np.any(sky[:, 0] == 1)):
        complaints.append(f"only {len(sky)} pairs at one sky position inside the s range, or of one sign or one list only")
    if scene == "wide":
        for key in ("by_chord", "by_cut"):
            if len(get(key)) < N_SENTINELS or 2 * get(key)[:, 6].sum() < len(get(key)):
                complaints.append(f"{key}: {len(get(key))} pairs, {get(key)[:, 6].sum()} of them with P2 > 0")
        if len(get("by_chord_mu")) < N_SENTINELS:
            complaints.append(f"by_chord_mu: {len(get('by_chord_mu'))} pairs")
        beyond = get("not_capped")
        for row in range(2):
            kinds = np.bincount(beyond[beyond[:, 3] == row, 4], minlength=3)
            if kinds.sum() < N_SENTINELS or kinds[0] < 3 or kinds[2] < 3:
                complaints.append(f"not capped in row {row}: {kinds} with P2 == 0, between, P2 > S2 / 2")
        for fold in (False, True):
            a, b = (smu_exact.scene(arrays, scene, cat, fold, False) for cat in "ab")
            for two in (False, True):
                smax = proj_oracle.reach(a, b if two else a, smu_exact.cells(arrays, scene, fold, two), get("s2"))
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
def cases(arrays, scene, weighted):
    """``(prefix, first, second, cells, s2, [(kind, name, squared edges, oracle)])`` of the scene's four lists."""
    import smu_exact
    import smu_oracle
    import smu_signed_oracle

    unsigned, signed = mu_sets()
    for fold in (False, True):
        a, b = (smu_exact.scene(arrays, scene, cat, fold, weighted) for cat in "ab")
        for two in (False, True):
            sets = [("mu", name, mu * mu, smu_oracle.smu_cells) for name, mu in unsigned.items()]
            sets += [("smu", name, smu_signed_oracle.signed_squares(mu), smu_signed_oracle.smu_signed_cells) for name, mu in signed.items()] if two else []
            yield smu_exact.prefix(scene, fold, two), a, b if two else a, smu_exact.cells(arrays, scene, fold, two), arrays[f"{scene}.s2"], sets


def compare_counts(arrays, scene, pairs):
    """The mirror oracles' pair counts against ``N_mu`` and ``N_smu``; a mismatch prints the pairs whose float64 bin or plane
    is not the exact one."""
    import smu_exact
    import smu_oracle
    import smu_signed_oracle

    ok = True
    for prefix, first, second, cells, s2, sets in cases(arrays, scene, False):
        for kind, name, squares, oracle in sets:
            W, _, N = oracle(first, second, cells, s2, squares)
            ok &= bool(np.array_equal(N, arrays[f"{prefix}.N_{kind}.{name}"]) and np.array_equal(W, N))
    if ok:
        return True
    unsigned, signed = mu_sets()
    s2 = arrays[f"{scene}.s2"]
    a, b = (smu_exact.scene(arrays, scene, cat, False, False) for cat in "ab")
    for (two, i, j), rec in sorted(pairs.records.items()):
        S2, sP2, _, _ = smu_signed_oracle.signed_smu_terms(a, b if two else a, np.array([i]), np.array([j]))
        who = f"{scene}: pair ({'a, b' if two else 'a, a'}) {i}, {j}"
        for row in range(len(s2)):
            e = int((S2[0] > s2[row]).sum()) - 1 if s2[row, 0] < S2[0] <= s2[row, -1] else None
            if e != rec.bins[row]:
                print(f"{who} row {row}: the contract's S2 = {S2[0]!r} falls into bin {e}, the exact one into {rec.bins[row]}")
        for name, mu in unsigned.items():
            plane = int(smu_oracle.mu_plane(S2, np.abs(sP2), mu * mu)[0])
            if plane != rec.planes[name]:
                print(f"{who}: the contract's S2, P2 = {S2[0]!r}, {abs(sP2[0])!r} fall into plane {plane} of {name}, the exact ones into {rec.planes[name]}")
        for name, mu in signed.items():
            plane = int(smu_signed_oracle.signed_mu_plane(S2, sP2, smu_signed_oracle.signed_squares(mu))[0])
            if plane != rec.splanes[name]:
                print(f"{who}: the contract's S2, sP2 = {S2[0]!r}, {sP2[0]!r} fall into signed plane {plane} of {name}, the exact ones into {rec.splanes[name]}")
    return False


def oracle_ratios(arrays, weighted):
    """Worst ``|mirror oracle - exact| / (2^-53 A)`` per scene, folding and cell list over every ``W_mu`` and ``W_smu``; and
    the sums of tests/smu_exact.py over the oracle's member pairs are the tool's, bit for bit."""
    import smu_exact

    out = {}
    for scene in smu_exact.SCENES:
        for prefix, first, second, cells, s2, sets in cases(arrays, scene, True):
            worst = 0.0
            for kind, name, squares, oracle in sets:
                W, A, _ = oracle(first, second, cells, s2, squares)
                exp = weighted[f"{prefix}.W_{kind}.{name}"]
                np.testing.assert_allclose(A, exp, rtol=1e-12, atol=0)
                worst = max(worst, smu_exact.worst_ratio(W, exp, exp))
                fold, two = ".fold." in prefix + ".", prefix.endswith(".two")
                assert np.array_equal(smu_exact.summed(arrays, scene, fold, two, name, kind == "smu"), exp), (prefix, kind, name)
            out[prefix] = worst
    return out


def write_design(K, worst):
    with open(DESIGN, encoding="utf-8") as fh:
        text = fh.read()
    marked = re.compile(r"(<!-- smu-exact-K -->).*?(<!-- /smu-exact-K -->)", re.S)
    if not marked.search(text):
        print("DESIGN.md has no smu-exact-K markers: not updated")
        return
    new = marked.sub(lambda m: f"{m.group(1)}`K` = {K:g} (worst measured ratio of the mirror oracles {worst:.3f}){m.group(2)}", text)
    if new != text:
        with open(DESIGN, "w", encoding="utf-8") as fh:
            fh.write(new)
    print(f"DESIGN.md: K = {K:g}")


def main():
    import smu_exact

    rng = np.random.default_rng(SEED)
    unsigned, signed = mu_sets()
    arrays = {"eps": np.float64(2.0**-53)}
    arrays.update({f"mu.{name}": mu for name, mu in unsigned.items()})
    arrays.update({f"smu.{name}": mu for name, mu in signed.items()})
    weighted = {}
    for scene, draw in (("as", draw_as), ("wide", draw_wide)):
        draws = 0
        while True:
            draws += 1
            a, b = draw(rng)
            try:
                part, sums, pairs = exact_scene(scene, a, b, radii2(scene))
            except Redraw as why:
                print(f"{scene} draw {draws}: {why}: drawing again")
                continue
            complaints = conditions(scene, part)
            if not complaints:
                break
            print(f"{scene} draw {draws}: " + "; ".join(complaints) + ": drawing again")
        arrays.update(part)
        weighted.update(sums)
        arrays[f"{scene}.draws"] = np.int32(draws)
        get = lambda name: part[f"{scene}.{name}"]  # noqa: E731
        print(f"{scene} draw {draws} ({draws - 1} redraws): every condition holds, 0 pairs excluded; {get('one.N_mu.one').sum()} + {get('two.N_mu.one').sum()} member "
              f"pairs (one handle + two), nearest s edge {get('margin'):.2e} away, nearest m2 S2 to P2 {get('mu_margin'):.2e}; d of the first object alone "
              f"would move {get('moved'):.3f} of them; {len(get('far'))} far along the line of sight, ps == 0 per row {np.bincount(get('zero_ps')[:, 3])}, "
              f"{len(get('one_sky'))} at one sky position")
        for which in ("one", "two", "fold.one", "fold.two"):
            fewest = {name: int(get(f"{which}.N_mu.{name}").sum(axis=(1, 2)).min()) for name in unsigned}
            fewest.update({"signed " + name: int(get(f"{which}.N_smu.{name}").sum(axis=(1, 2)).min()) for name in (signed if which.endswith("two") else {})})
            print(f"  {which}: {get(f'{which}.N_mu.one').sum()} member pairs, fewest in an s bin {get(f'{which}.N_mu.one').sum(axis=(0, 1)).min()}, in a plane {fewest}")
        if scene == "wide":
            beyond = get("not_capped")
            print(f"wide sentinels: {len(get('by_chord'))} member pairs change their s bin by the chord, {len(get('by_cut'))} by the series cut after s2 / 12, "
                  f"{len(get('by_chord_mu'))} keep it and change their plane of the 30-bin set by the chord; past DD s2 + P2 <= s2max with S2 beyond it, per row "
                  f"(P2 == 0, between, P2 > S2 / 2): {[np.bincount(beyond[beyond[:, 3] == row, 4], minlength=3).tolist() for row in range(2)]}")
        if not compare_counts(arrays, scene, pairs):
            sys.exit(f"{scene}: the mirror oracles do not count the pairs of the exact reference: a finding about the contract")
    print(f"mpmath {mpmath.__version__} at {mp.dps} digits; the mirror oracles count N_mu and N_smu in every cell, in two bins and folded")
    ratios = oracle_ratios(arrays, weighted)
    worst = max(ratios.values())
    K = 2.0 ** int(np.ceil(np.log2(4.0 * worst)))
    print("worst |oracle - exact| / (2^-53 A): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    print(f"measured worst {worst:.3f} -> K = {K:g}")
    # a sum of n rounded products added one by one is off by less than n 2^-53 A: a ratio beyond the fullest element's n says
    # that the reference is wrong, not the tolerance (there is no cut: the one plane of a folded cell holds hundreds of pairs)
    fullest = max(int(arrays[f"{smu_exact.prefix(scene, fold, two)}.N_mu.one"].max()) for scene in smu_exact.SCENES for fold in (False, True) for two in (False, True))
    assert worst <= min(fullest, 64.0), (worst, fullest)
    arrays.update({"K": np.float64(K), "K_measured": np.float64(worst)})
    assert smu_exact.SCENES == ("as", "wide")
    save(OUT, arrays)
    write_design(K, worst)


if __name__ == "__main__":
    main()
