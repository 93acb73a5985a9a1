"""CPU: the exact reference of the per-lens radial count, tests/golden/dsigma_radial_exact.npz
(tools/make_golden_dsigma_radial_exact.py: mpmath, ``R2 = m_l (2 asin(chord / 2))^2`` against the edges, no series), and the
mirror oracle of the contract (tests/dsigma_radial_oracle.py) against it. The conditions the tool asserts are asserted again
from the stored arrays, without mpmath: they say that no pair is left out of any comparison and that the file tells a kernel
that bins by another quantity from a right one -- shown here on two wrong variants of the oracle's series. The kernel meets
the same file in tests/test_gpu_dsigma_radial_exact.py."""
import functools
import os
import sys

import numpy as np
import pytest

import dsigma_radial_exact as dre
import dsigma_radial_oracle as oracle
import shear_exact as se
from conftest import ROOT

ARCSEC = np.pi / 180.0 / 3600.0
DEG = np.pi / 180.0
EDGE_MARGIN = {"as": 1e-6, "wide": 1e-9}
CASES = [(name, columns, fold) for name in dre.SCENES for columns in ("real", "shear") for fold in (False, True)]


@functools.lru_cache(maxsize=None)
def oracle_planes(name, columns, fold):
    fx = dre.fixture()
    out = oracle.radial_jobs(*dre.scene(fx, name, columns, fold), fx[f"{name}.jobs"], fx[f"{name}.r2"])
    for a in out:
        a.setflags(write=False)
    return out


def float_pairs(fx, name, pairs):
    """``(s2, theta2, m, row)`` of the pairs ``(lens, source)`` in float64; the angle by ``arcsin``, not by the series."""
    lens, src = dre.scene(fx, name)
    i, j = pairs[:, 0], pairs[:, 1]
    d = [src[c][j] - lens[c][i] for c in "xyz"]
    s2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return s2, (2.0 * np.arcsin(0.5 * np.sqrt(s2))) ** 2, lens["m"][i], dre.lens_rows(fx, name)[i]


def bins_of(R2, rows):
    """The fine bin of ``R2`` in its row ``f64[n, E]``, -1 outside."""
    e = (R2[:, None] > rows).sum(axis=1) - 1
    return np.where((R2 > rows[:, 0]) & (R2 <= rows[:, -1]), e, -1)


@pytest.mark.parametrize("name", dre.SCENES)
def test_the_fixture_is_what_the_issue_asks_for(name):
    fx = dre.fixture()
    r2, jobs, n_patches = fx[f"{name}.r2"], fx[f"{name}.jobs"], int(fx[f"{name}.n_patches"])
    assert r2.shape == (2, 7) and np.all(np.diff(r2, axis=1) > 0)
    ratio = r2[:, 1:] / r2[:, :-1]
    np.testing.assert_allclose(ratio, ratio[:, :1] * np.ones(6), rtol=1e-12)  # log-spaced
    assert len(jobs) == n_patches + 2 and np.all(jobs[:n_patches, 0] == jobs[:n_patches, 1])
    pairs, N = fx[f"{name}.pairs"], fx[f"{name}.N"]
    assert 1000 < len(pairs) < 3000 and N.sum() == len(pairs) and np.all(N == np.rint(N))
    assert np.all(N[:n_patches].sum(axis=2) > 0) and not np.any(N[n_patches:])  # (the jobs between sites: empty cells)
    assert fx[f"{name}.fold.N"].sum() > 1.3 * N.sum()  # folded, a lens is binned by both rows
    # the margins: every member pair, and the scene's worst over all pairs
    assert fx[f"{name}.pair_margin"].min() >= EDGE_MARGIN[name] and fx[f"{name}.margin"] >= EDGE_MARGIN[name]
    assert fx[f"{name}.pair_margin"].min() >= np.float32(fx[f"{name}.margin"]) * (1.0 - 1e-6)
    lens, src = dre.scene(fx, name)
    i, j = pairs[:, 0], pairs[:, 1]
    assert np.abs(1.0 - lens["c"][i] * src["u"][j]).min() >= 1e-6
    behind = fx[f"{name}.pair_T"] != 0.0
    assert 0.35 < behind.mean() < 0.65
    # the stored bins are those of float64 arcsin (margins of 1e-9 against errors of 1e-15)
    s2, theta2, m, row = float_pairs(fx, name, pairs)
    assert np.array_equal(bins_of(m * theta2, r2[row]), fx[f"{name}.pair_bin"])
    # (the float64 chord comes from coordinates rounded to eps: eps / theta each, relative to the chord)
    assert np.all(np.abs(m * theta2 / fx[f"{name}.pair_R2"] - 1.0) <= 4.0 * se.EPS / np.sqrt(theta2) + 8.0 * se.EPS)
    # the bin follows the pair's own lens: the median m of the segment moves a quarter of the member pairs
    off = lens["off"]
    segment = np.searchsorted(off, i, side="right") - 1
    median = np.array([np.median(lens["m"][a:b]) for a, b in zip(off[:-1], off[1:])])
    moved = bins_of(median[segment] * theta2, r2[row]) != fx[f"{name}.pair_bin"]
    assert moved.mean() >= 0.25 and fx[f"{name}.pair_moved"].mean() >= 0.25 and np.mean(moved != fx[f"{name}.pair_moved"]) < 0.01
    print(f"{name}: {len(pairs)} member pairs, nearest edge {fx[f'{name}.margin']:.2e} away, the median m moves {moved.mean():.3f} of them")
    assert 1.0 <= fx["K"] <= 64.0 and fx["K"] >= 4.0 * fx["K_measured"] and fx["K_measured"] <= 10.0 and fx["eps"] == se.EPS
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dsigma_radial_exact.npz")) < 300 * 1024


def test_the_arcsecond_scene():
    fx = dre.fixture()
    lens, src = dre.scene(fx, "as")
    assert len(lens["ra"]) == 150 and len(src["ra"]) == 70 and np.all(np.diff(lens["off"]) == 15) and np.all(np.diff(src["off"]) == 14)
    dec = np.rad2deg(lens["dec"])
    for site in (0.0, 60.0, 89.99, -89.99):
        assert np.any(np.abs(dec - site) < 1e-3)
    pairs = fx["as.pairs"]
    assert np.count_nonzero(np.abs(lens["ra"][pairs[:, 0]] - src["ra"][pairs[:, 1]]) > 6.0) > 50  # across the wrap, and counted
    D = np.sqrt(lens["m"])
    assert 600.0 <= D.min() < 700.0 and 2400.0 < D.max() <= 2500.0
    for axis in "xyz":  # neighbours in any sort order differ widely in m
        for a, b in zip(lens["off"][:-1], lens["off"][1:]):
            m = lens["m"][a:b][np.argsort(lens[axis][a:b], kind="stable")]
            assert np.max(np.maximum(m[1:] / m[:-1], m[:-1] / m[1:])) > 3.0
    s2, theta2, _, _ = float_pairs(fx, "as", pairs)
    assert 0.3 * ARCSEC < np.sqrt(theta2.min()) and np.sqrt(theta2.max()) < 32.0 * ARCSEC
    assert np.all(fx["as.outside"] > 0)  # both end edges of both rows cut through the pairs of every site


def test_the_wide_scene_and_its_sentinels():
    fx = dre.fixture()
    lens, src = dre.scene(fx, "wide")
    r2, off = fx["wide.r2"], lens["off"]
    dec = np.rad2deg(lens["dec"])
    for site in (0.0, 60.0, 86.0):
        assert np.any(np.abs(dec - site) < 1e-2)
    pole, wrap = slice(*src["off"][2:4]), slice(*src["off"][3:5])
    assert np.any(np.cos(src["ra"][pole] - lens["ra"][off[4]]) < 0.0)  # a ring over the pole
    assert min(np.sum(src["ra"][wrap] < 1.0), np.sum(src["ra"][wrap] > 5.0)) >= 10
    # the call is accepted at the cap, per row and folded, by the library's own rule; the other lenses reach less far
    for k in range(2):
        segments = [lens["m"][off[s]:off[s + 1]] for s in range(k, len(off) - 1, 2)]
        reach = r2[k, -1] / min(seg.min() for seg in segments)
        assert 0.0095 <= reach and reach * (1.0 + 1e-12) <= dre.S2_CAP
        for seg in segments:
            assert 0.0095 <= r2[k, -1] / seg[0] and np.all(seg[1:] > 1.6 * seg[0])
    assert r2[:, -1].max() / lens["m"].min() * (1.0 + 1e-12) <= dre.S2_CAP
    s2, theta2, _, _ = float_pairs(fx, "wide", fx["wide.pairs"])
    assert np.sqrt(theta2.min()) < 0.3 * DEG and np.sqrt(theta2.max()) > 5.6 * DEG and np.count_nonzero(s2 > 0.003) > 100
    # the sentinels, again in float64 (they sit half a term from their edge: 1e-7 at the least)
    member = {(int(a), int(b)): int(e) for (a, b), e in zip(fx["wide.pairs"], fx["wide.pair_bin"])}
    for key, wrong in (("by_chord", lambda s: s), ("by_cut", lambda s: s * (1.0 + s / 12.0))):
        listed = fx[f"wide.{key}"]
        s2, theta2, m, row = float_pairs(fx, "wide", listed)
        true = np.array([member[(int(a), int(b))] for a, b in listed])  # (a KeyError: a listed pair is no member)
        assert len(listed) >= 8 and np.all(bins_of(m * wrong(s2), r2[row]) != true) and np.all(bins_of(m * theta2, r2[row]) == true)
        assert np.count_nonzero(r2[row, true] / m >= 0.003) >= 8  # ... at edges where the lens's reach is large
    beyond = fx["wide.not_capped"]
    s2, theta2, m, _ = float_pairs(fx, "wide", beyond)
    last = r2[beyond[:, 2], -1]
    good = (m * s2 <= last) & (m * theta2 > last)
    assert np.all(np.bincount(beyond[good, 2], minlength=2) >= 8) and good.mean() > 0.9
    print(f"wide: {len(fx['wide.by_chord'])} by chord, {len(fx['wide.by_cut'])} by cut, not capped per row {np.bincount(beyond[:, 2])}")


@pytest.mark.parametrize("name,columns,fold", CASES)
def test_the_mirror_oracle_holds_the_file(name, columns, fold):
    """``N`` exactly (unit columns), ``|oracle - exact| <= K eps A_theta + 1e-13 A`` per cell, ``W`` to ``RTOL_W``."""
    fx = dre.fixture()
    if columns == "real":
        unit = oracle.radial_jobs(*dre.scene(fx, name, "unit", fold), fx[f"{name}.jobs"], fx[f"{name}.r2"])
        assert np.array_equal(unit[2], dre.counts(fx, name, fold)) and not np.any(unit[0]) and not np.any(unit[1])
    got = oracle_planes(name, columns, fold)
    exp = dre.expected(fx, name, columns, fold)
    worst = se.check(dre.prefix(name, columns, fold), "TX", got[:2], got[2], exp, float(fx["K"]))
    np.testing.assert_allclose(got[3], exp[2], rtol=1e-12, atol=0)  # the oracle's A is the file's
    np.testing.assert_allclose(got[4], exp[3], rtol=1e-9, atol=0)
    assert worst <= float(fx["K_measured"])


def test_the_worst_ratio_is_the_one_k_was_made_from():
    fx = dre.fixture()
    worst = 0.0
    for name, columns, fold in CASES:
        got, exp = oracle_planes(name, columns, fold), dre.expected(fx, name, columns, fold)
        worst = max(worst, *(se.worst_ratio(got[c], exp[0][c], exp[2], exp[3]) for c in range(2)))
    assert worst == pytest.approx(float(fx["K_measured"]), rel=1e-12)


@pytest.mark.parametrize("variant", ["the chord", "cut after s2 / 12"])
def test_a_wrong_squared_angle_fails_the_counts(variant, monkeypatch):
    """The fixture bites: an oracle that bins by ``m s2``, or by a series without its ``s2^2 / 90``, counts other pairs than
    ``N`` on ``wide`` -- in the cells of the sentinels at the least -- and still the same pairs on ``as``, where the terms are
    1e-9 and less."""
    fx = dre.fixture()
    wrong = {"the chord": lambda s2: np.asarray(s2, dtype=np.float64) * 1.0,
             "cut after s2 / 12": lambda s2: s2 * (1.0 + s2 * (1.0 / 12.0))}[variant]
    monkeypatch.setattr(oracle, "squared_angle", wrong)
    for fold in (False, True):
        W = oracle.radial_jobs(*dre.scene(fx, "wide", "unit", fold), fx["wide.jobs"], fx["wide.r2"])[2]
        differ = np.abs(W - dre.counts(fx, "wide", fold)).sum()
        print(f"{variant}, {'folded' if fold else 'two bins'}: {differ:.0f} pairs counted elsewhere")
        assert not np.array_equal(W, dre.counts(fx, "wide", fold)) and differ >= 8
    W = oracle.radial_jobs(*dre.scene(fx, "as", "unit"), fx["as.jobs"], fx["as.r2"])[2]
    assert np.array_equal(W, fx["as.N"])


def test_every_seventh_pair_is_the_tools():
    """The stored pairs derived again with the tool's functions: membership, bin, ``R2`` and the terms."""
    pytest.importorskip("mpmath")
    from mpmath import mpf

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_dsigma_radial_exact as tool
    finally:
        sys.path.pop(0)
    fx = dre.fixture()
    n_checked = 0
    for name in dre.SCENES:
        lens = {c: fx[f"{name}.lens.{c}"] for c in ("ra", "dec", "w", "f", "c", "m")}
        src = {c: fx[f"{name}.src.{c}"] for c in ("ra", "dec", "w", "g1", "g2", "u")}
        wg1, wg2 = src["w"] * src["g1"], src["w"] * src["g2"]
        rows = dre.lens_rows(fx, name)
        edges = [[mpf(float(e)) for e in row] for row in fx[f"{name}.r2"]]
        assert np.array_equal(fx[f"{name}.r2"], tool.radii2(name))
        for n in range(0, len(fx[f"{name}.pairs"]), 7):
            i, j = fx[f"{name}.pairs"][n]
            a, b = tool.Point(lens["ra"][i], lens["dec"][i]), tool.Point(src["ra"][j], src["dec"][j])
            theta = tool.separation(tool.chord2(a, b))
            R2 = mpf(float(lens["m"][i])) * theta * theta
            assert tool.bin_of(R2, edges[rows[i]]) == fx[f"{name}.pair_bin"][n] and float(R2) == fx[f"{name}.pair_R2"][n]
            assert np.float32(min(abs(R2 / e - 1) for row in edges for e in row)) == fx[f"{name}.pair_margin"][n]
            tv, xv = tool.tangential_terms(lens["w"][i], wg1[j], wg2[j], *tool.double_angle(b, a))
            eff, s = tool.lensing_factor(lens["f"][i], lens["c"][i], src["u"][j])
            assert abs(eff) >= tool.CLIP_MARGIN
            want = (float(tv * s), float(xv * s)) if s > 0 else (0.0, 0.0)
            assert want == (fx[f"{name}.pair_T"][n], fx[f"{name}.pair_X"][n]), (name, n)
            n_checked += 1
    assert n_checked > 350
