"""CPU: the numpy oracles of the four shear counts -- the contract's float64 algebra -- against the exact reference of
tests/golden/shear_exact.npz (tools/make_golden_shear_exact.py: mpmath, spherical-trigonometry position angles from the float64
``(ra, dec)``) at separations of 0.4 to 36 arcseconds, at dec 0, 60 and +-89.99 degrees and across the wrap of the right
ascension. The rule and ``K`` are those of tests/shear_exact.py; the kernels meet the same file in
tests/test_gpu_shear_exact.py."""
import os
import sys

import numpy as np
import pytest

import dsigma_oracle
import shear_auto_oracle
import shear_exact as se
import shear_oracle
import shear_pair_oracle
from conftest import ROOT

ARCSEC = np.pi / 180.0 / 3600.0


def scenes(fx):
    """``name -> (plane names, oracle result, expected)`` of every scene of the file."""
    t = fx["t"]
    lens, src = se.lenses(fx, "tan"), se.sources(fx, "tan")
    cat = se.catalogue(fx, "cat")
    twin = dict(cat, w=fx["catb.w"], g1=fx["catb.g1"], g2=fx["catb.g2"])
    return {
        "tan": ("TX", shear_oracle.shear_jobs(lens, src, fx["tan.jobs"], t)),
        "ds": ("TX", dsigma_oracle.dsigma_jobs(dict(lens, f=fx["ds.f"], c=fx["ds.c"]), dict(src, u=fx["ds.u"]), fx["tan.jobs"], t)),
        "pat": ("TX", shear_oracle.shear_jobs(se.lenses(fx, "pat"), se.sources(fx, "pat"), fx["pat.jobs"], t[:1])),
        "auto": ("PMC", shear_auto_oracle.shear_auto_jobs(cat, fx["auto.jobs"], t)),
        "one": ("PMC", shear_pair_oracle.shear_pair_cells(cat, cat, fx["one.cells"], t)),
        "two": ("PMC", shear_pair_oracle.shear_pair_cells(cat, twin, fx["two.cells"], t)),
    }


def test_the_fixture_is_what_the_issue_asks_for():
    fx = se.fixture()
    t = fx["t"]
    assert t.shape == (2, 7) and np.all(np.diff(t, axis=1) > 0) and not np.any(t[0] == t[1])
    chord = np.sqrt(t)
    assert chord.min() == pytest.approx(0.4 * ARCSEC, rel=1e-9) and chord.max() == pytest.approx(36.0 * ARCSEC, rel=1e-9)
    dec = np.rad2deg(fx["tan.lens.dec"])
    for site in (0.0, 60.0, 89.99, -89.99):
        assert np.any(np.abs(dec - site) < 1e-3)
    # partners on both sides of the wrap, in pairs that are counted
    ra_l, ra_s = fx["tan.lens.ra"][fx["tan.pairs"][:, 0]], fx["tan.src.ra"][fx["tan.pairs"][:, 1]]
    assert np.count_nonzero(np.abs(ra_l - ra_s) > 6.0) > 50
    ra = fx["cat.ra"]
    assert np.count_nonzero(np.abs(ra[fx["one.pairs"][:, 0]] - ra[fx["one.pairs"][:, 1]]) > 6.0) > 20
    # every kind of cell holds pairs, and empty cells sit next to them
    for prefix in ("tan", "ds", "auto", "one", "two"):
        A = fx[f"{prefix}.A"]
        assert np.count_nonzero(A) > 40 and np.any(A.reshape(len(A), -1).sum(axis=1) == 0), prefix
    cells, live = fx["one.cells"], fx["one.A"].sum(axis=1) > 0
    same_bin, diagonal = cells[:, 2] == cells[:, 3], (cells[:, 2] == cells[:, 3]) & (cells[:, 0] == cells[:, 1])
    assert np.any(live & diagonal) and np.any(live & same_bin & ~diagonal) and np.any(live & ~same_bin & (cells[:, 4] == 0))
    assert np.any(live & ~same_bin & (cells[:, 4] == 1)) and np.any(live & ~same_bin & (cells[:, 0] != cells[:, 1]))
    behind = fx["ds.pair_T"] != 0.0
    assert 0.4 < behind.mean() < 0.6
    assert 1.0 <= fx["K"] <= 64.0 and fx["K"] >= 4.0 * fx["K_measured"] and fx["K_measured"] <= 10.0 and fx["eps"] == se.EPS
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "shear_exact.npz")) < 300 * 1024


def test_the_numpy_oracles_hold_the_rule():
    fx = se.fixture()
    K = float(fx["K"])
    worst = 0.0
    for name, (planes, got) in scenes(fx).items():
        exp = se.expected(fx, name, planes)
        worst = max(worst, se.check(name, planes, got[:len(planes)], got[len(planes)], exp, K))
        np.testing.assert_allclose(got[len(planes) + 1], exp[2], rtol=1e-12, atol=0)  # the oracle's A is the file's
    assert worst == pytest.approx(float(fx["K_measured"]), rel=1e-12)  # the figure K was made from


def test_the_tangential_pattern_comes_back():
    """``T / W = amplitude`` and ``X / W = 0`` in every fine bin, within the bound of the rule."""
    fx = se.fixture()
    K, amplitude = float(fx["K"]), float(fx["pat.amplitude"])
    T, X, W, _ = shear_oracle.shear_jobs(se.lenses(fx, "pat"), se.sources(fx, "pat"), fx["pat.jobs"], fx["t"][:1])
    bound = K * se.EPS * fx["pat.Ath"] + se.ORDER_TERM * fx["pat.A"]
    assert np.all(W > 0) and W.sum() == pytest.approx(1.7 * fx["pat.src.w"].sum(), rel=1e-12)  # every source is counted
    for planes in ((T, X), (fx["pat.T"], fx["pat.X"])):  # the oracle, and the file's own sums
        assert np.all(np.abs(planes[0] - amplitude * W) <= bound) and np.all(np.abs(planes[1]) <= bound)
    print(f"pattern: worst |T / W - A| / A = {np.max(np.abs(T / W - amplitude)) / amplitude:.3e}, worst |X / W| / A = "
          f"{np.max(np.abs(X / W)) / amplitude:.3e}")


def test_every_seventh_pair_is_the_tools():
    """The per-pair terms of the file, derived again with the tool's functions: the file is the product of its tool."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_shear_exact as tool
    finally:
        sys.path.pop(0)
    fx = se.fixture()
    t = fx["t"]
    n_checked = 0

    def member(c2, rows):
        return any(tool.fine_bin(c2, t[row]) is not None for row in rows)

    for prefix, rows in (("tan", (0, 1)), ("pat", (0,))):
        lens = {c: fx[f"{prefix}.lens.{c}"] for c in ("ra", "dec", "w")}
        src = {c: fx[f"{prefix}.src.{c}"] for c in ("ra", "dec", "w", "g1", "g2")}
        wg1, wg2 = tool.products(src["w"], src["g1"], src["g2"])
        for n in range(0, len(fx[f"{prefix}.pairs"]), 7):
            i, j = fx[f"{prefix}.pairs"][n]
            a, b = tool.Point(lens["ra"][i], lens["dec"][i]), tool.Point(src["ra"][j], src["dec"][j])
            assert member(tool.chord2(a, b), rows)
            tv, xv = tool.tangential_terms(lens["w"][i], wg1[j], wg2[j], *tool.double_angle(b, a))
            assert (float(tv), float(xv)) == (fx[f"{prefix}.pair_T"][n], fx[f"{prefix}.pair_X"][n]), (prefix, n)
            if prefix == "tan":
                eff, s = tool.lensing_factor(fx["ds.f"][i], fx["ds.c"][i], fx["ds.u"][j])
                assert abs(eff) >= tool.CLIP_MARGIN
                want = (float(tv * s), float(xv * s)) if s > 0 else (0.0, 0.0)
                assert want == (fx["ds.pair_T"][n], fx["ds.pair_X"][n]), ("ds", n)
            n_checked += 1
    cat = {c: fx[f"cat.{c}"] for c in ("ra", "dec", "w", "g1", "g2")}
    twin = dict(cat, w=fx["catb.w"], g1=fx["catb.g1"], g2=fx["catb.g2"])
    for prefix, other in (("one", cat), ("two", twin)):
        wg_a = np.column_stack(tool.products(cat["w"], cat["g1"], cat["g2"]))
        wg_b = np.column_stack(tool.products(other["w"], other["g1"], other["g2"]))
        for n in range(0, len(fx[f"{prefix}.pairs"]), 7):
            i, j = fx[f"{prefix}.pairs"][n]
            a, b = tool.Point(cat["ra"][i], cat["dec"][i]), tool.Point(cat["ra"][j], cat["dec"][j])
            assert member(tool.chord2(a, b), (0, 1))
            terms = tool.shear_shear_terms(wg_a[i], wg_b[j], tool.double_angle(a, b), tool.double_angle(b, a))
            assert tuple(float(v) for v in terms) == tuple(fx[f"{prefix}.pair_{c}"][n] for c in "PMC"), (prefix, n)
            n_checked += 1
    assert n_checked > 700
