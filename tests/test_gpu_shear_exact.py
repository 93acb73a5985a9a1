"""GPU: the four shear counts on the device against the exact reference of tests/golden/shear_exact.npz
(tools/make_golden_shear_exact.py: mpmath from the float64 ``(ra, dec)``, position angles by spherical trigonometry -- not the
contract's algebra): separations of 0.4 to 36 arcseconds at dec 0, 60 and +-89.99 degrees and across the wrap of the right
ascension. The rule is that of tests/shear_exact.py, ``|ours - exact| <= K eps A_theta + 1e-13 A`` per cell with the ``K`` stored
in the file, ``W`` to ``helpers.RTOL_W``, empty cells exactly ``+0.0``. Every case prints its worst ratio. A few hundred objects
per call; nothing here reads mpmath."""
import numpy as np
import pytest

import shear_exact as se
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
AXES = [0, 1, 2]


def upload_tangential(ctx, lens, src, sort_axis, dsigma=None):
    n_patches = len(src["off"]) - 1
    if dsigma is None:
        lenses = _lib.DeviceCatalog(ctx, lens["x"], lens["y"], lens["z"], lens["w"], n_patches, lens["nb"], lens["off"], sort_axis=sort_axis)
    else:
        lenses = _lib.DsigmaLenses(ctx, lens["x"], lens["y"], lens["z"], lens["w"], dsigma[0], dsigma[1], n_patches, lens["nb"],
                                   lens["off"], sort_axis=sort_axis)
    sources = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], src["w"], src["g1"], src["g2"], n_patches, src["off"],
                                sort_axis=sort_axis, u=None if dsigma is None else dsigma[2])
    return lenses, sources


def upload_catalogue(ctx, cat, sort_axis):
    n_patches = (len(cat["off"]) - 1) // cat["nb"]
    return _lib.ShearSources(ctx, cat["x"], cat["y"], cat["z"], cat["w"], cat["g1"], cat["g2"], n_patches, cat["off"],
                             sort_axis=sort_axis, n_bins=cat["nb"])


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("scene", ["tan", "pat"])
def test_shear_count(scene, sort_axis):
    fx = se.fixture()
    ctx = engine.get_context(0)
    t = fx["t"] if scene == "tan" else fx["t"][:1]
    jobs = fx[f"{scene}.jobs"]
    lenses, sources = upload_tangential(ctx, se.lenses(fx, scene), se.sources(fx, scene), sort_axis)
    try:
        T, X, W, stats = _lib.shear_count(ctx, lenses, sources, jobs, t)
    finally:
        lenses.free(), sources.free()
    assert stats.n_workgroups == len(jobs) * len(t) and stats.evaluated_pairs > 0
    se.check(f"shear_count {scene} axis={sort_axis}", "TX", (T, X), W, se.expected(fx, scene, "TX"), float(fx["K"]))
    if scene == "pat":  # the known answer: T / W = amplitude, X = 0
        bound = float(fx["K"]) * se.EPS * fx["pat.Ath"] + se.ORDER_TERM * fx["pat.A"]
        assert np.all(W > 0) and np.all(np.abs(T - float(fx["pat.amplitude"]) * W) <= bound) and np.all(np.abs(X) <= bound)


@pytest.mark.parametrize("sort_axis", AXES)
def test_dsigma_count(sort_axis):
    fx = se.fixture()
    ctx = engine.get_context(0)
    jobs = fx["tan.jobs"]
    lenses, sources = upload_tangential(ctx, se.lenses(fx, "tan"), se.sources(fx, "tan"), sort_axis, (fx["ds.f"], fx["ds.c"], fx["ds.u"]))
    try:
        T, X, W, stats = _lib.dsigma_count(ctx, lenses, sources, jobs, fx["t"])
    finally:
        lenses.free(), sources.free()
    assert stats.n_workgroups == len(jobs) * 2 and stats.evaluated_pairs > 0
    se.check(f"dsigma_count axis={sort_axis}", "TX", (T, X), W, se.expected(fx, "ds", "TX"), float(fx["K"]))


@pytest.mark.parametrize("sort_axis", AXES)
def test_shear_auto_count(sort_axis):
    fx = se.fixture()
    ctx = engine.get_context(0)
    jobs = fx["auto.jobs"]
    handle = upload_catalogue(ctx, se.catalogue(fx, "cat"), sort_axis)
    try:
        P, M, C, W, stats = _lib.shear_auto_count(ctx, handle, jobs, fx["t"])
    finally:
        handle.free()
    assert stats.n_workgroups == len(jobs) * 2 and stats.evaluated_pairs > 0
    se.check(f"shear_auto_count axis={sort_axis}", "PMC", (P, M, C), W, se.expected(fx, "auto", "PMC"), float(fx["K"]))


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("handles", ["one", "two", "swapped"])
def test_shear_pair_count(handles, sort_axis):
    """One handle; the catalogue and its twin (other weights and shears at the same positions); and the twin first with
    the cell list transposed, which has to give the same sums: every term is symmetric in the two ends."""
    fx = se.fixture()
    ctx = engine.get_context(0)
    cat = se.catalogue(fx, "cat")
    scene = "one" if handles == "one" else "two"
    cells = fx[f"{scene}.cells"]
    a = upload_catalogue(ctx, cat, sort_axis)
    b = a if handles == "one" else upload_catalogue(ctx, dict(cat, w=fx["catb.w"], g1=fx["catb.g1"], g2=fx["catb.g2"]), sort_axis)
    try:
        if handles == "swapped":
            P, M, C, W, stats = _lib.shear_pair_count(ctx, b, a, se.swapped(cells), fx["t"])
        else:
            P, M, C, W, stats = _lib.shear_pair_count(ctx, a, b, cells, fx["t"])
    finally:
        a.free()
        if b is not a:
            b.free()
    assert stats.n_workgroups == len(cells) and stats.evaluated_pairs > 0
    se.check(f"shear_pair_count {handles} axis={sort_axis}", "PMC", (P, M, C), W, se.expected(fx, scene, "PMC"), float(fx["K"]))
