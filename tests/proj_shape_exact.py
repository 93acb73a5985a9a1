"""The exact reference of the projected shape-shape count (``yawhip_proj_count_shapes``): tests/golden/proj_shape_exact.npz,
written by tools/make_golden_proj_shape_exact.py (mpmath at 50 digits from the float64 ``(ra, dec)`` and columns: the exact
angle ``2 asin(chord / 2)``, ``R2 = ((d_a + d_b) / 2)^2 theta^2`` and ``p = |c_a - c_b|`` against the float64 edges taken
exactly, the exact bearing of spherical trigonometry at BOTH ends for the rotation -- never the contract's series or its
``pa / pb / den`` algebra). Shared by the CPU test of the numpy oracle (tests/test_proj_shape_exact_fixture.py), the GPU test of
the kernel (tests/test_gpu_proj_shape_exact.py) and the tool, which measures ``K`` with ``worst_ratio`` below.

Scenes ``as`` (arcseconds; sites at dec 0, 60 and +-89.99 degrees and across the wrap of the right ascension) and ``wide``
(3 arcmin to 5.6 degrees, reaches at the cap of 5.73 degrees; a ring over the pole, one across the wrap): two shape catalogues
``a`` and ``b`` of two patches per site and two redshift bins per patch, and two cell lists, ``two`` (``a`` with ``b``) and ``one``
(``a`` with itself, diagonal cells included), each with two more cells between different sites, which hold nothing. Scene
``pairs``: the known answer, one catalogue of isolated pairs whose shapes lie along the great circle that joins them
(``along``), both turned by 45 degrees (``both``) or the first of the two turned (``one``); its "cell lists" are these three
sets of shears over the two diagonal cells.

The rule per pi bin, cell and fine bin is the project's for a signed sum (tests/shear_exact.py):
``|ours - exact| <= K * EPS * A_theta + 1e-13 * A`` with ``A = sum |w_a w_b| (|g1_a| + |g2_a|) (|g1_b| + |g2_b|)`` over the member
pairs, ``A_theta`` the same sum with every pair divided by its angle, and ``EPS = 2^-52``. ``K`` is stored in the file. ``W`` holds
to 1e-10; membership ``N`` is an integer and must be equal."""
import functools

import numpy as np

from conftest import load_golden
from yet_another_wizz_amd.coordinates import radec_to_xyz

SCENES = ("as", "wide")
LISTS = ("two", "one")
VARIANTS = ("along", "both", "one")  # the sets of shears of ``pairs``; the plane that holds sum w_a w_b e^2 is SIGNED[i]
PI_SETS = ("one", "four", "uneven")
EPS = 2.0**-52
ORDER_TERM = 1e-13
RTOL_W = 1e-10
SIGNED = ("PP", "XX", "PX")
PLANES = SIGNED + ("W", "A", "Ath", "N")


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("proj_shape_exact.npz")


def catalogue(fx, scene, cat, weighted=True):
    """Catalogue ``cat`` of the scene as the dict of tests/proj_shape_oracle.py: ``a`` or ``b`` of ``as`` and ``wide``, a name
    of VARIANTS for ``pairs`` (one catalogue under three sets of shears)."""
    own = f"{scene}.{cat}" if scene != "pairs" else scene
    cols = {c: fx[f"{own}.{c}"] for c in ("ra", "dec", "w", "d", "c")}
    cols.update(g1=fx[f"{scene}.{cat}.g1"], g2=fx[f"{scene}.{cat}.g2"])
    x, y, z = radec_to_xyz(cols.pop("ra"), cols.pop("dec"))
    if not weighted:
        cols["w"] = None
    return dict(cols, x=x, y=y, z=z, nb=2, off=fx[f"{own}.off"].astype(np.int64))


def cells(fx, scene, which):
    """The cell list ``which`` (``two`` or ``one``) of a scene; ``pairs``: its two diagonal cells."""
    return fx["pairs.cells"] if scene == "pairs" else fx[f"{scene}.cells.{which}"]


def expected(fx, scene, which, edges):
    """``{plane: f64[n_pi, n_cells, nf]}`` of the cell list (``pairs``: set of shears) ``which`` and the edge set ``edges`` (a
    name of PI_SETS), for the stored weights."""
    return {plane: fx[f"{scene}.{which}.{edges}.{plane}"] for plane in PLANES}


def worst_ratio(ours, exact, Ath):
    """Worst ``|ours - exact| / (EPS * A_theta)`` over the elements that hold a pair (0 where there are none)."""
    held = Ath > 0
    return float(np.max(np.abs(ours - exact)[held] / (EPS * Ath[held]))) if held.any() else 0.0


def bound(exp, K):
    return K * EPS * exp["Ath"] + ORDER_TERM * exp["A"]


def check(key, got, exp, K):
    """The rule of the module docstring for ``got = (PP, XX, PX, W)`` against ``exp = expected(...)``; prints the worst ratio
    of each signed plane and returns the largest."""
    worst = 0.0
    empty = exp["N"] == 0
    for name, ours in zip(SIGNED, got):
        assert ours.shape == exp[name].shape, (key, name)
        ratio = worst_ratio(ours, exp[name], exp["Ath"])
        print(f"{key} {name}: worst |ours - exact| / (eps A_theta) = {ratio:.3f} (K = {K:g}) over {np.count_nonzero(exp['A'])} elements with pairs")
        assert np.all(np.abs(ours - exp[name]) <= bound(exp, K)), (key, name, ratio)
        assert np.all(ours[empty] == 0.0) and not np.any(np.signbit(ours[empty])), (key, name)
        worst = max(worst, ratio)
    W = got[3]
    assert np.all(W[empty] == 0.0) and not np.any(np.signbit(W[empty])), key
    np.testing.assert_allclose(W, exp["W"], rtol=RTOL_W, atol=0, err_msg=key)
    return worst
