"""The exact reference of the four shear counts at arcsecond separations: tests/golden/shear_exact.npz, written by
tools/make_golden_shear_exact.py (mpmath, >= 40 digits, from the float64 ``(ra, dec)`` of the scenes: spherical-trigonometry
position angles, exact chords, exact pair terms, per-cell sums rounded to float64 at the end). Shared by the CPU test of the
numpy oracles (tests/test_shear_exact_fixture.py), the GPU test of the kernels (tests/test_gpu_shear_exact.py) and the tool,
which measures ``K`` with ``worst_ratio`` below.

The rule for a signed sum, per cell:  ``|ours - exact| <= K * EPS * A_theta + 1e-13 * A``  with
``A_theta = sum |ww| (|g1| + |g2|) / theta_pair`` (shear-shear: the product of the two ends' magnitudes in the place of
``|g1| + |g2|``; Delta Sigma: the pair's ``s`` besides), ``A`` the same sum without ``1 / theta`` (it covers the summation order)
and ``EPS = 2^-52``. ``K`` is stored in the file: four times the worst ``|oracle - exact| / (EPS * A_theta)`` of the numpy
oracles over the whole file, rounded up to a power of two. ``W`` holds to ``helpers.RTOL_W``; a cell the reference finds empty
is exactly ``+0.0``."""
import functools

import numpy as np

from conftest import load_golden
from yet_another_wizz_amd.coordinates import radec_to_xyz

EPS = 2.0**-52
ORDER_TERM = 1e-13
RTOL_W = 1e-10  # helpers.RTOL_W (helpers imports the compiled oracle, which the tool does not need)


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("shear_exact.npz")


def _columns(fx, prefix, names):
    cat = {c: fx[f"{prefix}.{c}"] for c in names}
    cat["x"], cat["y"], cat["z"] = radec_to_xyz(cat["ra"], cat["dec"])
    cat["off"] = fx[f"{prefix}.off"].astype(np.int64)
    return cat


def lenses(fx, prefix):
    """The oracles' lens dict of ``<prefix>.lens.*`` (``nb`` from the offsets and the scene's patch count)."""
    cat = _columns(fx, f"{prefix}.lens", ("ra", "dec", "w"))
    cat["nb"] = (len(cat["off"]) - 1) // int(fx[f"{prefix}.n_patches"])
    return cat


def sources(fx, prefix):
    return _columns(fx, f"{prefix}.src", ("ra", "dec", "w", "g1", "g2"))


def catalogue(fx, prefix):
    """The oracles' dict of a binned shear catalogue ``<prefix>.*`` (two redshift bins)."""
    cat = _columns(fx, prefix, ("ra", "dec", "w", "g1", "g2"))
    cat["nb"] = 2
    return cat


def expected(fx, prefix, names):
    """``(signed planes, W, A, A_theta)`` of ``<prefix>.<name>``."""
    return [fx[f"{prefix}.{n}"] for n in names], fx[f"{prefix}.W"], fx[f"{prefix}.A"], fx[f"{prefix}.Ath"]


def worst_ratio(ours, exact, A, Ath):
    """Worst ``|ours - exact| / (EPS * A_theta)`` over the cells with pairs (0 where there are none)."""
    with_pairs = Ath > 0
    if not np.any(with_pairs):
        return 0.0
    return float(np.max(np.abs(ours - exact)[with_pairs] / (EPS * Ath[with_pairs])))


def check(key, names, got, got_w, exp, K):
    """The rule of the module docstring for every signed plane of ``got`` against ``exp = expected(...)``; prints the worst
    ratio of every plane and returns the largest."""
    planes, W, A, Ath = exp
    assert np.array_equal(A > 0, Ath > 0) and np.any(A > 0), key
    worst = 0.0
    for name, ours, exact in zip(names, got, planes):
        assert ours.shape == exact.shape, (key, name)
        ratio = worst_ratio(ours, exact, A, Ath)
        print(f"{key} {name}: worst |ours - exact| / (eps A_theta) = {ratio:.3f} (K = {K:g}) over {np.count_nonzero(A)} cells with pairs")
        assert np.all(np.abs(ours - exact) <= K * EPS * Ath + ORDER_TERM * A), (key, name, ratio)
        assert np.all(ours[A == 0] == 0.0) and not np.any(np.signbit(ours[A == 0])), (key, name)
        worst = max(worst, ratio)
    assert got_w.shape == W.shape, key
    assert np.all(got_w[W == 0] == 0.0) and not np.any(np.signbit(got_w[W == 0])), key
    np.testing.assert_allclose(got_w, W, rtol=RTOL_W, atol=0, err_msg=key)
    return worst


def swapped(cells):
    """The cell list of ``shear_pair_count`` with the two handles exchanged."""
    return np.ascontiguousarray(cells[:, [1, 0, 3, 2, 4]])
