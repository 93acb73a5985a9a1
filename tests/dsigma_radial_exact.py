"""The exact reference of the per-lens radial count (``yawhip_dsigma_count_radial``): tests/golden/dsigma_radial_exact.npz,
written by tools/make_golden_dsigma_radial_exact.py (mpmath at 50 digits from the float64 ``(ra, dec)`` and columns: the exact
angle ``2 asin(chord / 2)``, ``R2 = m_l theta^2`` against the float64 edges taken exactly -- never the contract's series).
Shared by the CPU test of the mirror oracle (tests/test_dsigma_radial_exact_fixture.py), the GPU test of the kernel
(tests/test_gpu_dsigma_radial_exact.py) and the tool. The rule, ``check`` and ``worst_ratio`` are those of tests/shear_exact.py;
``K`` is the one stored in THIS file.

Scenes ``as`` (arcseconds, five sites) and ``wide`` (3 arcmin to 5.6 degrees, reaches at the cap). Per scene the planes exist
for three sets of columns -- ``"real"`` (everything as stored), ``"shear"`` (``f = 1``, ``c = 0``, ``u = 0``, real weights and
shears: what ``crosscorrelate_shear(radius="lens")`` sends; prefix ``sh.``) and ``"unit"`` (no weights, zero shear besides: ``W``
is the pair count ``N``) -- and for the lenses in their two redshift bins or folded into one bin under both rows (``fold.``)."""
import functools

import numpy as np

from conftest import load_golden
from yet_another_wizz_amd.coordinates import radec_to_xyz

SCENES = ("as", "wide")
S2_CAP = 0.01


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("dsigma_radial_exact.npz")


def prefix(name, columns="real", fold=False):
    """The key prefix of the planes of a scene (``columns`` "real" or "shear"; the counts ``N`` do not depend on them)."""
    return name + (".fold" if fold else "") + (".sh" if columns == "shear" else "")


def counts(fx, name, fold=False):
    return fx[f"{name}{'.fold' if fold else ''}.N"]


def scene(fx, name, columns="real", fold=False):
    """``(lens, src)``, the dicts of tests/dsigma_radial_oracle.py."""
    lens = {c: np.asarray(fx[f"{name}.lens.{c}"]) for c in ("ra", "dec", "w", "f", "c", "m")}
    src = {c: np.asarray(fx[f"{name}.src.{c}"]) for c in ("ra", "dec", "w", "g1", "g2", "u")}
    for cat, off in ((lens, fx[f"{name}.lens.off"]), (src, fx[f"{name}.src.off"])):
        cat["x"], cat["y"], cat["z"] = radec_to_xyz(cat["ra"], cat["dec"])
        cat["off"] = np.asarray(off).astype(np.int64)
    lens["nb"] = 2
    if fold:
        lens.update(nb=1, off=lens["off"][::2].copy())
    if columns in ("shear", "unit"):
        lens.update(f=np.ones_like(lens["f"]), c=np.zeros_like(lens["c"]))
        src.update(u=np.zeros_like(src["u"]))
    if columns == "unit":
        lens.update(w=None)
        src.update(w=None, g1=np.zeros_like(src["g1"]), g2=np.zeros_like(src["g2"]))
    return lens, src


def expected(fx, name, columns="real", fold=False):
    """``((T, X), W, A, A_theta)`` for ``shear_exact.check``."""
    p = prefix(name, columns, fold)
    return [fx[f"{p}.T"], fx[f"{p}.X"]], fx[f"{p}.W"], fx[f"{p}.A"], fx[f"{p}.Ath"]


def lens_rows(fx, name):
    """The row (redshift bin) of every lens of the scene as uploaded in two bins."""
    off = np.asarray(fx[f"{name}.lens.off"])
    return (np.searchsorted(off, np.arange(off[-1]), side="right") - 1) % 2
