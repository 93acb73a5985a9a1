"""The float32 guard of the band kernel (k_count_band32, yet_another_wizz_amd/csrc/yawhip_band32.inc): for unit vectors rounded
to float32, the float32 distance s32 = fma(dz, dz, fma(dy, dy, dx * dx)) stays within
g(s) = 2.1e-7 sqrt(s) + 5e-7 s + 1e-12 of the float64 value of the parity contract. The derivation is in the kernel's
header; here the bound is checked on a few million pairs, with adversarial coordinates included (CPU, numpy)."""
import os
import re

import numpy as np

from conftest import ROOT


def _s32(a, b):
    """The kernel's float32 arithmetic, emulated: float32 images, float32 differences, mul + 2 fma."""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    d = a32 - b32  # float32 subtraction, correctly rounded
    dx, dy, dz = (d[:, i].astype(np.float64) for i in range(3))
    acc = (dx * dx).astype(np.float32).astype(np.float64)            # v_mul_f32 (the product of two float32 is exact in float64)
    acc = (dy * dy + acc).astype(np.float32).astype(np.float64)     # v_fma_f32: one rounding of the exact sum
    return (dz * dz + acc).astype(np.float32).astype(np.float64)


def _s64(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _guard(s):
    return 2.1e-7 * np.sqrt(s) + 5e-7 * s + 1e-12


def test_constants_match_the_kernel_source():
    csrc = os.path.join(ROOT, "yet_another_wizz_amd", "csrc")
    header = open(os.path.join(csrc, "yawhip_count_kernels.h")).read()  # the constant the kernels and the host tables share
    src = open(os.path.join(csrc, "yawhip_count.hip")).read()           # build_thr32 / build_fine32
    assert re.search(r"BAND32_GUARD_SQRT = 2\.1e-7;", header)
    assert src.count("BAND32_GUARD_SQRT * std::sqrt(te) + 5e-7 * te + 1e-12") == 2
    assert "const double fold = 4e-7 * cd;" in src


def test_float32_guard_holds():
    rng = np.random.default_rng(20261004)
    worst = 0.0
    for trial in range(8):
        n = 500_000
        a = rng.normal(size=(n, 3))
        if trial % 2:  # points near the coordinate axes and planes: coordinates next to 1, 0.5, 0.25 (binade borders) and 0
            a *= np.array([1.0, 1e-3, 1e-5])[rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1)]
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        v = rng.normal(size=(n, 3))
        v -= (v * a).sum(1, keepdims=True) * a
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        ang = 10.0 ** rng.uniform(-6.0, np.log10(np.pi), n)
        b = a * np.cos(ang)[:, None] + v * np.sin(ang)[:, None]
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        s64 = _s64(a, b)
        err = np.abs(_s32(a, b) - s64)
        ratio = err / _guard(s64)
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (trial, float(ratio.max()))
    assert 0.05 < worst <= 1.0  # the bound is conservative, not absurdly so


def _q32(a, b, c):
    """One annulus: the kernel's q = fma(dz, dz, fma(dy, dy, fma(dx, dx, -c))) with the float32 centre c as the first addend."""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    d = a32 - b32
    dx, dy, dz = (d[:, i].astype(np.float64) for i in range(3))
    acc = (dx * dx - c.astype(np.float64)).astype(np.float32).astype(np.float64)
    acc = (dy * dy + acc).astype(np.float32).astype(np.float64)
    return (dz * dz + acc).astype(np.float32).astype(np.float64)


def _annulus_classes(t0, t1):
    """build_thr32 for two edges (yawhip_count.hip), restated: centre, half width of "certainly inside", of "possibly inside"."""
    g0, g1 = _guard(t0), _guard(t1)
    c = (0.5 * (t0 + t1)).astype(np.float32)
    cd = c.astype(np.float64)
    fold = 4e-7 * cd
    h_in = (np.minimum(cd - (t0 + g0), (t1 - g1) - cd) - fold) * (1.0 - 1e-6)
    h_out = (np.maximum(cd - (t0 - g0), (t1 + g1) - cd) + fold) * (1.0 + 1e-6)
    h_in32 = h_in.astype(np.float32)
    h_in32 = np.where(h_in32.astype(np.float64) > h_in, np.nextafter(h_in32, np.float32(-np.inf)), h_in32)
    h_in32 = np.where(h_in > 0.0, h_in32, np.float32(0.0))
    h_out32 = np.maximum(h_out, 0.0).astype(np.float32)
    h_out32 = np.where(h_out32.astype(np.float64) < h_out, np.nextafter(h_out32, np.float32(np.inf)), h_out32)
    return c, h_in32.astype(np.float64), h_out32.astype(np.float64)


def test_annulus_classes_with_the_centre_folded_into_the_fma_chain():
    """Pairs placed at an edge of their annulus (within a few guard widths), deep inside and far outside: a class claimed in
    float32 is the float64 truth; only guard-band pairs stay undecided."""
    rng = np.random.default_rng(4)
    undecided = total = 0
    for trial in range(6):
        n = 400_000
        a = rng.normal(size=(n, 3))
        if trial % 2:
            a *= np.array([1.0, 1e-3, 1e-5])[rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1)]
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        v = rng.normal(size=(n, 3))
        v -= (v * a).sum(1, keepdims=True) * a
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        # annuli from arcseconds to tens of degrees, inner edge from 0 to 0.99 of the outer one
        th1 = 10.0 ** rng.uniform(-5.5, np.log10(2.0), n)
        th0 = th1 * rng.choice([0.0, 0.01, 0.1, 0.5, 0.9, 0.99], n)
        t0, t1 = (2.0 * np.sin(th0 / 2.0)) ** 2, (2.0 * np.sin(th1 / 2.0)) ** 2
        edge = np.where(rng.random(n) < 0.5, th0, th1)
        kind = rng.integers(0, 3, n)
        ang = np.where(kind == 0, edge * (1.0 + rng.normal(size=n) * 3e-7) + rng.normal(size=n) * 1e-10,  # on an edge
                       np.where(kind == 1, rng.uniform(th0, th1), th1 * 10.0 ** rng.uniform(0.0, 1.0, n)))
        ang = np.clip(np.abs(ang), 0.0, np.pi)
        b = a * np.cos(ang)[:, None] + v * np.sin(ang)[:, None]
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        c, h_in, h_out = _annulus_classes(t0, t1)
        q = np.abs(_q32(a, b, c))
        s = _s64(a, b)
        inside = (s > t0) & (s <= t1)
        certainly = q < h_in
        possibly = q < h_out
        assert not np.any(certainly & ~inside), trial
        assert not np.any(~possibly & inside), trial
        far = (kind != 0) & (th0 <= 0.5 * th1) & (th1 > 1e-4)  # wide annuli of at least 20 arcsec, pairs not placed on an edge
        undecided += int((possibly & ~certainly & far).sum())
        total += int(far.sum())
    assert undecided < 1e-2 * total  # away from the edges the classes decide (2.3e-3 observed: 20-arcsec annuli are a few hundred guards wide)
