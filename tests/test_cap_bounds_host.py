"""The float32 cap bounds of the band kernels (cap_lo32 / cap_hi32, csrc/yawhip_count_device.h), mirrored in numpy float32.

The bounds cull: the band of a lane runs over the streamed keys in [cap_lo32(u32), cap_hi32(u32)], so a bound that lies INSIDE
the true cap loses pairs. The mirror evaluates the device's expressions operation by operation in float32 (the fused
multiply-adds exactly rounded) with the square root taken correctly rounded and one ulp below and above it: the hardware
square root the kernels use is within one ulp, the derivation beside cap_lo32 budgets two. For every key u^ (float64, what the
exact path sees) and its float32 image the float32 bound must lie outside the float64 bound of the unshifted key,
u^ c -/+ sqrt(1 - u^2) s (clipped to -/+ 1 where the cap holds a pole), by at least 3.1e-8: the distance the PARTNER's float32
key can lie from its float64 key (2^-25 + 5e-10), the last term of that derivation.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import ARCMIN

CAP32_SHIFT, CAP32_CLIP, CAP32_MARGIN = np.float32(1e-7), np.float32(1.2e-7), np.float32(8e-7)
PARTNER_IMAGE = 3.1e-8
THETAS = {"0.5'": 0.5 * ARCMIN, "1'": ARCMIN, "10'": 10 * ARCMIN, "1deg": np.deg2rad(1.0), "5.7deg": np.deg2rad(5.7)}
N_KEYS = 200_000
f32 = np.float32


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays: the product is exact in float64, the sum is rounded to ODD there (TwoSum gives the
    error of the float64 add) and then to float32 -- 53 >= 2 x 24 + 2 bits, so the double rounding is the single one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float32), p.shape).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((err != 0.0) & even, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return odd.astype(np.float32)


def sqrt32(x, ulps):
    r = np.sqrt(x)  # float32 in, correctly rounded float32 out
    if ulps:
        r = np.where(r > 0, np.nextafter(r, f32(np.inf if ulps > 0 else -np.inf)), r).astype(np.float32)
    return r


def cap_lo32(u, c, s, ulps):
    ul = np.maximum(u - CAP32_SHIFT, f32(-1.0))
    root = sqrt32(np.maximum(fma32(-ul, ul, f32(1.0)), f32(0.0)), ulps)
    formula = fma32(ul, np.broadcast_to(c, ul.shape), -root * s) - CAP32_MARGIN
    return np.where(ul <= -c + CAP32_CLIP, f32(-1.0) - CAP32_MARGIN, formula)


def cap_hi32(u, c, s, ulps):
    uh = np.minimum(u + CAP32_SHIFT, f32(1.0))
    root = sqrt32(np.maximum(fma32(-uh, uh, f32(1.0)), f32(0.0)), ulps)
    formula = fma32(uh, np.broadcast_to(c, uh.shape), root * s) + CAP32_MARGIN
    return np.where(uh >= c - CAP32_CLIP, f32(1.0) + CAP32_MARGIN, formula)


def keys(theta: float) -> np.ndarray:
    """float64 keys: a regular grid over [-1, 1], and a quarter of them within a few float32 steps of -1, +1 and of the
    clips at -/+ cos theta (where the bound changes branch)."""
    rng = np.random.default_rng(20261021)
    n_edge = N_KEYS // 16
    c = np.cos(theta)
    near = [centre + sign * 10.0 ** rng.uniform(-9.0, -5.5, n_edge) for centre in (-1.0, 1.0, -c, c) for sign in (-1.0, 1.0)]
    grid = np.linspace(-1.0, 1.0, N_KEYS - 8 * n_edge)
    exact = np.array([-1.0, 1.0, -c, c, np.nextafter(-c, 0.0), np.nextafter(c, 0.0), 0.0])
    u = np.clip(np.concatenate([grid, *near, exact]), -1.0, 1.0)
    return u


def test_fma32_is_exactly_rounded():
    rng = np.random.default_rng(5)
    a, b, c = (rng.uniform(-1, 1, 2000).astype(np.float32) for _ in range(3))
    c[:1000] = -(a[:1000] * b[:1000])  # cancellation: the low bits of the product decide
    from fractions import Fraction

    got = fma32(a, b, c)
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # the nearest float32 of an exact rational: float() of a Fraction rounds correctly to float64 only, so compare distances
        g = Fraction(float(got[i]))
        for other in (np.nextafter(got[i], f32(np.inf)), np.nextafter(got[i], f32(-np.inf))):
            assert abs(g - exact) <= abs(Fraction(float(other)) - exact), i


@pytest.mark.parametrize("ulps", [-1, 0, 1], ids=["sqrt-1ulp", "sqrt", "sqrt+1ulp"])
@pytest.mark.parametrize("name", list(THETAS))
def test_float32_bounds_lie_outside_the_float64_cap(name, ulps):
    theta = THETAS[name]
    u = keys(theta)
    assert len(u) >= N_KEYS
    c64, s64 = np.cos(theta), np.sin(theta)
    c32, s32 = f32(c64), f32(s64)  # what the kernels are given (ucap)
    u32 = u.astype(np.float32)
    root = np.sqrt(np.maximum(1.0 - u * u, 0.0))
    lo64 = np.where(u <= -c64, -1.0, u * c64 - root * s64)
    hi64 = np.where(u >= c64, 1.0, u * c64 + root * s64)
    lo = cap_lo32(u32, c32, s32, ulps).astype(np.float64)
    hi = cap_hi32(u32, c32, s32, ulps).astype(np.float64)
    slack_lo, slack_hi = lo64 - lo, hi - hi64
    print(f"{name} sqrt{ulps:+d}ulp: least slack below {slack_lo.min():.3e}, above {slack_hi.min():.3e}")
    assert slack_lo.min() >= PARTNER_IMAGE, (name, ulps, u[slack_lo.argmin()])
    assert slack_hi.min() >= PARTNER_IMAGE, (name, ulps, u[slack_hi.argmin()])
