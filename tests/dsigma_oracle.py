"""numpy brute force of the excess-surface-density count (``yawhip_dsigma_count``, include/yawhip.h)
over a job list, in the operation order of the contract.

Pair membership and the rotation are those of tests/shear_oracle.py (``projection``); with ``wg = w_s * g`` as the upload
makes it (``g`` itself without source weights) a pair in fine bin ``e`` adds

    eff = 1.0 - c_l*u_s
    if eff > 0.0:
        s = f_l*eff;  ws = w_l*s
        tv = -(wg1*c2 + wg2*s2p);  xv = wg1*s2p - wg2*c2
        T += ws*tv;  X += ws*xv        (den == 0: skipped)
        W += (ws*s)*w_s

every product and sum rounded on its own. The loops, chunks and the order of the pairs are shear_oracle.shear_jobs', so that
``f = 1, c = 0`` adds the same numbers in the same order. Small inputs only: every pair of a job is evaluated."""
import numpy as np

from shear_oracle import CHUNK_PAIRS, projection


def dsigma_jobs(lens, src, jobs, t):
    """``lens`` = dict(x, y, z, w | None, f, c, nb, off[int64 P*nb+1]), ``src`` = dict(x, y, z, w | None, g1, g2, u, off[int64
    P+1]), jobs int[n, 2] = (lens patch, source patch), t f64[B, E]. Returns ``(T, X, W, A)``, f64[n_jobs, B, E-1] each;
    ``A`` is the cancellation-free magnitude ``sum |w_l w_s| s (|g1| + |g2|)`` of a cell's pairs with ``eff > 0``."""
    t = np.asarray(t, dtype=np.float64)
    n_bins, n_edges = t.shape
    nf = n_edges - 1
    jobs = np.asarray(jobs).reshape(-1, 2)
    out = np.zeros((4, len(jobs), n_bins, nf), dtype=np.float64)
    for j, (p, q) in enumerate(jobs):
        a0, a1 = int(src["off"][q]), int(src["off"][q + 1])
        sx, sy, sz = (src[c][a0:a1] for c in "xyz")
        sw = np.ones(a1 - a0) if src["w"] is None else src["w"][a0:a1]
        g1, g2, su = src["g1"][a0:a1], src["g2"][a0:a1], src["u"][a0:a1]
        wg1, wg2 = (g1, g2) if src["w"] is None else (sw * g1, sw * g2)
        if a1 == a0:
            continue
        rows = max(1, CHUNK_PAIRS // (a1 - a0))
        for k in range(n_bins):
            seg = p * lens["nb"] + (0 if lens["nb"] == 1 else k)
            b0, b1 = int(lens["off"][seg]), int(lens["off"][seg + 1])
            for lo in range(b0, b1, rows):
                hi = min(lo + rows, b1)
                lx, ly, lz = (lens[c][lo:hi, None] for c in "xyz")
                lw = np.ones(hi - lo) if lens["w"] is None else lens["w"][lo:hi]
                lf, lc = lens["f"][lo:hi], lens["c"][lo:hi]
                dx, dy, dz = sx[None, :] - lx, sy[None, :] - ly, sz[None, :] - lz
                s2 = (dx * dx + dy * dy) + dz * dz
                il, isrc = np.nonzero((s2 > t[k, 0]) & (s2 <= t[k, -1]))
                if len(il) == 0:
                    continue
                eff = 1.0 - lc[il] * su[isrc]
                behind = eff > 0.0
                il, isrc, eff = il[behind], isrc[behind], eff[behind]
                if len(il) == 0:
                    continue
                s_in = s2[il, isrc]
                e = (s_in[:, None] > t[k][None, :]).sum(axis=1) - 1  # t[e] < s2 <= t[e+1]
                c2, s2p, den = projection(sx[isrc], sy[isrc], sz[isrc], lx[il, 0], ly[il, 0], lz[il, 0])
                s = lf[il] * eff
                ws = lw[il] * s
                pole = den == 0
                tv = np.where(pole, 0.0, ws * -(wg1[isrc] * c2 + wg2[isrc] * s2p))
                xv = np.where(pole, 0.0, ws * (wg1[isrc] * s2p - wg2[isrc] * c2))
                wv = (ws * s) * sw[isrc]
                av = np.abs(lw[il] * sw[isrc]) * s * (np.abs(g1[isrc]) + np.abs(g2[isrc]))
                for c, v in enumerate((tv, xv, wv, av)):
                    out[c, j, k] += np.bincount(e, weights=v, minlength=nf)
    return out[0], out[1], out[2], out[3]


def as_lens(layout, f, c):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, f=f, c=c, nb=layout.num_bins, off=layout.offsets)


def as_sources(layout, u):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, g1=layout.g1, g2=layout.g2, u=u, off=layout.offsets)


def count_dsigma_fine(lens_layout, source_layout, jobs, thresholds, *, cosmology, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_dsigma_fine`` built on the brute force: lets the CPU suite exercise
    the host driver without a GPU. The three columns are the engine's (``engine.dsigma_columns``), as on the device path."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    f, c, u = engine.dsigma_columns(lens_layout, source_layout, cosmology)
    T, X, W, _ = dsigma_jobs(as_lens(lens_layout, f, c), as_sources(source_layout, u), jobs, thresholds)
    return T, X, W, CountStats(candidate_pairs=0)


# --------------------------------------------------------------------------- physics, independent of the package's constant
C_M_S = 299792458.0
MPC_M = 3.085677581491367e22
GM_SUN = 1.32712440018e20  # m^3 s^-2
PC_M = MPC_M * 1e-6


def sigma_crit(cosmology, z_l, z_s):
    """Critical surface density in M_sun / pc^2 (physical) of a flat cosmology from its angular diameter distances:
    ``c^2 D_s / (4 pi G D_l D_ls)`` with ``D_ls = (chi_s - chi_l) / (1 + z_s)``; inf where the source is not behind the lens."""
    z_l, z_s = np.broadcast_arrays(np.asarray(z_l, dtype=np.float64), np.asarray(z_s, dtype=np.float64))
    d_l = np.asarray(cosmology.angular_diameter_distance(z_l.ravel())).reshape(z_l.shape) * MPC_M
    d_s = np.asarray(cosmology.angular_diameter_distance(z_s.ravel())).reshape(z_s.shape) * MPC_M
    chi_l = np.asarray(cosmology.comoving_distance(z_l.ravel())).reshape(z_l.shape) * MPC_M
    chi_s = np.asarray(cosmology.comoving_distance(z_s.ravel())).reshape(z_s.shape) * MPC_M
    d_ls = (chi_s - chi_l) / (1.0 + z_s)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_m2 = C_M_S**2 * d_s / (4.0 * np.pi * GM_SUN * d_l * d_ls)  # M_sun / m^2
    return np.where(d_ls > 0, per_m2 * PC_M**2, np.inf)


def sis_delta_sigma(sigma_v_km_s, r_mpc):
    """``Delta Sigma (R) = sigma_v^2 / (2 G R)`` of a singular isothermal sphere, M_sun / pc^2, ``R`` physical in Mpc."""
    return (sigma_v_km_s * 1e3) ** 2 / (2.0 * GM_SUN * np.asarray(r_mpc) * MPC_M) * PC_M**2
