"""numpy brute force of the excess-surface-density count binned in each lens's own radius (``yawhip_dsigma_count_radial``,
include/yawhip.h) over a job list, in the operation order of the contract:

    s2  = ((sx - lx)^2 + (sy - ly)^2) + (sz - lz)^2
    q   = 1/16632;  q = 1/3150 + s2*q;  q = 1/560 + s2*q;  q = 1/90 + s2*q;  q = 1/12 + s2*q;  q = 1 + s2*q
    th2 = s2*q;   R2 = m_l*th2;   fine bin e  iff  r2[k][e] < R2 <= r2[k][e + 1]

every product and sum rounded on its own (numpy contracts nothing). The pair term, the loops, the chunks and the order of the
pairs are those of tests/dsigma_oracle.py. Small inputs only: every pair of a job is evaluated."""
import numpy as np

from shear_oracle import CHUNK_PAIRS, projection

COEFFICIENTS = (1.0 / 16632.0, 1.0 / 3150.0, 1.0 / 560.0, 1.0 / 90.0, 1.0 / 12.0, 1.0)
S2_CAP = 0.01  # the largest squared chord the library accepts as a reach


def squared_angle(s2):
    """``(2 asin(sqrt(s2) / 2))^2`` by the contract's series, operation by operation."""
    s2 = np.asarray(s2, dtype=np.float64)
    q = np.full_like(s2, COEFFICIENTS[0])
    for coefficient in COEFFICIENTS[1:]:
        q = coefficient + s2 * q
    return s2 * q


def radial_jobs(lens, src, jobs, r2):
    """``lens`` = dict(x, y, z, w | None, f, c, m, nb, off[int64 P*nb+1]), ``src`` = dict(x, y, z, w | None, g1, g2, u, off[int64
    P+1]), jobs int[n, 2] = (lens patch, source patch), r2 f64[B, E]. Returns ``(T, X, W, A, A_theta)``, f64[n_jobs, B, E-1]
    each; ``A`` is the cancellation-free magnitude ``sum |w_l w_s| s (|g1| + |g2|)`` of a cell's pairs with ``eff > 0`` and
    ``A_theta`` the same sum with each pair over its angle (tests/shear_exact.py)."""
    r2 = np.asarray(r2, dtype=np.float64)
    n_bins, n_edges = r2.shape
    nf = n_edges - 1
    jobs = np.asarray(jobs).reshape(-1, 2)
    out = np.zeros((5, len(jobs), n_bins, nf), dtype=np.float64)
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
                lf, lc, lm = lens["f"][lo:hi], lens["c"][lo:hi], lens["m"][lo:hi]
                dx, dy, dz = sx[None, :] - lx, sy[None, :] - ly, sz[None, :] - lz
                s2 = (dx * dx + dy * dy) + dz * dz
                th2 = squared_angle(s2)
                R2 = lm[:, None] * th2
                il, isrc = np.nonzero((R2 > r2[k, 0]) & (R2 <= r2[k, -1]))
                if len(il) == 0:
                    continue
                eff = 1.0 - lc[il] * su[isrc]
                behind = eff > 0.0
                il, isrc, eff = il[behind], isrc[behind], eff[behind]
                if len(il) == 0:
                    continue
                R_in = R2[il, isrc]
                e = (R_in[:, None] > r2[k][None, :]).sum(axis=1) - 1  # r2[e] < R2 <= r2[e+1]
                c2, s2p, den = projection(sx[isrc], sy[isrc], sz[isrc], lx[il, 0], ly[il, 0], lz[il, 0])
                s = lf[il] * eff
                ws = lw[il] * s
                pole = den == 0
                tv = np.where(pole, 0.0, ws * -(wg1[isrc] * c2 + wg2[isrc] * s2p))
                xv = np.where(pole, 0.0, ws * (wg1[isrc] * s2p - wg2[isrc] * c2))
                wv = (ws * s) * sw[isrc]
                av = np.abs(lw[il] * sw[isrc]) * s * (np.abs(g1[isrc]) + np.abs(g2[isrc]))
                ath = av / np.sqrt(th2[il, isrc])
                for c, v in enumerate((tv, xv, wv, av, ath)):
                    out[c, j, k] += np.bincount(e, weights=v, minlength=nf)
    return tuple(out)


def nearest_margin(lens, src, jobs, r2):
    """The smallest ``|R2 / edge - 1|`` over every pair and every edge of its row (how far the scene stays off the edges)."""
    r2 = np.asarray(r2, dtype=np.float64)
    worst = np.inf
    for p, q in np.asarray(jobs).reshape(-1, 2):
        a0, a1 = int(src["off"][q]), int(src["off"][q + 1])
        for k in range(len(r2)):
            seg = p * lens["nb"] + (0 if lens["nb"] == 1 else k)
            b0, b1 = int(lens["off"][seg]), int(lens["off"][seg + 1])
            if a1 == a0 or b1 == b0:
                continue
            dx, dy, dz = (src[c][None, a0:a1] - lens[c][b0:b1, None] for c in "xyz")
            R2 = lens["m"][b0:b1, None] * squared_angle((dx * dx + dy * dy) + dz * dz)
            edges = r2[k][r2[k] > 0]
            worst = min(worst, float(np.min(np.abs(R2[:, :, None] / edges[None, None, :] - 1.0))))
    return worst


def as_lens(layout, f, c, m):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, f=f, c=c, m=m, nb=layout.num_bins, off=layout.offsets)


def as_sources(layout, u):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, g1=layout.g1, g2=layout.g2, u=u, off=layout.offsets)


def count_dsigma_radial_fine(lens_layout, source_layout, jobs, r2, *, cosmology, unit, sort_axis=2, unit_columns=False):
    """Stand-in for ``yet_another_wizz_amd.engine.count_dsigma_radial_fine`` built on the brute force: lets the CPU suite
    exercise the host driver without a GPU. The columns are the engine's (``engine.dsigma_radial_columns``), and so is the
    refusal of a reach beyond the cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    f, c, m, u = engine.dsigma_radial_columns(lens_layout, source_layout, cosmology, unit, unit_columns=unit_columns)
    engine.check_radial_reach(lens_layout, m, r2)
    T, X, W, _, _ = radial_jobs(as_lens(lens_layout, f, c, m), as_sources(source_layout, u), jobs, r2)
    return T, X, W, CountStats(candidate_pairs=0)
