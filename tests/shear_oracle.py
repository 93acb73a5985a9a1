"""numpy brute force of the shear count (``yawhip_shear_count``, include/yawhip.h) over a job list.

Pair membership is the count predicate, ``s2 = ((sx-lx)^2 + (sy-ly)^2) + (sz-lz)^2`` in float64 with every product and sum
rounded on its own and ``t[k][e] < s2 <= t[k][e+1]``; the projection follows the contract operation by operation:

    a = x*ly - y*lx;  rho2 = x*x + y*y;  b = rho2*lz - z*(x*lx + y*ly);  den = a*a + b*b
    c2 = (a*a - b*b)/den;  s2p = (2*a*b)/den;  ww = w_l*w_s
    T += ww * -(g1*c2 + g2*s2p);  X += ww * (g1*s2p - g2*c2);  W += ww        (den == 0: W only)

with (x, y, z) the source and (lx, ly, lz) the lens. Small inputs only: every pair of a job is evaluated."""
import numpy as np

CHUNK_PAIRS = 4_000_000


def projection(x, y, z, lx, ly, lz):
    """``(c2, s2p, den)`` of sources (x, y, z) and lenses (lx, ly, lz), broadcast against each other: cos and sin of twice the
    position angle of the lens seen from the source, from east towards north (nan where ``den == 0``)."""
    a = x * ly - y * lx
    rho2 = x * x + y * y
    b = rho2 * lz - z * (x * lx + y * ly)
    a2, b2 = a * a, b * b
    den = a2 + b2
    with np.errstate(invalid="ignore", divide="ignore"):
        c2 = (a2 - b2) / den
        s2p = (2 * a * b) / den
    return c2, s2p, den


def shear_jobs(lens, src, jobs, t):
    """``lens`` = dict(x, y, z, w | None, nb, off[int64 P*nb+1]), ``src`` = dict(x, y, z, w | None, g1, g2, off[int64 P+1]), jobs
    int[n, 2] = (lens patch, source patch), t f64[B, E]. Returns ``(T, X, W, A)``, f64[n_jobs, B, E-1] each; ``A`` is the
    cancellation-free magnitude ``sum |ww| (|g1| + |g2|)`` of a cell's pairs."""
    t = np.asarray(t, dtype=np.float64)
    n_bins, n_edges = t.shape
    nf = n_edges - 1
    jobs = np.asarray(jobs).reshape(-1, 2)
    out = np.zeros((4, len(jobs), n_bins, nf), dtype=np.float64)
    for j, (p, q) in enumerate(jobs):
        a0, a1 = int(src["off"][q]), int(src["off"][q + 1])
        sx, sy, sz = (src[c][a0:a1] for c in "xyz")
        sw = np.ones(a1 - a0) if src["w"] is None else src["w"][a0:a1]
        g1, g2 = src["g1"][a0:a1], src["g2"][a0:a1]
        if a1 == a0:
            continue
        rows = max(1, CHUNK_PAIRS // (a1 - a0))
        for k in range(n_bins):
            seg = p * lens["nb"] + (0 if lens["nb"] == 1 else k)
            b0, b1 = int(lens["off"][seg]), int(lens["off"][seg + 1])
            for lo in range(b0, b1, rows):
                hi = min(lo + rows, b1)
                lx, ly, lz = (lens[c][lo:hi, None] for c in "xyz")
                lw = np.ones((hi - lo, 1)) if lens["w"] is None else lens["w"][lo:hi, None]
                dx, dy, dz = sx[None, :] - lx, sy[None, :] - ly, sz[None, :] - lz
                s2 = (dx * dx + dy * dy) + dz * dz
                il, isrc = np.nonzero((s2 > t[k, 0]) & (s2 <= t[k, -1]))
                if len(il) == 0:
                    continue
                s_in = s2[il, isrc]
                e = (s_in[:, None] > t[k][None, :]).sum(axis=1) - 1  # t[e] < s2 <= t[e+1]
                c2, s2p, den = projection(sx[isrc], sy[isrc], sz[isrc], lx[il, 0], ly[il, 0], lz[il, 0])
                ww = lw[il, 0] * sw[isrc]
                pole = den == 0
                tv = np.where(pole, 0.0, ww * -(g1[isrc] * c2 + g2[isrc] * s2p))
                xv = np.where(pole, 0.0, ww * (g1[isrc] * s2p - g2[isrc] * c2))
                av = np.abs(ww) * (np.abs(g1[isrc]) + np.abs(g2[isrc]))
                for c, v in enumerate((tv, xv, ww, av)):
                    out[c, j, k] += np.bincount(e, weights=v, minlength=nf)
    return out[0], out[1], out[2], out[3]


def as_lens(layout):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, nb=layout.num_bins, off=layout.offsets)


def as_sources(layout):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, g1=layout.g1, g2=layout.g2, off=layout.offsets)


def count_shear_fine(lens_layout, source_layout, jobs, thresholds, *, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_shear_fine`` built on the brute force: lets the CPU suite exercise
    the host driver without a GPU."""
    from yet_another_wizz_amd._lib import CountStats

    T, X, W, _ = shear_jobs(as_lens(lens_layout), as_sources(source_layout), jobs, thresholds)
    return T, X, W, CountStats(candidate_pairs=0)


def tangential_pattern(ra, dec, ra_l, dec_l, amplitude):
    """``(g1, g2)`` of a pure tangential shear of ``amplitude`` around the lens at (ra_l, dec_l), radian, from the
    spherical-trigonometry position angle of the lens seen from the source (independent of ``projection``)."""
    phi = position_angle(ra, dec, ra_l, dec_l)
    return -amplitude * np.cos(2 * phi), -amplitude * np.sin(2 * phi)


def position_angle(ra, dec, ra_l, dec_l):
    """Angle of the great circle from the source (ra, dec) towards the lens, from east towards north: pi/2 minus the
    bearing from north towards east of spherical trigonometry."""
    dra = ra_l - ra
    east = np.cos(dec_l) * np.sin(dra)
    north = np.cos(dec) * np.sin(dec_l) - np.sin(dec) * np.cos(dec_l) * np.cos(dra)
    return np.arctan2(north, east)
