"""numpy brute force of the shear-shear count (``yawhip_shear_auto_count``, include/yawhip.h) over a job
list.

Objects ``a``, ``b`` of the same redshift bin of one catalogue; pair membership is the count predicate,
``s2 = ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2`` in float64 with every product and sum rounded on its own and
``t[k][e] < s2 <= t[k][e+1]``; the rotation of the two shears follows the contract operation by operation:

    pa = ax*by - ay*bx;  dot = ax*bx + ay*by
    pbA = (ax*ax + ay*ay)*bz - az*dot;  pbB = (bx*bx + by*by)*az - bz*dot
    denA = pa*pa + pbA*pbA;  denB = pa*pa + pbB*pbB
    cA = (pa*pa - pbA*pbA)/denA;  sA = (2*pa*pbA)/denA;  cB = (pa*pa - pbB*pbB)/denB;  sB = ((-2*pa)*pbB)/denB
    tA = -(wg1a*cA + wg2a*sA);  xA = wg1a*sA - wg2a*cA;  tB = -(wg1b*cB + wg2b*sB);  xB = wg1b*sB - wg2b*cB
    P += tA*tB + xA*xB;  M += tA*tB - xA*xB;  C += tA*xB + xA*tB;  W += w_a*w_b        (a den == 0: W only)

with ``wg = w*g`` one product per object. A job ``(p, q)`` with ``p < q`` takes ``a`` from segment ``(p, k)`` and ``b`` from
``(q, k)``; ``p == q`` takes every unordered pair of the segment once. Small inputs only: every pair of a job is evaluated."""
import numpy as np


def rotations(ax, ay, az, bx, by, bz):
    """``(cA, sA, cB, sB, denA, denB)``: cos and sin of twice the position angle of ``b`` seen from ``a`` and of ``a`` seen from
    ``b``, from east towards north (nan where the den is 0)."""
    pa = ax * by - ay * bx
    dot = ax * bx + ay * by
    pbA = (ax * ax + ay * ay) * bz - az * dot
    pbB = (bx * bx + by * by) * az - bz * dot
    den_a = pa * pa + pbA * pbA
    den_b = pa * pa + pbB * pbB
    with np.errstate(invalid="ignore", divide="ignore"):
        c_a = (pa * pa - pbA * pbA) / den_a
        s_a = (2 * pa * pbA) / den_a
        c_b = (pa * pa - pbB * pbB) / den_b
        s_b = ((-2 * pa) * pbB) / den_b
    return c_a, s_a, c_b, s_b, den_a, den_b


def shear_auto_jobs(cat, jobs, t):
    """``cat`` = dict(x, y, z, w | None, g1, g2, nb, off[int64 P*nb+1]), jobs int[n, 2] with ``p <= q``, t f64[B, E] with
    ``B == nb``. Returns ``(P, M, C, W, A)``, f64[n_jobs, B, E-1] each; ``A`` is the cancellation-free magnitude
    ``sum |w_a w_b| (|g1a| + |g2a|) (|g1b| + |g2b|)`` of a cell's pairs."""
    t = np.asarray(t, dtype=np.float64)
    n_bins, n_edges = t.shape
    assert n_bins == cat["nb"]
    nf = n_edges - 1
    jobs = np.asarray(jobs).reshape(-1, 2)
    w = np.ones(len(cat["x"])) if cat["w"] is None else cat["w"]
    wg1, wg2 = (cat["g1"], cat["g2"]) if cat["w"] is None else (w * cat["g1"], w * cat["g2"])
    mag = np.abs(cat["g1"]) + np.abs(cat["g2"])
    out = np.zeros((5, len(jobs), n_bins, nf), dtype=np.float64)
    for j, (p, q) in enumerate(jobs):
        assert p <= q
        for k in range(n_bins):
            a0, a1 = (int(v) for v in cat["off"][p * n_bins + k: p * n_bins + k + 2])
            b0, b1 = (int(v) for v in cat["off"][q * n_bins + k: q * n_bins + k + 2])
            if a1 == a0 or b1 == b0:
                continue
            ax, ay, az = (cat[c][a0:a1, None] for c in "xyz")
            bx, by, bz = (cat[c][None, b0:b1] for c in "xyz")
            dx, dy, dz = ax - bx, ay - by, az - bz
            s2 = (dx * dx + dy * dy) + dz * dz
            inside = (s2 > t[k, 0]) & (s2 <= t[k, -1])
            if p == q:
                inside &= np.triu(np.ones_like(inside), 1)  # every unordered pair once
            ia, ib = np.nonzero(inside)
            if len(ia) == 0:
                continue
            e = (s2[ia, ib][:, None] > t[k][None, :]).sum(axis=1) - 1  # t[e] < s2 <= t[e+1]
            ia, ib = ia + a0, ib + b0
            c_a, s_a, c_b, s_b, den_a, den_b = rotations(*(cat[c][ia] for c in "xyz"), *(cat[c][ib] for c in "xyz"))
            t_a, x_a = -(wg1[ia] * c_a + wg2[ia] * s_a), wg1[ia] * s_a - wg2[ia] * c_a
            t_b, x_b = -(wg1[ib] * c_b + wg2[ib] * s_b), wg1[ib] * s_b - wg2[ib] * c_b
            pole = (den_a == 0) | (den_b == 0)
            terms = (np.where(pole, 0.0, t_a * t_b + x_a * x_b), np.where(pole, 0.0, t_a * t_b - x_a * x_b),
                     np.where(pole, 0.0, t_a * x_b + x_a * t_b), w[ia] * w[ib], np.abs(w[ia] * w[ib]) * mag[ia] * mag[ib])
            for c, v in enumerate(terms):
                out[c, j, k] += np.bincount(e, weights=v, minlength=nf)
    return tuple(out)


def as_catalogue(layout):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, g1=layout.g1, g2=layout.g2, nb=layout.num_bins, off=layout.offsets)


def count_shear_auto_fine(layout, jobs, thresholds, *, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_shear_auto_fine`` built on the brute force: lets the CPU suite
    exercise the host driver without a GPU."""
    from yet_another_wizz_amd._lib import CountStats

    P, M, C, W, _ = shear_auto_jobs(as_catalogue(layout), jobs, thresholds)
    return P, M, C, W, CountStats(candidate_pairs=0)
