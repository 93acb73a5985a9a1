"""numpy brute force of the shear-shear count between two (patch, bin) segments of one or two catalogues
(``yawhip_shear_pair_count``, include/yawhip.h) over a cell list.

A cell ``(p, q, ka, kb, row)`` takes ``a`` from segment ``(p, ka)`` of catalogue ``cat_a`` and ``b`` from segment ``(q, kb)`` of
``cat_b``; membership is ``t[row][e] < s2 <= t[row][e+1]`` with the ``s2`` of every count, and the pair term is the one of
tests/shear_auto_oracle.py, built on its ``rotations``. A cell is diagonal iff ``cat_a is cat_b``, ``ka == kb`` and ``p == q``:
it takes every unordered pair of the segment once. Small inputs only: every pair of a cell is evaluated."""
import numpy as np

from shear_auto_oracle import as_catalogue, rotations


def _columns(cat):
    w = np.ones(len(cat["x"])) if cat["w"] is None else cat["w"]
    wg1, wg2 = (cat["g1"], cat["g2"]) if cat["w"] is None else (w * cat["g1"], w * cat["g2"])
    return w, wg1, wg2, np.abs(cat["g1"]) + np.abs(cat["g2"])


def shear_pair_cells(cat_a, cat_b, cells, t):
    """``cat_*`` = dict(x, y, z, w | None, g1, g2, nb, off[int64 P*nb+1]) (the same object twice: one catalogue), cells
    int[n, 5], t f64[n_rows, E]. Returns ``(P, M, C, W, A)``, f64[n_cells, E-1] each; ``A`` is the cancellation-free magnitude
    ``sum |w_a w_b| (|g1a| + |g2a|) (|g1b| + |g2b|)`` of a cell's pairs."""
    t = np.asarray(t, dtype=np.float64)
    nf = t.shape[1] - 1
    cells = np.asarray(cells).reshape(-1, 5)
    w_a, wg1_a, wg2_a, mag_a = _columns(cat_a)
    w_b, wg1_b, wg2_b, mag_b = _columns(cat_b)
    out = np.zeros((5, len(cells), nf), dtype=np.float64)
    for c, (p, q, ka, kb, row) in enumerate(cells):
        sa, sb = p * cat_a["nb"] + ka, q * cat_b["nb"] + kb
        a0, a1 = (int(v) for v in cat_a["off"][sa: sa + 2])
        b0, b1 = (int(v) for v in cat_b["off"][sb: sb + 2])
        if a1 == a0 or b1 == b0:
            continue
        ax, ay, az = (cat_a[col][a0:a1, None] for col in "xyz")
        bx, by, bz = (cat_b[col][None, b0:b1] for col in "xyz")
        dx, dy, dz = ax - bx, ay - by, az - bz
        s2 = (dx * dx + dy * dy) + dz * dz
        inside = (s2 > t[row, 0]) & (s2 <= t[row, -1])
        if cat_a is cat_b and sa == sb:
            inside &= np.triu(np.ones_like(inside), 1)  # every unordered pair once
        ia, ib = np.nonzero(inside)
        if len(ia) == 0:
            continue
        e = (s2[ia, ib][:, None] > t[row][None, :]).sum(axis=1) - 1  # t[e] < s2 <= t[e+1]
        ia, ib = ia + a0, ib + b0
        c_a, s_a, c_b, s_b, den_a, den_b = rotations(*(cat_a[col][ia] for col in "xyz"), *(cat_b[col][ib] for col in "xyz"))
        t_a, x_a = -(wg1_a[ia] * c_a + wg2_a[ia] * s_a), wg1_a[ia] * s_a - wg2_a[ia] * c_a
        t_b, x_b = -(wg1_b[ib] * c_b + wg2_b[ib] * s_b), wg1_b[ib] * s_b - wg2_b[ib] * c_b
        pole = (den_a == 0) | (den_b == 0)
        terms = (np.where(pole, 0.0, t_a * t_b + x_a * x_b), np.where(pole, 0.0, t_a * t_b - x_a * x_b),
                 np.where(pole, 0.0, t_a * x_b + x_a * t_b), w_a[ia] * w_b[ib], np.abs(w_a[ia] * w_b[ib]) * mag_a[ia] * mag_b[ib])
        for plane, v in enumerate(terms):
            out[plane, c] += np.bincount(e, weights=v, minlength=nf)
    return tuple(out)


def count_shear_pair_fine(layout_a, layout_b, cells, thresholds, *, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_shear_pair_fine`` built on the brute force: lets the CPU suite
    exercise the host driver without a GPU. The same layout twice is one catalogue, as it is one handle on the device."""
    from yet_another_wizz_amd._lib import CountStats

    cat_a = as_catalogue(layout_a)
    cat_b = cat_a if layout_b is layout_a else as_catalogue(layout_b)
    P, M, C, W, _ = shear_pair_cells(cat_a, cat_b, cells, thresholds)
    return P, M, C, W, CountStats(candidate_pairs=0)
