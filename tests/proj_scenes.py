"""The scenes of the projected-count tests (``yawhip_proj_count``), shared by the CPU test that checks
the oracle's membership with mpmath (tests/test_projected_host.py) and the device tests (tests/test_gpu_projected.py): the
same generator and the same seeds, so that what is proven of the oracle on the CPU is what the device is held to."""
import numpy as np

from yet_another_wizz_amd.catalog import radec_to_xyz

# four sites of the kind of DESIGN.md section 15: on the equator, at 60 degrees, next to a pole, across the RA wrap
SITES = ((0.7, 0.0), (2.1, np.deg2rad(60.0)), (4.0, np.deg2rad(89.99)), (2.0 * np.pi - 1e-7, 0.3))
SEED_A, SEED_B = 11, 12  # chosen on the CPU: no pair within 1e-9 of an edge or of PMAX (asserted in both test modules)
PMAX = 40.0
DISC = 1.6e-3  # radian: the radius of a site's disc; at d = 800 .. 1700 the pairs reach 5.4 in radius


def disc_around(rng, ra_c, dec_c, n, radius):
    """``n`` points uniform in a disc of ``radius`` (radian) around (ra_c, dec_c), as unit vectors ``(x, y, z)``."""
    r, phi = radius * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * np.pi, n)
    centre = np.array([np.cos(dec_c) * np.cos(ra_c), np.cos(dec_c) * np.sin(ra_c), np.sin(dec_c)])
    east = np.array([-np.sin(ra_c), np.cos(ra_c), 0.0])
    north = np.cross(centre, east)
    xyz = np.cos(r)[:, None] * centre + np.sin(r)[:, None] * (np.cos(phi)[:, None] * east + np.sin(phi)[:, None] * north)
    xyz /= np.sqrt((xyz * xyz).sum(axis=1))[:, None]
    return xyz[:, 0], xyz[:, 1], xyz[:, 2]


def handle(seed, nb, per_segment, weighted=True):
    """A projected catalogue as the oracle takes it (tests/proj_oracle.py): two patches per site over the same disc, ``nb``
    redshift bins per patch, ``per_segment`` objects per (patch, bin) -- one more in every third segment, and segment 5 empty
    where there are more than 8. ``d`` is 800 .. 1700 (bin k of it shifted by 5 %), ``c`` 0 .. 120."""
    rng = np.random.default_rng(seed)
    cols, sizes = [], []
    for site, (ra_c, dec_c) in enumerate(SITES):
        for patch in (2 * site, 2 * site + 1):
            for k in range(nb):
                seg = patch * nb + k
                n = 0 if (seg == 5 and nb > 1) else per_segment + (seg % 3 == 0)
                x, y, z = disc_around(rng, ra_c, dec_c, n, DISC)
                cols.append((x, y, z, rng.uniform(0.5, 1.5, n), rng.uniform(800.0, 1700.0, n) * (1.0 + 0.05 * k), rng.uniform(0.0, 120.0, n)))
                sizes.append(n)
    x, y, z, w, d, c = (np.concatenate([col[i] for col in cols]) for i in range(6))
    return dict(x=x, y=y, z=z, w=w if weighted else None, d=d, c=c, nb=nb, off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                n_patches=2 * len(SITES))


def radius_edges(n_fine, n_rows):
    """Squared radius edges f64[n_rows, n_fine + 1]: 0.3 .. 4.5 in radius, logarithmic, row k stretched by 3 % per row."""
    edges = np.geomspace(0.3, 4.5, n_fine + 1)
    return np.array([(edges * (1.0 + 0.03 * k)) ** 2 for k in range(n_rows)])


def cells_one_handle(nb, n_sites=len(SITES)):
    """Every diagonal cell, and the two patches of every site against each other in every bin; row = bin."""
    n_patches = 2 * n_sites
    cells = [(p * nb + k, p * nb + k, k, 1) for p in range(n_patches) for k in range(nb)]
    cells += [(2 * s * nb + k, (2 * s + 1) * nb + k, k, 0) for s in range(n_sites) for k in range(nb)]
    return np.array(cells, dtype=np.int32)


def cells_two_handles(nb, n_sites=len(SITES)):
    """Patch p of the first handle against the patches of the same site of the second, bin k with bin k; row = bin."""
    cells = [(p * nb + k, q * nb + k, k, 0) for p in range(2 * n_sites) for q in (p, p ^ 1) for k in range(nb)]
    return np.array(cells, dtype=np.int32)


def unweighted(h):
    return dict(h, w=None)
