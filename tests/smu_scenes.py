"""The scenes of the redshift-space count's tests (``yawhip_proj_count_smu``), shared by the CPU test
that checks the oracle's membership with mpmath (tests/test_smu_host.py) and the device tests (tests/test_gpu_smu.py): the
handles of tests/proj_scenes.py with the line-of-sight coordinate scaled by 2^-5 -- an exact scaling, so ``c`` is 0 .. 3.75
against radii of up to 5.4 and every mu from 0 to 1 is populated -- and its radius edges read as edges of ``s``."""
import functools

import numpy as np

import proj_scenes
from proj_scenes import SEED_A, SEED_B, cells_one_handle, cells_two_handles, unweighted  # noqa: F401 (the scenes' cells)

PER_SEGMENT = 24
C_SCALE = 2.0**-5
MU_4 = np.linspace(0.0, 1.0, 5)
MU_30 = np.linspace(0.0, 1.0, 31)
MU_UNEVEN = np.array([0.0, 0.05, 0.3, 0.55, 0.9, 1.0])
MU_SETS = {"uniform4": MU_4, "uniform30": MU_30, "uneven": MU_UNEVEN}


def squares(mu_edges):
    """What the engine hands the library: the float64 products ``mu * mu``."""
    mu_edges = np.asarray(mu_edges, dtype=np.float64)
    return mu_edges * mu_edges


def handle(seed, nb, weighted=True):
    h = proj_scenes.handle(seed, nb, PER_SEGMENT, weighted)
    h["c"] = h["c"] * C_SCALE
    return h


@functools.lru_cache(maxsize=None)
def scene(nb, weighted):
    """The two handles of the tests, made once per case and never modified."""
    a, b = handle(SEED_A, nb, weighted), handle(SEED_B, nb, weighted)
    for h in (a, b):
        for value in h.values():
            if isinstance(value, np.ndarray):
                value.setflags(write=False)
    return a, b


def s_edges(n_fine, n_rows):
    """Squared s edges f64[n_rows, n_fine + 1]: ``proj_scenes.radius_edges``."""
    return proj_scenes.radius_edges(n_fine, n_rows)
