"""Patch centres from a deterministic k-means over ALL objects of a catalogue (``patch_method="full"``).

``create_patch_centers`` stands in for the treecorr k-means behind the reference's ``create_patch_centers``
(src/yaw/catalog/catalog.py:183-226). It has two routes that return the same centres bit for bit: the numpy route of this
module, which is the oracle, and the device route (``csrc/yawhip_kmeans.hip`` behind ``_lib.KMeans``), on which the columns
are uploaded once and only centre tables and scalars move afterwards. What makes the routes equal is that everything summed
over objects is an INTEGER: integer addition is associative, so numpy's blocked sums, the device's atomics and
per-workgroup partials, and any grid shape give the same bits, run after run.

The algorithm
-------------
Inputs: unit vectors ``x, y, z`` (float64, ``radec_to_xyz``), optional finite weights ``w`` (float64), ``k = patch_num``,
``seed``, ``max_iterations``; ``k <= n <= 2^31`` objects.

Distance. ``d(i, c) = ((x_i - c_x)^2 + (y_i - c_y)^2) + (z_i - c_z)^2``, every product and sum rounded on its own (no
FMA): the arithmetic of ``yawhip_assign_patches``. Among equal distances the lowest centre index wins.

Seeding (k-means++ on integers; unweighted, as ``catalog.kmeans_centers`` seeds).

1. ``rng = np.random.default_rng(seed)``; the first centre is the point at index ``rng.integers(n)``.
2. ``m_i`` = the smallest ``d(i, c)`` over the centres chosen so far.
3. ``q_i = floor(m_i * 2^29)`` as an unsigned integer (``d <= 4``, so ``q_i <= 2^31``).
4. ``T = sum q_i``, exact and below 2^63.
5. ``T == 0``: fewer distinct points than ``k`` -- ``ValueError``.
6. ``r = rng.integers(T)``; the next centre is the point with the smallest index ``i`` whose inclusive prefix sum of ``q``
   exceeds ``r`` (a point with ``q_i = 0`` is never drawn).
7. Back to 2 until there are ``k`` centres.

Lloyd round.

1. ``id_i = argmin_c d(i, c)``.
2. Per cluster, in int64: the count ``N_c`` and, per axis, ``S_c = sum a_i`` with ``a_i = rint(x_i * 2^30)``. With weights
   ``a_i = rint((w_i * x_i) * s)``, ``s = 2^(30 - e)`` a float64 and ``e`` the exponent ``np.frexp(max |w|)`` returns: one
   IEEE product ``w_i * x_i``, one IEEE multiplication by ``s`` (exact unless it leaves the normal range), then
   round-half-even. ``max |w| == 0`` or ``e`` outside [-900, 900] is a ``ValueError``.
3. The integer inertia ``J = sum floor(d(i, id_i) * 2^29)``. It is not weighted: it decreases from round to round (up to
   the quantisation, below ``4 n``) in unweighted runs, where the centre update minimises it, and is a diagnostic otherwise.
4. ``|a_i| <= 2^30`` and ``n <= 2^31``: nothing overflows.
5. Centre update (``update_centres``, on the host for both routes): ``S`` as float64, ``c = S / sqrt((S_x^2 + S_y^2) +
   S_z^2)``; a cluster with ``N_c == 0`` or a zero norm keeps its centre.
6. Stop when ``(S, N)`` equal those of the round before exactly -- a fixed point, which both routes reach in the same
   round -- or after ``max_iterations`` rounds.

Not built: treecorr's variant that balances the patch sizes, and weighted seeding.
"""
from __future__ import annotations

import time

import numpy as np

from . import _threads
from .coordinates import AngularCoordinates

__all__ = ["create_patch_centers", "centers_from_xyz", "numpy_round", "update_centres", "weight_scale", "DEVICE_KMEANS_MIN"]

# Objects from which the device route is taken when there is a device: the smallest catalogue measured on an MI355X
# (9 ms against numpy's 0.39 s at 64 patches, context already open). It is not a break-even -- that
# lies below and has not been located.
DEVICE_KMEANS_MIN = 20_000
HOST_BLOCK: int | None = None  # objects per block of the numpy route's passes; None: sized so that a block's distance table
                               # holds 2^17 values and stays in cache (the results do not depend on it)
N_MAX = 1 << 31
Q_SCALE = 2.0 ** 29  # q = floor(d * Q_SCALE): d <= 4 -> q <= 2^31
A_SCALE = 2.0 ** 30  # a = rint(x * A_SCALE): |x| <= 1 -> |a| <= 2^30
_SPLIT = 15          # a = hi * 2^15 + lo: np.bincount adds float64 weights, and both parts sum exactly below 2^53


def weight_scale(weights) -> float:
    """``s = 2^(30 - e)`` with ``e`` the binary exponent of ``max |w|``: ``|w x s| < 2^30`` for every ``|x| <= 1``.
    ``ValueError`` for weights that are all zero or whose largest lies outside 2^±900."""
    wmax = float(np.max(np.abs(weights)))
    if not wmax > 0.0:
        raise ValueError("k-means weights are all zero")
    _, e = np.frexp(wmax)
    if abs(int(e)) > 900:
        raise ValueError(f"largest k-means weight {wmax:g} is outside the supported range 2^-900 .. 2^900")
    return float(np.ldexp(1.0, 30 - int(e)))


def _dist2(x, y, z, cx, cy, cz):
    dx, dy, dz = x - cx, y - cy, z - cz
    return (dx * dx + dy * dy) + dz * dz


def _fixed_point(col, w, wscale):
    return np.rint(col * A_SCALE if w is None else (w * col) * wscale).astype(np.int64)


def _block_size(n: int, row: int = 1) -> int:
    if HOST_BLOCK is not None:
        return max(1, int(HOST_BLOCK))
    return max(1, min(n, (1 << 17) // max(row, 1)))


def numpy_round(x, y, z, centres, weights=None, wscale: float | None = None):
    """One Lloyd round on the host against ``centres`` float64[k, 3] -> ``(S int64[k, 3], N int64[k], J int, ids int32[n])``
    (steps 1 to 3 of the module docstring). The distance table is made in blocks of bounded size, side by side in the
    host thread pool where it is large: the blocks' integer sums add up to the same values in any order."""
    centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
    k, n = len(centres), len(x)
    if weights is not None and wscale is None:
        wscale = weight_scale(weights)
    ids = np.empty(n, dtype=np.int32)
    cx, cy, cz = centres[None, :, 0], centres[None, :, 1], centres[None, :, 2]
    block = _block_size(n, k)  # rows of one distance table
    chunk = block if HOST_BLOCK is not None else max(block, min(n, 1 << 14))  # rows of one set of integer sums

    def one_chunk(lo):
        hi = min(n, lo + chunk)
        nearest, best = np.empty(hi - lo, dtype=np.intp), np.empty(hi - lo, dtype=np.float64)
        for b0 in range(lo, hi, block):
            sl = slice(b0, min(hi, b0 + block))
            d = x[sl, None] - cx  # ((x - c_x)^2 + (y - c_y)^2) + (z - c_z)^2 in two buffers: the values of _dist2
            np.multiply(d, d, out=d)
            for col, c in ((y, cy), (z, cz)):
                t = col[sl, None] - c
                np.multiply(t, t, out=t)
                np.add(d, t, out=d)
            first = d.argmin(axis=1)  # first minimum
            nearest[b0 - lo : sl.stop - lo] = first
            best[b0 - lo : sl.stop - lo] = d[np.arange(len(first)), first]
        sl = slice(lo, hi)
        ids[sl] = nearest
        inertia = int(np.floor(best * Q_SCALE).astype(np.uint64).sum(dtype=np.uint64))
        sums = np.empty((k, 3), dtype=np.int64)
        w = None if weights is None else weights[sl]
        for axis, col in enumerate((x, y, z)):
            a = _fixed_point(col[sl], w, wscale)
            high = np.bincount(nearest, weights=a >> _SPLIT, minlength=k).astype(np.int64)
            low = np.bincount(nearest, weights=a & ((1 << _SPLIT) - 1), minlength=k).astype(np.int64)
            sums[:, axis] = (high << _SPLIT) + low
        return sums, np.bincount(nearest, minlength=k), inertia

    starts = range(0, n, chunk)
    if len(starts) > 1 and n * k >= _threads.MIN_PARALLEL and _threads.pool_size() > 1:
        parts = list(_threads._executor().map(one_chunk, starts))
    else:
        parts = [one_chunk(lo) for lo in starts]
    sums, counts = np.zeros((k, 3), dtype=np.int64), np.zeros(k, dtype=np.int64)
    inertia = 0
    for s, c, j in parts:
        sums += s
        counts += c
        inertia += j
    return sums, counts, inertia, ids


def update_centres(sums, counts, centres):
    """Step 5: the centres after a round with per-cluster ``sums`` int64[k, 3] and ``counts`` int64[k] (both routes)."""
    s = sums.astype(np.float64)
    norm = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    keep = (counts == 0) | ~(norm > 0.0)
    out = np.array(centres, dtype=np.float64, copy=True)
    moved = ~keep
    out[moved] = s[moved] / norm[moved, None]
    return out


class _HostRoute:
    """The numpy route: seed / pick / step as ``_lib.KMeans`` has them."""

    name = "numpy"

    def __init__(self, x, y, z, weights, wscale):
        self.x, self.y, self.z, self.w, self.wscale = x, y, z, weights, wscale
        self.n = len(x)
        self.m = np.empty(self.n, dtype=np.float64)
        self.q = np.empty(self.n, dtype=np.uint32)  # q <= 2^31
        self.block_sums: list = []
        self.block = 1
        self.step_path = None

    def seed(self, centre, first: bool) -> int:
        cx, cy, cz = (float(v) for v in centre)
        self.block = _block_size(self.n, 4)
        self.block_sums = []
        for lo in range(0, self.n, self.block):
            sl = slice(lo, min(self.n, lo + self.block))
            d = _dist2(self.x[sl], self.y[sl], self.z[sl], cx, cy, cz)
            if not first:
                d = np.minimum(self.m[sl], d)
            self.m[sl] = d
            q = np.floor(d * Q_SCALE).astype(np.uint64)
            self.q[sl] = q
            self.block_sums.append(int(q.sum(dtype=np.uint64)))
        return sum(self.block_sums)

    def pick(self, r: int) -> int:
        before = 0
        for b, total in enumerate(self.block_sums):
            if before + total > r:
                lo = b * self.block
                prefix = np.cumsum(self.q[lo : lo + self.block], dtype=np.uint64)
                return lo + int(np.searchsorted(prefix, np.uint64(r - before), side="right"))
            before += total
        raise ValueError("r is not below the total")

    def step(self, centres):
        return numpy_round(self.x, self.y, self.z, centres, self.w, self.wscale)[:3]

    def close(self) -> None:
        pass


class _DeviceRoute:
    name = "device"

    def __init__(self, handle):
        self.km = handle
        self.step_path = None

    def seed(self, centre, first: bool) -> int:
        return self.km.seed(centre, first)

    def pick(self, r: int) -> int:
        return self.km.pick(r)

    def step(self, centres):
        sums, counts, inertia, _ = self.km.step(centres)
        self.step_path = self.km.last_path
        return sums, counts, inertia

    def close(self) -> None:
        self.km.close()


def _open_route(x, y, z, weights, wscale, k: int):
    n = len(x)
    if n >= DEVICE_KMEANS_MIN:
        from . import engine

        handle = engine.kmeans_open(x, y, z, weights, wscale or 0.0)
        if handle is not None:
            if k <= handle.max_centres:
                return _DeviceRoute(handle)
            handle.close()  # the centre table does not fit the LDS: the numpy route computes the same values
    return _HostRoute(x, y, z, weights, wscale)


def centers_from_xyz(xyz, weights, patch_num: int, *, seed: int = 12345, max_iterations: int = 100, return_info: bool = False):
    """``create_patch_centers`` for unit vectors that exist already: ``xyz`` is a tuple of three float64 columns."""
    if not isinstance(patch_num, (int, np.integer)):
        raise TypeError("'patch_num' must be an integer")
    k = int(patch_num)
    if k < 1:
        raise ValueError("'patch_num' must be at least 1")
    if int(max_iterations) < 0:
        raise ValueError("'max_iterations' must not be negative")
    x, y, z = (np.ascontiguousarray(c, dtype=np.float64) for c in xyz)
    n = len(x)
    if not (len(y) == n and len(z) == n):
        raise ValueError("input columns differ in length")
    if n < k:
        raise ValueError(f"cannot make {k} patches from {n} objects")
    if n > N_MAX:
        raise ValueError("the k-means takes at most 2^31 objects")
    wscale = None
    if weights is not None:
        weights = np.ascontiguousarray(np.asarray_chkfinite(weights, dtype=np.float64))
        if len(weights) != n:
            raise ValueError("input columns differ in length")
        wscale = weight_scale(weights)

    t_open = time.perf_counter()
    route = _open_route(x, y, z, weights, wscale, k)
    try:
        t_seed = time.perf_counter()
        rng = np.random.default_rng(seed)
        chosen = [int(rng.integers(n))]
        while len(chosen) < k:
            i = chosen[-1]
            total = route.seed((x[i], y[i], z[i]), len(chosen) == 1)
            if total == 0:
                raise ValueError(f"fewer distinct points than patches: {len(chosen)} < {k}")
            chosen.append(route.pick(int(rng.integers(total))))
        index = np.array(chosen, dtype=np.int64)
        centres = np.column_stack([x[index], y[index], z[index]])
        t_lloyd = time.perf_counter()
        inertia, previous, converged, sums, counts = [], None, False, None, None
        while len(inertia) < int(max_iterations):
            sums, counts, j = route.step(centres)
            inertia.append(int(j))
            if previous is not None and np.array_equal(sums, previous[0]) and np.array_equal(counts, previous[1]):
                converged = True  # the update would return these centres again
                break
            centres = update_centres(sums, counts, centres)
            previous = (sums, counts)
        info = dict(iterations=len(inertia), converged=converged, inertia=inertia, counts=counts, sums=sums, route=route.name,
                    step_path=route.step_path, seeds=index, open_s=t_seed - t_open, seed_s=t_lloyd - t_seed,
                    lloyd_s=time.perf_counter() - t_lloyd)
    finally:
        route.close()
    coords = AngularCoordinates.from_3d(centres)
    return (coords, info) if return_info else coords


def create_patch_centers(ra, dec, patch_num: int, *, weights=None, degrees: bool = True, seed: int = 12345,
                         max_iterations: int = 100, return_info: bool = False):
    """``patch_num`` patch centres (``AngularCoordinates``) from the k-means of the module docstring over all objects
    ``(ra, dec)``, with ``weights`` in the centre update. Deterministic for given inputs, and the same on the device and
    on the host: the device route is taken from ``DEVICE_KMEANS_MIN`` objects when there is a device, else the numpy route.
    With ``return_info`` also a dict: ``iterations`` (Lloyd rounds run), ``converged`` (stopped on a repeated ``(S, N)``),
    ``inertia`` (``J`` of every round), ``counts`` and ``sums`` (``N``, ``S`` of the last round), ``route`` (``"device"`` /
    ``"numpy"``), ``step_path`` (device route: ``"lds"`` / ``"global"``), ``seeds`` (indices of the seeding's points) and the
    wall times ``open_s`` (upload), ``seed_s`` and ``lloyd_s``."""
    ra = np.asarray_chkfinite(ra, dtype=np.float64)
    dec = np.asarray_chkfinite(dec, dtype=np.float64)
    if degrees:
        ra, dec = np.deg2rad(ra), np.deg2rad(dec)
    return centers_from_xyz(_threads.radec_to_xyz(ra, dec), weights, patch_num, seed=seed, max_iterations=max_iterations,
                            return_info=return_info)
