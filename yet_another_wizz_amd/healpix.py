"""HEALPix pixels and maps of points on the sphere: what the reference leaves to healpy's ``ang2pix`` and ``np.bincount``
when it prepares the mask of a ``HealPixRandoms``. No healpy.

:func:`ang2pix` is HEALPix' ``loc2pix`` (Gorski et al. 2005, section 4.1) for ``(phi, z) = (ra in radian, sin dec)``, the pair
the random generators emit and a catalogue holds. Every float64 step is one IEEE operation in a fixed order, without a
transcendental::

    r = fmod(phi, 2 pi);  r < 0: r = r + 2 pi;  r >= 2 pi: r = 0;  tt = r / (pi / 2)
    belt, |z| <= 2/3:
        t1 = nside * (0.5 + tt);  t2 = nside * z * 0.75
        jp = min(floor(t1 - t2), 5 nside - 1);  jm = min(floor(t1 + t2), 5 nside - 1)
        ifp = jp >> order;  ifm = jm >> order;  face = ifp | 4 if ifp == ifm, ifp if ifp < ifm, else ifm + 8
        ix = jm & (nside - 1);  iy = nside - (jp & (nside - 1)) - 1
    caps:
        ntt = min(3, int(tt));  tp = tt - ntt;  tmp = nside * sqrt(3 * (1 - |z|))
        jp = min(int(tp * tmp), nside - 1);  jm = min(int((1 - tp) * tmp), nside - 1)
        north: face = ntt, ix = nside - jm - 1, iy = nside - jp - 1;  south: face = ntt + 8, ix = jp, iy = jm
    pixel = face * nside^2 + spread(ix) + 2 * spread(iy)

(``5 nside - 1``: with ``tt`` one step below 4, ``0.5 + tt`` rounds to 4.5 and at ``|z| = 2/3`` an edge line gets the index
``5 nside``, one past the last; the point lies on the corner of the pixel one below.) The RING number of a point is
``randoms.nest2ring`` of its nested pixel: one arithmetic path, two numberings that cannot disagree. Near a pole the
resolution is that of ``1 - |z|``, as for the generators.

The plain-numpy route here is the oracle of the device route (``yawhip_healpix_map``, ``csrc/yawhip_healpix.hip``), which
repeats it bit for bit and is taken from :data:`DEVICE_MAP_MIN` points on when there is a GPU.

:func:`map_pixels` goes the other way, from a full-sky scalar map (a convergence map, a y-map) to the columns of a
catalogue: the unmasked pixels in ascending nested number, their centres (``randoms.pix2loc_nest``), values and weights
(DESIGN.md section 13); its device route is ``yawhip_healpix_pixels``, from :data:`DEVICE_PIXELS_MIN` pixels on.
:func:`map_values` samples a map at positions.
"""
from __future__ import annotations

import math

import numpy as np

from .randoms import MAX_MAP_ORDER, nest2ring, pix2loc_nest

__all__ = ["ang2pix", "healpix_map", "map_pixels", "map_values", "nside2order", "UNSEEN"]

DEVICE_MAP_MIN = 200_000  # points from which the device route is taken: catalog.DEVICE_ASSIGN_MIN until measured
# pixels of a map from which map_pixels takes the device route: nside 64, the smallest map measured, where the device route
# already took a fifth of the numpy route's time; the break-even lies below and has not been located
DEVICE_PIXELS_MIN = 49_152
UNSEEN = -1.6375e30  # healpy's sentinel of a pixel without data
_TWOPI = 2.0 * np.pi
_HALFPI = np.pi / 2
_TWOTHIRD = 2.0 / 3.0
_HOST_STEP = 1 << 22  # points per slice of the numpy route: bounds its temporaries


def nside2order(nside) -> int:
    """Order of a map of ``nside``; ValueError unless ``nside`` is a power of two up to ``2^MAX_MAP_ORDER`` (8192)."""
    if isinstance(nside, (bool, np.bool_)) or not isinstance(nside, (int, np.integer)):
        raise ValueError(f"nside must be an integer power of two, got {nside!r}")
    nside = int(nside)
    if nside < 1 or nside & (nside - 1) or nside > 1 << MAX_MAP_ORDER:
        raise ValueError(f"nside must be a power of two between 1 and {1 << MAX_MAP_ORDER}, got {nside}")
    return nside.bit_length() - 1


def _spread_bits(v):
    """Bits 0 .. 13 of the non-negative int64 values ``v`` moved to the even positions."""
    v = v.astype(np.uint64)
    for shift, mask in ((8, 0x00FF00FF00FF00FF), (4, 0x0F0F0F0F0F0F0F0F), (2, 0x3333333333333333), (1, 0x5555555555555555)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v.astype(np.int64)


def _loc2pix_nest(order: int, phi, z):
    """The steps of the module docstring on valid float64 arrays."""
    nside = 1 << order
    fn = float(nside)
    r = np.fmod(phi, _TWOPI)
    r = np.where(r < 0.0, r + _TWOPI, r)
    r = np.where(r >= _TWOPI, 0.0, r)
    tt = r / _HALFPI
    za = np.abs(z)
    # belt
    t1 = fn * (0.5 + tt)
    t2 = fn * z * 0.75
    jp = np.minimum(np.floor(t1 - t2).astype(np.int64), 5 * nside - 1)
    jm = np.minimum(np.floor(t1 + t2).astype(np.int64), 5 * nside - 1)
    ifp, ifm = jp >> order, jm >> order
    face_b = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))
    ix_b, iy_b = jm & (nside - 1), nside - (jp & (nside - 1)) - 1
    # caps
    ntt = np.minimum(3, tt.astype(np.int64))
    tp = tt - ntt.astype(np.float64)
    tmp = fn * np.sqrt(3.0 * (1.0 - za))
    jp = np.minimum((tp * tmp).astype(np.int64), nside - 1)
    jm = np.minimum(((1.0 - tp) * tmp).astype(np.int64), nside - 1)
    north = z > 0.0
    face_c = np.where(north, ntt, ntt + 8)
    ix_c, iy_c = np.where(north, nside - jm - 1, jp), np.where(north, nside - jp - 1, jm)
    belt = za <= _TWOTHIRD
    face, ix, iy = np.where(belt, face_b, face_c), np.where(belt, ix_b, ix_c), np.where(belt, iy_b, iy_c)
    return face * (nside * nside) + _spread_bits(ix) + 2 * _spread_bits(iy)


def _checked(order, phi, z, weights=None):
    order = int(order)
    if not 0 <= order <= MAX_MAP_ORDER:
        raise ValueError(f"order must be in 0 .. {MAX_MAP_ORDER}, got {order}")
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    if phi.ndim != 1 or phi.shape != z.shape:
        raise ValueError(f"phi and z must be one-dimensional and of equal length, got shapes {phi.shape} and {z.shape}")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != phi.shape:
            raise ValueError(f"{len(phi)} points but weights of shape {weights.shape}")
    if not np.isfinite(phi).all():
        raise ValueError("phi must be finite")
    if not (np.abs(z) <= 1.0).all():  # a NaN fails the comparison
        raise ValueError("z = sin(dec) must be finite and in [-1, 1]")
    return order, phi, z, weights


def _host_pixels(order: int, phi, z, nested: bool):
    pix = np.empty(len(phi), dtype=np.int64)
    for lo in range(0, len(phi), _HOST_STEP):
        part = _loc2pix_nest(order, phi[lo : lo + _HOST_STEP], z[lo : lo + _HOST_STEP])
        pix[lo : lo + _HOST_STEP] = part if nested else nest2ring(order, part)
    return pix


def _device(order, phi, z, weights, nested, *, want_pixels: bool, want_map: bool):
    if len(phi) < DEVICE_MAP_MIN:
        return None
    from . import engine

    return engine.healpix_map(phi, z, weights, order, nested, want_pixels=want_pixels, want_map=want_map)


def ang2pix(order: int, phi, z, *, nested: bool = True):
    """Pixel (int64[n]) of the map of ``order`` (0 .. 13, ``nside = 2^order``) that holds each point ``(phi, z)`` =
    (ra in radian, sin dec), NESTED numbers unless ``nested=False`` (RING). ``phi`` may be any finite value; ValueError
    for a non-finite value, ``|z| > 1``, arrays of different length or an order out of range."""
    order, phi, z, _ = _checked(order, phi, z)
    done = _device(order, phi, z, None, nested, want_pixels=True, want_map=False)
    if done is not None:
        return done[0]
    return _host_pixels(order, phi, z, nested)


def healpix_map(order: int, phi, z, weights=None, *, nested: bool = True):
    """Map (float64[12 * 4^order]) of the points ``(phi, z)``: objects per pixel, or with ``weights`` their sum per pixel,
    ``np.bincount(ang2pix(...), weights, minlength=npix)`` bit for bit on either route. Arguments and errors as for
    :func:`ang2pix`. The device sums a pixel's weights in one thread: a weighted map of few pixels and very many
    points is slow there (and correct)."""
    order, phi, z, weights = _checked(order, phi, z, weights)
    done = _device(order, phi, z, weights, nested, want_pixels=False, want_map=True)
    if done is not None:
        return done[1]
    npix = 12 << (2 * order)
    return np.bincount(_host_pixels(order, phi, z, nested), weights, minlength=npix).astype(np.float64, copy=False)


# ---- from a map to a catalogue's columns ----
def _checked_map(values, weights):
    """``(order, values, weights)`` of a full-sky map and its optional weight map as contiguous float64; the checks of
    ``HealPixRandoms`` without its sign rule."""
    values = np.asarray(values)
    if values.ndim != 1:
        raise ValueError("pixel values must be a one-dimensional map")
    nside = math.isqrt(len(values) // 12)
    if 12 * nside * nside != len(values) or nside < 1 or nside & (nside - 1):
        raise ValueError(f"{len(values)} pixel values are no HEALPix map: not 12 nside^2 with nside a power of two")
    order = nside.bit_length() - 1
    if order > MAX_MAP_ORDER:
        raise ValueError(f"maps above order {MAX_MAP_ORDER} (nside {1 << MAX_MAP_ORDER}) are not supported: the map alone "
                         "is more than 6 GB")
    values = np.ascontiguousarray(values, dtype=np.float64)  # (after the checks: no copy of what is no map)
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != values.shape:
            raise ValueError(f"a map of {len(values)} pixels but a weight map of shape {weights.shape}")
    return order, values, weights


def _selected(v, wt):
    """The selection rule on map values ``v`` and their weights ``wt`` (or None) -> bool mask."""
    keep = np.isfinite(v) & (v != UNSEEN)
    if wt is not None:
        keep &= np.isfinite(wt) & (wt > 0.0)
    return keep


def count_selected(values, weights=None) -> int:
    """Number of pixels :func:`map_pixels` selects (the rule does not depend on the scheme), counted in blocks."""
    total = 0
    for lo in range(0, len(values), _HOST_STEP):
        total += int(np.count_nonzero(_selected(values[lo : lo + _HOST_STEP], None if weights is None else weights[lo : lo + _HOST_STEP])))
    return total


def _host_map_pixels(order: int, values, weights, nested: bool):
    parts = []
    for lo in range(0, len(values), _HOST_STEP):  # blocks of nested pixels: no index temporary of the map's size
        q = np.arange(lo, min(lo + _HOST_STEP, len(values)), dtype=np.int64)
        src = q if nested else nest2ring(order, q)
        v = values[src]
        wt = None if weights is None else weights[src]
        keep = _selected(v, wt)
        if not keep.any():
            continue
        phi, z = pix2loc_nest(order, q[keep])
        parts.append((src[keep], phi, z, v[keep], None if wt is None else wt[keep]))
    if not parts:
        raise ValueError("every pixel is masked")
    columns = [np.concatenate(c) for c in list(zip(*parts))[:4]]
    return (*columns, None if weights is None else np.concatenate([p[4] for p in parts]))


def _map_pixels(values, weights, nested: bool, chunksize: int = 0):
    """:func:`map_pixels` and the route it took, "device" or "host"."""
    order, values, weights = _checked_map(values, weights)
    if len(values) >= DEVICE_PIXELS_MIN:
        from . import engine

        done = engine.healpix_pixels(values, weights, order, nested, chunksize=chunksize)
        if done is not None:
            return done, "device"
    return _host_map_pixels(order, values, weights, bool(nested)), "host"


def map_pixels(values, weights=None, *, nested: bool = False, chunksize: int = 0):
    """The unmasked pixels of a full-sky scalar map as columns: ``(ipix, phi, z, kappa, w)``.

    ``values`` is a float64 map of ``12 nside^2`` entries, ``nside`` a power of two up to 8192, in RING order unless
    ``nested``; ``weights`` is None or a weight / coverage map of the same length and scheme. A pixel is selected when its
    value is finite and not :data:`UNSEEN` (healpy's -1.6375e30) and, with ``weights``, its weight is finite and > 0:
    ``-0.0``, denormals and negative values are data; NaN, +-inf, ``UNSEEN`` and a weight that is 0, negative, NaN or inf
    mask a pixel. The selected pixels come in ascending NESTED number for either scheme: ``ipix`` (int64) is the pixel
    number in the map's own scheme (``values[ipix]`` is ``kappa``), ``(phi, z)`` = (ra in radian, sin dec) the pixel centre
    (``randoms.pix2loc_nest``), ``kappa`` the value and ``w`` the weight (None without ``weights``). ValueError for an input
    that is no such map, a weight map of another length, or when every pixel is masked.

    Maps of at least :data:`DEVICE_PIXELS_MIN` pixels are compacted on the GPU when there is one (``yawhip_healpix_pixels``
    in passes of ``chunksize`` nested pixels, 0: the library's default), the same values bit for bit."""
    return _map_pixels(values, weights, nested, chunksize)[0]


def map_values(order: int, phi, z, values, *, nested: bool = True):
    """The map ``values`` (``12 * 4^order`` entries, NESTED unless ``nested=False``) sampled at the points ``(phi, z)``:
    ``values[ang2pix(order, phi, z, nested=nested)]`` -- a kappa column for a galaxy sample, weights from a completeness
    map. Arguments and errors as for :func:`ang2pix`; ValueError for a map of another length."""
    values = np.asarray(values)
    if values.ndim != 1 or not 0 <= int(order) <= MAX_MAP_ORDER or len(values) != 12 << (2 * int(order)):
        raise ValueError(f"a map of order {order} has 12 * 4^order entries (order 0 .. {MAX_MAP_ORDER}), got shape {values.shape}")
    return values[ang2pix(order, phi, z, nested=nested)]
