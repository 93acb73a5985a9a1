"""Generators of random points for random catalogues (reference src/yaw/randoms.py).

``BoxRandoms`` keeps the reference's constructor, attributes and draws: calling it with the same seed returns the
reference's values bit for bit, since both read numpy's ``PCG64`` stream in the same order. ``HealPixRandoms`` keeps the
reference's constructor and what it draws -- centres of order-29 nested pixels inside the unmasked pixels of a HEALPix
map -- without healpy, on a stream of its own (see its docstring). ``__call__`` is plain numpy;
:meth:`Catalog.from_random <yet_another_wizz_amd.Catalog.from_random>` draws the same values on the GPU when it can
(``engine.draw_box_randoms`` / ``engine.draw_healpix_randoms``, ``csrc/yawhip_random.hip``).
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ["BoxRandoms", "HealPixRandoms"]


class RandomsBase:
    """What the generators share (the reference's ``RandomsBase``, randoms.py:37-184): the seeded stream, the attached
    values and their draw, ``__call__`` and ``generate_dataframe``. A subclass gives ``_draw_coords(probe_size)`` ->
    ``(ra, dec)`` in radian."""

    def __init__(self, *, weights=None, redshifts=None, seed: int = 12345) -> None:
        self.has_weights = weights is not None
        self.has_redshifts = redshifts is not None
        self.reseed(seed)
        self.weights = None if weights is None else np.asarray(weights, dtype=np.float64)
        self.redshifts = None if redshifts is None else np.asarray(redshifts, dtype=np.float64)
        self.data_size = self.get_data_size()

    def __repr__(self) -> str:
        return f"{type(self).__name__}(has_weights={self.has_weights}, has_redshifts={self.has_redshifts})"

    def get_data_size(self) -> int:
        """Number of attached values to draw from, -1 if none; raises ValueError if weights and redshifts differ in
        length (randoms.py:58-82)."""
        if self.weights is None and self.redshifts is None:
            return -1
        if self.weights is None:
            return len(self.redshifts)
        if self.redshifts is None:
            return len(self.weights)
        if len(self.weights) != len(self.redshifts):
            raise ValueError("number of 'weights' and 'redshifts' to draw from does not match")
        return len(self.weights)

    def reseed(self, seed: int | None = None) -> None:
        """Restart the stream, from ``seed`` if given (randoms.py:84-93: one spawned child of ``SeedSequence(seed)``)."""
        if seed is not None:
            self.seed = int(seed)
        self.rng = np.random.default_rng(np.random.SeedSequence(self.seed).spawn(1)[0])

    @staticmethod
    def _sky2cylinder(ra, dec):
        return ra, np.sin(dec)

    @staticmethod
    def _cylinder2sky(x, y):
        return x, np.arcsin(y)

    def _draw_coords(self, probe_size: int):
        raise NotImplementedError

    def _draw_attributes(self, probe_size: int) -> dict:
        if self.data_size == -1:
            return {}
        idx = self.rng.integers(0, self.data_size, size=probe_size)
        data = {}
        if self.has_weights:
            data["weights"] = self.weights[idx]
        if self.has_redshifts:
            data["redshifts"] = self.redshifts[idx]
        return data

    def __call__(self, probe_size: int) -> dict:
        """Draw ``probe_size`` points: a dict of float64 arrays ``ra``, ``dec`` (radian) and, with attached values,
        ``weights`` / ``redshifts``."""
        ra, dec = self._draw_coords(probe_size)
        return dict(ra=ra, dec=dec, **self._draw_attributes(probe_size))

    def generate_dataframe(self, probe_size: int, *, degrees: bool = True):
        """Draw ``probe_size`` points into a pandas DataFrame, coordinates in degrees unless ``degrees=False``."""
        try:
            import pandas as pd
        except ImportError as err:
            raise ImportError("optional dependency 'pandas' required to generate DataFrames") from err
        df = pd.DataFrame(self(probe_size))
        if degrees:
            df["ra"] = np.rad2deg(df["ra"])
            df["dec"] = np.rad2deg(df["dec"])
        return df


class BoxRandoms(RandomsBase):
    """Random points uniform on the sphere inside a right ascension / declination window (limits in degrees), with
    optional weights and redshifts drawn with repetition from attached values (randoms.py:195-259).

    A call draws ``x = ra`` uniform in ``[x_min, x_max)`` and ``y = sin(dec)`` uniform in ``[y_min, y_max)``, then, with
    attached values, the indices of the values to copy, and returns radians."""

    def __init__(self, ra_min: float, ra_max: float, dec_min: float, dec_max: float, *, weights=None, redshifts=None,
                 seed: int = 12345) -> None:
        super().__init__(weights=weights, redshifts=redshifts, seed=seed)
        self.x_min, self.y_min = self._sky2cylinder(np.deg2rad(ra_min), np.deg2rad(dec_min))
        self.x_max, self.y_max = self._sky2cylinder(np.deg2rad(ra_max), np.deg2rad(dec_max))

    def _draw_coords(self, probe_size: int):
        x = self.rng.uniform(self.x_min, self.x_max, probe_size)
        y = self.rng.uniform(self.y_min, self.y_max, probe_size)
        return self._cylinder2sky(x, y)


# ---- HEALPix in integers and a few float64 operations (Gorski et al. 2005; the pix2loc arithmetic of HEALPix' C++) ----
MAX_ORDER = 29  # the order whose pixel centres are drawn (randoms.py:344)
MAX_MAP_ORDER = 13  # a float64 map of order 14 is 25 GB, its list of unmasked pixels and cdf as much again
_JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], dtype=np.int64)  # ring of a face's north corner, in nside
_JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7], dtype=np.int64)  # longitude of a face's centre, in pi / 4
_HALFPI = np.pi / 2


def _even_bits(v):
    """Bits 0, 2, 4, ... of the uint64 values ``v``, packed into the low half (shift / mask steps, as the kernel)."""
    for shift, mask in ((0, 0x5555555555555555), (1, 0x3333333333333333), (2, 0x0F0F0F0F0F0F0F0F), (4, 0x00FF00FF00FF00FF),
                        (8, 0x0000FFFF0000FFFF), (16, 0x00000000FFFFFFFF)):
        v = (v | (v >> np.uint64(shift))) & np.uint64(mask)
    return v.astype(np.int64)


def _ring_position(order: int, ipix):
    """Where the nested pixels ``ipix`` of ``order`` lie in the ring scheme: ring ``jr`` (1 .. 4 nside - 1 from the north),
    ``nr`` (the ring's pixels per quadrant: jr, nside, or 4 nside - jr), ``kshift`` (1 on belt rings that start at phi = 0),
    position ``jp`` in the ring (1 .. 4 nr) and the cap masks ``north`` / ``south``. All integer."""
    ipix = np.asarray(ipix, dtype=np.int64)
    nside = 1 << order
    face = ipix >> (2 * order)
    low = (ipix & ((1 << (2 * order)) - 1)).astype(np.uint64)
    ix, iy = _even_bits(low), _even_bits(low >> np.uint64(1))
    jr = (_JRLL[face] << order) - ix - iy - 1
    north, south = jr < nside, jr > 3 * nside
    nr = np.where(north, jr, np.where(south, 4 * nside - jr, nside))
    kshift = np.where(north | south, 0, (jr - nside) & 1)
    jp = (_JPLL[face] * nr + ix - iy + 1 + kshift) >> 1  # the sum is even
    jp = np.where(jp > 4 * nside, jp - 4 * nside, jp)
    jp = np.where(jp < 1, jp + 4 * nside, jp)
    return jr, nr, kshift, jp, north, south


def nest2ring(order: int, ipix):
    """Ring-scheme numbers of the nested pixels ``ipix`` of ``order`` (int64)."""
    nside = 1 << order
    jr, nr, _, jp, north, south = _ring_position(order, ipix)
    ncap, npix = 2 * nside * (nside - 1), 12 * nside * nside
    return np.where(north, 2 * jr * (jr - 1) + jp - 1,
                    np.where(south, npix - 2 * nr * (nr + 1) + jp - 1, ncap + (jr - nside) * (4 * nside) + jp - 1))


def pix2loc_nest(order: int, ipix):
    """Centres of the nested pixels ``ipix`` of ``order``: ``(phi, z)`` with ``z = cos(theta) = sin(dec)``, float64. Every float
    step is one IEEE operation in the written order (no FMA, no transcendental): the device repeats them bit for bit."""
    nside = 1 << order
    jr, nr, kshift, jp, north, south = _ring_position(order, ipix)
    fact2 = 4.0 / float(12 * nside * nside)
    fact1 = float(2 * nside) * fact2
    nrf = nr.astype(np.float64)
    tmp = nrf * nrf * fact2
    z = np.where(north, 1.0 - tmp, np.where(south, tmp - 1.0, (2 * nside - jr).astype(np.float64) * fact1))
    phi = (jp.astype(np.float64) - (kshift + 1).astype(np.float64) * 0.5) * (_HALFPI / nrf)
    return phi, z


class HealPixRandoms(RandomsBase):
    """Random points inside a HEALPix mask or probability map (randoms.py:262-363), with optional weights and redshifts
    drawn with repetition from attached values. No healpy: the pixel arithmetic is :func:`pix2loc_nest` / :func:`nest2ring`.

    ``pix_values`` is a full-sky map of ``12 nside^2`` non-negative values, ``nside`` a power of two up to 2^13 (a map of
    order 14 is more than 6 GB), in RING order unless ``nested``. Pixels with value 0 are masked; the others are drawn
    with probability proportional to their value, or all alike with ``is_mask``. As in the reference, a point is not
    continuous inside its pixel: it is the centre of one of the order-29 nested pixels inside the drawn map pixel
    (0.4 mas apart), returned as ``ra = phi`` and ``dec = arcsin(z)``. Within about 3 mas of a pole ``1 - nr^2 fact2``
    rounds ``z`` to +-1, the resolution ``BoxRandoms`` has in ``sin(dec)`` too.

    **The stream is this package's own.** The reference picks the map pixel with ``np.random.choice`` on numpy's global
    RNG, so its output does not depend on ``seed`` and there is no reference stream to reproduce. Here every draw comes
    from the generator's ``PCG64`` and is fixed by ``seed``. One call of ``k`` points reads, in this order:

    1. ``k`` raw 64-bit outputs: ``u = (out >> 11) * 2^-53``, slot ``j = searchsorted(cdf, u, side="right")`` in the float64
       cumulative probabilities of the unmasked pixels (``p.cumsum() / p.cumsum()[-1]``, numpy's ``Generator.choice``
       recipe; ``p`` all ones with ``is_mask``), ``ipix = _ipix_unmasked[j]``;
    2. ``k`` raw 64-bit outputs: ``sub = out >> (64 - 2 (29 - order))``, uniform in ``[0, 4^(29 - order))`` without rejection,
       ``ipix29 = ipix * 4^(29 - order) + sub``;
    3. with attached values, ``k`` indices ``rng.integers(0, data_size)`` as ``BoxRandoms``.

    The plain-numpy draw here is the oracle of the device route (``yawhip_random_healpix``)."""

    def __init__(self, pix_values, *, nested: bool = False, is_mask: bool = False, weights=None, redshifts=None,
                 seed: int = 12345) -> None:
        super().__init__(weights=weights, redshifts=redshifts, seed=seed)
        values = np.asarray(pix_values, dtype=np.float64)
        if values.ndim != 1:
            raise ValueError("pixel values must be a one-dimensional map")
        nside = math.isqrt(len(values) // 12)
        if 12 * nside * nside != len(values) or nside < 1 or nside & (nside - 1):
            raise ValueError(f"{len(values)} pixel values are no HEALPix map: not 12 nside^2 with nside a power of two")
        self.nside = nside
        self.order = nside.bit_length() - 1
        if self.order > MAX_MAP_ORDER:
            raise ValueError(f"maps above order {MAX_MAP_ORDER} (nside {1 << MAX_MAP_ORDER}) are not supported: the map alone "
                             "is more than 6 GB")
        if not np.all(values >= 0.0) or not np.isfinite(values.sum()):
            raise ValueError("pixel values must be positive and finite for random generation")
        if not nested:
            values = self._ring2nest(values)
        self._ipix_unmasked = np.nonzero(values)[0]
        if len(self._ipix_unmasked) == 0:
            raise ValueError("every pixel is masked")
        cdf = np.ones(len(self._ipix_unmasked)) if is_mask else values[self._ipix_unmasked]
        np.cumsum(cdf, out=cdf)
        cdf /= cdf[-1]
        self._cdf = cdf

    @classmethod
    def from_catalog(cls, catalog, nside: int, *, is_mask: bool = True, weights=None, redshifts=None, seed: int = 12345):
        """Generator over the footprint of ``catalog``: its nested map at ``nside`` (``Catalog.healpix_map``: summed weights,
        or counts for a catalogue without weights) as ``pix_values``. With ``is_mask`` (the default) every occupied pixel is
        drawn alike, otherwise in proportion to its value. ``weights`` / ``redshifts`` are the values to attach, as in the
        constructor."""
        return cls(catalog.healpix_map(nside, nested=True), nested=True, is_mask=is_mask, weights=weights, redshifts=redshifts,
                   seed=seed)

    def _ring2nest(self, values):
        nested = np.empty_like(values)
        step = 1 << 22  # pixels reordered at a time: bounds the index temporaries of a large map
        for lo in range(0, len(values), step):
            ipix = np.arange(lo, min(lo + step, len(values)), dtype=np.int64)
            nested[lo : lo + step] = values[nest2ring(self.order, ipix)]
        return nested

    def _draw_pixels(self, probe_size: int):
        """The order-29 nested pixels of ``probe_size`` points (int64): steps 1 and 2 of the stream. ``random_raw`` leaves a
        pending 32-bit half of the generator alone."""
        raw = self.rng.bit_generator.random_raw(probe_size)
        u = (raw >> np.uint64(11)).astype(np.float64) * 2.0**-53
        ipix = self._ipix_unmasked[np.searchsorted(self._cdf, u, side="right")]
        shift = 2 * (MAX_ORDER - self.order)
        sub = self.rng.bit_generator.random_raw(probe_size) >> np.uint64(64 - shift)
        return (ipix << shift) + sub.astype(np.int64)

    def _draw_coords(self, probe_size: int):
        return self._cylinder2sky(*pix2loc_nest(MAX_ORDER, self._draw_pixels(probe_size)))
