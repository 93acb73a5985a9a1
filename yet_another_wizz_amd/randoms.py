"""Generators of uniform random points for random catalogues (reference src/yaw/randoms.py).

``BoxRandoms`` keeps the reference's constructor, attributes and draws: calling it with the same seed returns the
reference's values bit for bit, since both read numpy's ``PCG64`` stream in the same order. ``__call__`` is plain numpy;
:meth:`Catalog.from_random <yet_another_wizz_amd.Catalog.from_random>` draws the same values on the GPU when it can
(``engine.draw_box_randoms``, ``csrc/yawhip_random.hip``). ``HealPixRandoms`` needs healpy and is not provided.
"""
from __future__ import annotations

import numpy as np

__all__ = ["BoxRandoms"]


class BoxRandoms:
    """Random points uniform on the sphere inside a right ascension / declination window (limits in degrees), with
    optional weights and redshifts drawn with repetition from attached values (randoms.py:195-259).

    A call draws ``x = ra`` uniform in ``[x_min, x_max)`` and ``y = sin(dec)`` uniform in ``[y_min, y_max)``, then, with
    attached values, the indices of the values to copy, and returns radians."""

    def __init__(self, ra_min: float, ra_max: float, dec_min: float, dec_max: float, *, weights=None, redshifts=None,
                 seed: int = 12345) -> None:
        self.has_weights = weights is not None
        self.has_redshifts = redshifts is not None
        self.reseed(seed)
        self.weights = None if weights is None else np.asarray(weights, dtype=np.float64)
        self.redshifts = None if redshifts is None else np.asarray(redshifts, dtype=np.float64)
        self.data_size = self.get_data_size()
        self.x_min, self.y_min = self._sky2cylinder(np.deg2rad(ra_min), np.deg2rad(dec_min))
        self.x_max, self.y_max = self._sky2cylinder(np.deg2rad(ra_max), np.deg2rad(dec_max))

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
        x = self.rng.uniform(self.x_min, self.x_max, probe_size)
        y = self.rng.uniform(self.y_min, self.y_max, probe_size)
        return self._cylinder2sky(x, y)

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
