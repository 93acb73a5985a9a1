"""Redshift distributions: the clustering-redshift estimate and the true n(z) histogram of a sample.

Mirror of ``yaw.RedshiftData`` (src/yaw/redshifts.py:195-399): n(z) = w_sp / sqrt(dz^2 * w_ss * w_pp), evaluated for the
data and every jackknife sample, and its normalisation. It is the last step of the reference's end-to-end known-answer
test (tests/test_setups.py:155-172).

Mirror of ``yaw.HistData`` (redshifts.py:44-192): the per-patch redshift histogram of a catalogue, computed on the device
(``yawhip_redshift_histogram``, csrc/yawhip_hist.hip) with the reference's bin rule, its sum over patches and its
jackknife samples. Both write and read the reference's ASCII result files (``SampledData.to_files`` / ``from_files``).
"""
from __future__ import annotations

import numpy as np

from .config import Configuration
from .corrdata import CorrData, SampledData
from .options import Closed

__all__ = ["HistData", "RedshiftData", "resample_jackknife"]


def resample_jackknife(observations):
    """Jackknife samples of per-patch values [P, B] in the reference's order (redshifts.py:60-74): sample i sums every
    patch but P - 1 - i, in increasing patch order. Row i of the index matrix holds the ids i (P - 1) .. (i + 1) (P - 1) - 1
    taken modulo P, which are exactly those patches in that order, so identical per-patch values give the reference's
    bits. With one patch the samples are zeros [1, B]."""
    observations = np.asarray(observations)
    n = observations.shape[0]
    others = (np.arange(n * (n - 1)) % n).reshape(n, n - 1)
    return observations[others].sum(axis=1)


class HistData(SampledData):
    """Redshift histogram of a catalogue with jackknife samples from its spatial patches (redshifts.py:77-192)."""

    __slots__ = ()

    @classmethod
    def from_catalog(cls, catalog, config, progress: bool = False, max_workers: int | None = None):
        """Histogram of the catalogue's redshifts in the bins of ``config`` (a ``Configuration`` or a ``BinningConfig``),
        per patch on the device: object counts, or sums of weights when the catalogue has weights. ``progress`` and
        ``max_workers`` are accepted for the reference's signature; one device computes the whole histogram."""
        if isinstance(config, Configuration):
            config = config.binning
        binning = config.binning
        if not catalog.has_redshifts:
            raise ValueError("catalog has no 'redshifts' attached")
        from . import engine

        counts = engine.redshift_histogram(catalog._z, catalog._w, catalog._patch_off, binning.edges,
                                           binning.closed == Closed.right)
        return cls(binning.copy(), counts.sum(axis=0), resample_jackknife(counts))

    @property
    def _description_data(self) -> str:
        return "n(z) histogram with symmetric 68% percentile confidence"

    @property
    def _description_samples(self) -> str:
        return f"{self.num_samples} n(z) histogram jackknife samples"

    @property
    def _description_covariance(self) -> str:
        return f"n(z) histogram covariance matrix ({self.num_bins}x{self.num_bins})"

    def normalised(self, *args, **kwargs):
        """The histogram as a probability density over the binning; arguments are ignored (redshifts.py:166-192). The
        reference first divides each bin by its width times -B / (z_max - z_min) and then by the integral, which gives
        this package the same bits; the negative factor cancels."""
        widths = self.binning.dz
        per_width = (self.binning.edges[0] - self.binning.edges[-1]) / (self.num_bins * widths)
        data, samples = self.data * per_width, self.samples * per_width
        integral = np.nansum(widths * data)
        return type(self)(self.binning, data / integral, samples / integral)


class RedshiftData(SampledData):
    __slots__ = ()

    @classmethod
    def from_corrdata(cls, cross_data: CorrData, ref_data: CorrData | None = None, unk_data: CorrData | None = None):
        def parts(corr):
            if corr is None:
                return np.float64(1.0), np.float64(1.0)
            if corr.binning != cross_data.binning or corr.num_samples != cross_data.num_samples:
                raise ValueError("correlation data are not compatible (binning or number of samples)")
            return corr.data, corr.samples

        w_ss, w_ss_samples = parts(ref_data)
        w_pp, w_pp_samples = parts(unk_data)
        dz2 = cross_data.binning.dz ** 2
        dz2_samples = np.tile(dz2, cross_data.num_samples).reshape((cross_data.num_samples, -1))
        with np.errstate(invalid="ignore", divide="ignore"):
            data = cross_data.data / np.sqrt(dz2 * w_ss * w_pp)
            samples = cross_data.samples / np.sqrt(dz2_samples * w_ss_samples * w_pp_samples)
        return cls(cross_data.binning, data, samples)

    @classmethod
    def from_corrfuncs(cls, cross_corr, ref_corr=None, unk_corr=None):
        """Sample the correlation functions (``CorrFunc.sample()``) and combine them (redshifts.py:302-330)."""
        for corr in (ref_corr, unk_corr):
            if corr is not None:
                cross_corr.is_compatible(corr, require=True)
        return cls.from_corrdata(
            cross_corr.sample(),
            None if ref_corr is None else ref_corr.sample(),
            None if unk_corr is None else unk_corr.sample(),
        )

    @property
    def _description_data(self) -> str:
        return "n(z) estimate with symmetric 68% percentile confidence"

    @property
    def _description_samples(self) -> str:
        return f"{self.num_samples} n(z) jackknife samples"

    @property
    def _description_covariance(self) -> str:
        return f"n(z) estimate covariance matrix ({self.num_bins}x{self.num_bins})"

    def normalised(self, target: SampledData | None = None):
        """Divide data and samples by one factor: the integral of the data over the binning (NaN bins left out), or, with
        ``target``, the factor that best maps the data onto ``target.data`` (redshifts.py:355-399): a one-parameter
        ``scipy.optimize.curve_fit`` of data / factor to the target over the bins where both are finite and the target is
        positive, with the target's inverse as the uncertainty of each bin, starting from 1."""
        if target is None:
            factor = np.nansum(self.binning.dz * self.data)
        else:
            from scipy.optimize import curve_fit

            used = np.isfinite(self.data) & np.isfinite(target.data) & (target.data > 0.0)
            ours, theirs = self.data[used], target.data[used]

            def model(_z, factor):
                return ours / factor

            (factor,), _ = curve_fit(model, target.binning.mids[used], theirs, p0=[1.0], sigma=1.0 / theirs)
        return type(self)(self.binning, self.data / factor, self.samples / factor)
