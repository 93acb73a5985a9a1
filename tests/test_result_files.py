"""ASCII result files (.dat / .smp / .cov) of CorrData, RedshiftData and HistData against the reference's own files
(tests/golden/result_files, made by tools/make_golden_nz.py), the round trip of the committed reference estimate, the
normalisations and the HistData constructor. No GPU."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from yet_another_wizz_amd import Binning, CorrData, HistData, RedshiftData
from yet_another_wizz_amd.corrdata import format_float_fixed_width
from yet_another_wizz_amd.redshifts import resample_jackknife

FILES = os.path.join(GOLDEN, "result_files")
EXAMPLE = os.path.join(GOLDEN, "reference_example", "estimate")
KINDS = {"corrdata": CorrData, "redshiftdata": RedshiftData, "histdata": HistData}


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def inputs():
    return np.load(os.path.join(FILES, "inputs.npz"))


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(FILES, "expected.npz"))


def build(kind, inputs):
    if kind == "corrdata":
        return CorrData(Binning(inputs["edges_right"], closed="right"), inputs["corr_data"], inputs["corr_samples"])
    if kind == "redshiftdata":
        return RedshiftData(Binning(inputs["edges_left"], closed="left"), inputs["nz_data"], inputs["nz_samples"])
    return HistData(Binning(inputs["edges_left"], closed="left"), inputs["hist_data"], inputs["hist_samples"])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_writers_byte_identical(kind, inputs, tmp_path):
    build(kind, inputs).to_files(tmp_path / kind)
    for ext in (".dat", ".smp", ".cov"):
        assert read_bytes(tmp_path / f"{kind}{ext}") == read_bytes(os.path.join(FILES, f"{kind}{ext}")), ext


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_from_files_matches_reference(kind, expected):
    got = KINDS[kind].from_files(os.path.join(FILES, kind))
    assert type(got) is KINDS[kind]
    assert np.array_equal(got.binning.edges, expected[f"{kind}.edges"])
    assert str(got.binning.closed) == str(expected[f"{kind}.closed"])
    assert np.array_equal(got.data, expected[f"{kind}.data"], equal_nan=True)
    assert np.array_equal(got.samples, expected[f"{kind}.samples"], equal_nan=True)


def test_to_files_replaces_an_extension_of_the_prefix(inputs, tmp_path):
    build("histdata", inputs).to_files(tmp_path / "nz.txt")
    assert sorted(os.listdir(tmp_path)) == ["nz.cov", "nz.dat", "nz.smp"]


def test_reference_estimate_round_trip(tmp_path):
    est = RedshiftData.from_files(EXAMPLE)
    assert est.num_bins == 11 and str(est.binning.closed) == "right"
    est.to_files(tmp_path / "estimate")
    assert read_bytes(tmp_path / "estimate.smp") == read_bytes(EXAMPLE + ".smp")
    # .dat / .cov: the errors are recomputed from 7-decimal samples, in the reference too; headers and z / nz survive
    for ext in (".dat", ".cov"):
        ours = read_bytes(tmp_path / f"estimate{ext}").decode().splitlines()
        ref = read_bytes(EXAMPLE + ext).decode().splitlines()
        assert len(ours) == len(ref)
        assert ours[0] == ref[0]
        if ext == ".dat":
            assert ours[1] == ref[1]
            assert [line.split()[:3] for line in ours[2:]] == [line.split()[:3] for line in ref[2:]]


def test_normalised_matches_reference(inputs, expected):
    hist = build("histdata", inputs).normalised()
    assert type(hist) is HistData
    assert np.array_equal(hist.data, expected["norm_hist.data"], equal_nan=True)
    assert np.array_equal(hist.samples, expected["norm_hist.samples"], equal_nan=True)
    nz = build("redshiftdata", inputs)
    plain = nz.normalised()
    assert type(plain) is RedshiftData
    assert np.array_equal(plain.data, expected["norm_nz.data"], equal_nan=True)
    assert np.array_equal(plain.samples, expected["norm_nz.samples"], equal_nan=True)
    fitted = nz.normalised(target=hist)
    np.testing.assert_allclose(fitted.data, expected["norm_nz_target.data"], rtol=1e-8, equal_nan=True)
    np.testing.assert_allclose(fitted.samples, expected["norm_nz_target.samples"], rtol=1e-8, equal_nan=True)


def test_histdata_normalised_is_a_density():
    binning = Binning([0.0, 0.5, 1.5, 2.0], closed="left")
    hist = HistData(binning, [2.0, 4.0, 1.0], np.ones((3, 3)))
    norm = hist.normalised("ignored", target=None)
    assert np.isclose(np.sum(binning.dz * norm.data), 1.0)


def test_format_float_fixed_width():
    assert format_float_fixed_width(0.5, 10) == " 0.5000000"
    assert format_float_fixed_width(-12345.678, 10) == "-12345.678"
    assert format_float_fixed_width(float("nan"), 10) == "       nan"
    assert format_float_fixed_width(123456789012.5, 10) == " 123456789012"


def test_histdata_constructor_and_shapes():
    binning = Binning(np.linspace(0.0, 1.0, 5))
    counts = np.arange(12.0).reshape(3, 4)
    hist = HistData(binning, counts.sum(axis=0), resample_jackknife(counts))
    assert hist.num_bins == 4 and hist.num_samples == 3
    # the reference's index arithmetic leaves out patch P - 1 - i in sample i (a permutation of the leave-one-out sums)
    for i in range(3):
        assert np.array_equal(hist.samples[i], counts.sum(axis=0) - counts[2 - i])
    with pytest.raises(ValueError):
        HistData(binning, np.zeros(3), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        HistData(binning, np.zeros(4), np.zeros((3, 5)))
    with pytest.raises(ValueError):
        HistData(binning, np.zeros(4), np.zeros(4))
    assert resample_jackknife(np.ones((1, 4))).shape == (1, 4)
    assert not np.any(resample_jackknife(np.ones((1, 4))))


def test_histdata_from_catalog_needs_redshifts():
    from yet_another_wizz_amd import Catalog, Configuration

    cat = Catalog.from_arrays(np.array([10.0, 20.0]), np.array([0.0, 5.0]), patch_ids=np.array([0, 1]))
    config = Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", zmin=0.1, zmax=1.0, num_bins=3)
    with pytest.raises(ValueError, match="redshifts"):
        HistData.from_catalog(cat, config)
