"""bench.py bookkeeping that needs no GPU: a bench line may only quote counters (profiles/pmc_traffic.json) taken on its own
workload AND its own kernel variant, and only while the kernel sources still hash to what they were taken with."""
import json
import os
import types

import numpy as np

import bench
from conftest import ROOT


def _args(**kw):
    base = dict(n_ref=10e6, n_unk=10e6, patches=64, zbins=30, scales=1, weights=False, rweight=None, kpc=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_traffic_keys_name_workload_and_kernel_variant():
    keys = {
        bench.traffic_key(_args(), "band", 32),
        bench.traffic_key(_args(weights=True), "band", 32),
        bench.traffic_key(_args(rweight=-1.0), "band", 33),
        bench.traffic_key(_args(kpc=True), "band", 32),
        bench.traffic_key(_args(), "band", 64),            # band_fp32 = 0: another kernel, other counters
        bench.traffic_key(_args(scales=3, n_ref=50e6, n_unk=50e6, patches=128), "band", 32),
        bench.traffic_key(_args(), "exact", None),
    }
    assert len(keys) == 7
    assert bench.traffic_key(_args(rweight=-1.0), "band", 33).endswith(":rw50:v33")
    assert ":kpc:" in bench.traffic_key(_args(kpc=True), "band", 32)


def test_committed_counters_are_keyed_as_bench_asks_for_them():
    """Every band entry of the committed table carries the variant suffix, its provenance and one source hash."""
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        table = json.load(f)
    entries = {k: v for k, v in table.items() if isinstance(v, dict) and (k.startswith("band:") or k.startswith("autocorr:"))}
    assert bench.traffic_key(_args(), "band", 32) in entries  # the headline
    assert bench.traffic_key(_args(weights=True), "band", 32) in entries
    assert bench.traffic_key(_args(kpc=True), "band", 32) in entries
    assert bench.traffic_key(_args(rweight=-1.0), "band", 33) in entries
    assert any(k.startswith("autocorr:RR:") for k in entries)
    hashes = set()
    for key, e in entries.items():
        assert key.rsplit(":", 1)[1] in ("v32", "v33", "v64"), key
        assert e["bytes"] > 0 and e["source"].startswith("profiles/") and os.path.exists(os.path.join(ROOT, e["source"])), key
        assert e.get("sq_active_inst_valu") and e.get("sq_insts_valu"), key
        hashes.add(e["source_sha16"])
    assert len(hashes) == 1  # one collection run of one build


def test_reference_timing_finds_the_committed_runs():
    assert bench.reference_timing(_args())["seconds"] > 5
    assert bench.reference_timing(_args(weights=True))["seconds"] > 5       # round 3 returned nothing for --weights
    assert bench.reference_timing(_args(kpc=True)) is None                  # not what the reference was timed on
    assert bench.reference_timing(_args(n_ref=3e6)) is None


def _normalised_counts(rng, num_scales, num_bins, num_patches):
    from yet_another_wizz_amd.binning import Binning
    from yet_another_wizz_amd.paircounts import NormalisedCounts, PatchedCounts, PatchedSumWeights

    binning = Binning(np.linspace(0.1, 1.0, num_bins + 1))
    sw = PatchedSumWeights(binning, rng.uniform(1, 2, (num_bins, num_patches)), rng.uniform(1, 2, (num_bins, num_patches)),
                           auto=False)
    return [NormalisedCounts(PatchedCounts(binning, rng.integers(0, 99, (num_bins, num_patches, num_patches)).astype(float),
                                           auto=False), sw) for _ in range(num_scales)]


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    """--dump-outputs: every array a caller of count_pairs receives, float64, one file each."""
    rng = np.random.default_rng(5)
    dd, dr = _normalised_counts(rng, 2, 3, 4), _normalised_counts(rng, 2, 3, 4)
    bench.dump_outputs(str(tmp_path), {"DD": dd, "DR": dr})
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted(f"{c}_{k}.npy" for c in ("DD", "DR") for k in ("s0_counts", "s1_counts", "sum_weights1", "sum_weights2"))
    for c, res in (("DD", dd), ("DR", dr)):
        for s in range(2):
            got = np.load(tmp_path / f"{c}_s{s}_counts.npy")
            assert got.dtype == np.float64 and np.array_equal(got, res[s].counts.counts)
        assert np.array_equal(np.load(tmp_path / f"{c}_sum_weights1.npy"), res[0].sum_weights.sum_weights1)
        assert np.array_equal(np.load(tmp_path / f"{c}_sum_weights2.npy"), res[0].sum_weights.sum_weights2)


def test_dump_outputs_samples_large_results_within_the_limit(tmp_path, monkeypatch):
    """Beyond the size limit every array keeps the same seeded sample of its elements, so runs stay comparable."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    res = _normalised_counts(np.random.default_rng(6), 3, 30, 40)  # 3 x 288 kB of counts
    for out in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(out), {"DD": res})
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 200_000
    full = res[0].counts.counts.reshape(-1)
    got = np.load(tmp_path / "a" / "DD_s0_counts.npy")
    assert got.dtype == np.float64 and 0 < got.size < full.size and np.isin(got, full).all()
    for p in (tmp_path / "a").iterdir():
        assert np.array_equal(np.load(p), np.load(tmp_path / "b" / p.name)), p.name
