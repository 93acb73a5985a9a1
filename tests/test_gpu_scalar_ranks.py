"""GPU: a κ-weighted count under several ranks. Two ranks (gloo group, both on GPU 0, fresh child processes) shard the jobs
of ``count_pairs(mode="kk")`` over the golden 8-patch catalogue, count their share on their own twin catalogue and
all-reduce; every rank must hold the tensor a single process counts."""
import os
import socket
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
RANK_TIMEOUT = 240  # seconds for the whole group: import, two uploads and four small counts per rank


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _measure():
    import test_gpu_scalar as cases
    import yet_another_wizz_amd as yaw
    from conftest import load_golden

    g = load_golden("scalar_drivers.npz")
    cats = cases._driver_catalogs(g, weights=True)
    config = cases._driver_config(g)
    ref = cats["ref"]
    ref.build_trees(config.binning.edges, closed="right")
    links = yaw.PatchLinkage.from_catalogs(config, ref)
    kk = np.stack([c.counts.counts for c in links.count_pairs(ref, mode="kk")])
    scalar = links.count_scalar_pairs(ref, mode="kk", count_type_info="DD")  # several ranks: one count after the other
    assert all(np.array_equal(s.kappa_counts.counts, k) for s, k in zip(scalar, kk))
    ref.drop_layouts()
    return g, kk, np.stack([s.number_counts.counts for s in scalar])


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), YAW_AMD_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _, kk, nn = _measure()
        np.save(os.path.join(out_dir, f"kk{rank}.npy"), kk)
        np.save(os.path.join(out_dir, f"nn{rank}.npy"), nn)
    finally:
        dist.destroy_process_group()


def test_two_ranks_count_kk(tmp_path):
    import torch.multiprocessing as mp

    import test_gpu_scalar as cases

    g, single_kk, single_nn = _measure()  # this process: no group, the dense path
    for s in range(2):
        cases.check_kappa_slots(f"auto.s{s}.dd", single_kk[s], g[f"auto.s{s}.dd.kappa_counts"], g[f"auto.s{s}.dd.abs_counts"])
    world = 2
    group = mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=False, start_method="spawn")
    deadline = time.monotonic() + RANK_TIMEOUT
    try:
        while not group.join(timeout=5):  # raises if a rank failed
            if time.monotonic() > deadline:
                pytest.fail(f"the ranks did not finish within {RANK_TIMEOUT} s")
    finally:
        for proc in group.processes:
            if proc.is_alive():
                proc.kill()
    for rank in range(world):
        # every scale sums at most two fine bins per slot and halves the diagonal: the host epilogue of the ranks path and the
        # device epilogue of the single process do the same arithmetic on the same per-job sums
        assert np.array_equal(np.load(tmp_path / f"kk{rank}.npy"), single_kk), rank
        assert np.array_equal(np.load(tmp_path / f"nn{rank}.npy"), single_nn), rank
