"""Feature matching, data parallel (after tests/test_palette_dp_gloo.py: CPU, gloo, two ranks, kernels replaced by
tests/emulator_featmatch.py): each rank takes the term's mean over its own rows, so the rank-mean of the loss dict and the all-reduced
gradient over the rank count are what one process computes at batch 2B.  No collective is added."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import featmatch_cases as P
from tests.emulator_featmatch import FeatmatchEmuOps

BG = 2


def _global_randomness(tr_like):
    torch.manual_seed(4242)
    return tr_like.sample_randomness(batch=BG)


def _config():
    return P.config(aug=True)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    bl = BG // world
    tr = P.trainer(FeatmatchEmuOps(), "cpu", _config(), batch_size=bl, world_size=world, process_group=dist.group.WORLD)
    photos, monets = P.batch("cpu", n=BG)
    rnd = tr.shard_randomness(_global_randomness(tr), rank * bl, (rank + 1) * bl)
    out[f"loss{rank}"] = tr.train_step(0, photos[rank * bl:(rank + 1) * bl], monets[rank * bl:(rank + 1) * bl], rnd)
    if rank == 0:
        out["flat_g"] = tr.opt_G.flat_g.clone()
    dist.destroy_process_group()


def test_two_ranks_equal_one_process_at_twice_the_batch():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    torch.set_num_threads(4)
    single = P.trainer(FeatmatchEmuOps(), "cpu", _config(), batch_size=BG)
    photos, monets = P.batch("cpu", n=BG)
    ref = single.train_step(0, photos, monets, _global_randomness(single))
    a, b = out["loss0"], out["loss1"]
    assert "featmatch" in ref and sorted(a) == sorted(ref)
    assert a["featmatch"] != b["featmatch"], "the ranks saw the same rows: the case shows nothing"
    for k in ref:           # the fp32 noise allowance of tests/test_palette_dp_gloo.py
        mean = 0.5 * (a[k] + b[k])
        assert abs(mean - ref[k]) <= 2e-4 * max(abs(ref[k]), 1e-3), (k, mean, ref[k])
    g = out["flat_g"] / 2
    assert float((g - single.opt_G.flat_g).abs().max() / single.opt_G.flat_g.abs().max()) < 2e-4
