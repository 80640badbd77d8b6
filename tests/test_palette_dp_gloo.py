"""Palette prior, data parallel (after tests/test_dp_gloo.py: CPU, gloo, two ranks, kernels replaced by tests/emulator_palette.py): the six
batch means of the Monet statistics are all-reduced between the two small launches, so both ranks hold the same prior after a step, and it
is the prior one process computes at batch 2B; the rank-mean of the palette loss is the one-process loss."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import palette_cases as P
from tests.emulator_palette import PaletteEmuOps

BG = 2


def _global_randomness(tr_like):
    torch.manual_seed(4242)
    return tr_like.sample_randomness()


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    bl = BG // world
    tr = P.trainer(PaletteEmuOps(), "cpu", P.config(), batch_size=bl, world_size=world, process_group=dist.group.WORLD)
    photos, monets = P.batch("cpu", n=BG)
    rnd = tr.shard_randomness(_global_randomness(tr), rank * bl, (rank + 1) * bl)
    losses = tr.train_step(0, photos[rank * bl:(rank + 1) * bl], monets[rank * bl:(rank + 1) * bl], rnd)
    out[f"prior{rank}"], out[f"steps{rank}"], out[f"loss{rank}"] = tr.pal_prior.clone(), int(tr.pal_steps), losses
    if rank == 0:
        out["flat_g"] = tr.opt_G.flat_g.clone()
    dist.destroy_process_group()


def test_two_ranks_hold_the_one_process_prior():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    torch.set_num_threads(4)
    single = P.trainer(PaletteEmuOps(), "cpu", P.config(), batch_size=BG)
    photos, monets = P.batch("cpu", n=BG)
    ref = single.train_step(0, photos, monets, _global_randomness(single))
    assert out["steps0"] == out["steps1"] == 1
    assert torch.equal(out["prior0"], out["prior1"]), "the ranks hold different priors"
    want = single.pal_prior[:6]
    assert float(want.abs().min()) > 0
    np.testing.assert_allclose(out["prior0"][:6].numpy(), want.numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(0.5 * (out["loss0"]["palette"] + out["loss1"]["palette"]), ref["palette"], rtol=2e-4)
    g = out["flat_g"] / 2
    assert float((g - single.opt_G.flat_g).abs().max() / single.opt_G.flat_g.abs().max()) < 2e-4
