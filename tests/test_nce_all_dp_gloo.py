"""PatchNCE with negatives from the whole minibatch, data parallel (after tests/test_palette_dp_gloo.py: CPU, gloo, two ranks, kernels replaced
by tests/emulator_nce_all.py): two ranks at batch 1 each exchange the normalised source rows of all layers in ONE collective per step, score
their own rows against both ranks' keys, and their rank-mean loss and summed gradient / 2 are those of one process at batch 2."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import cut_nce_all_cases as K
from tests.emulator_nce_all import NceAllEmuOps

BG = 2


def _global_randomness(tr_like):
    torch.manual_seed(4242)
    return tr_like.sample_randomness(batch=BG)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    bl = BG // world
    tr = K.trainer(NceAllEmuOps(), "cpu", K.config(True), bl, world_size=world, process_group=dist.group.WORLD)
    photos, monets = K.batch("cpu", BG)
    rnd = tr.shard_randomness(_global_randomness(tr), rank * bl, (rank + 1) * bl)
    out[f"loss{rank}"] = tr.train_step(0, photos[rank * bl:(rank + 1) * bl], monets[rank * bl:(rank + 1) * bl], rnd)
    out[f"exchanges{rank}"] = tr.nce_exchanges
    if rank == 0:
        out["flat_g"] = tr.opt_G.flat_g.clone()
    dist.destroy_process_group()


def test_two_ranks_are_one_process_at_twice_the_batch():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    torch.set_num_threads(4)
    single = K.trainer(NceAllEmuOps(), "cpu", K.config(True), BG)
    photos, monets = K.batch("cpu", BG)
    ref = single.train_step(0, photos, monets, _global_randomness(single))
    assert out["exchanges0"] == out["exchanges1"] == 1 and single.nce_exchanges == 0
    np.testing.assert_allclose(0.5 * (out["loss0"]["nce"] + out["loss1"]["nce"]), ref["nce"], rtol=2e-4)
    g = out["flat_g"] / 2
    assert float((g - single.opt_G.flat_g).abs().max() / single.opt_G.flat_g.abs().max()) < 2e-4
    # the whole-minibatch term is what ties the ranks: with per-image negatives the same comparison holds with no exchange at all, so the
    # step must differ from it
    assert abs(ref["nce"] - K.nce_of(NceAllEmuOps, "cpu", False, False)) > 0.1
