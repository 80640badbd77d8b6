"""Data-parallel launching for the two training drivers (train_cutpp, train_basic): `--gpus N` on one node.

    python -m gan_variant_research_amd.train_cutpp --config CFG --gpus 8
    python -m torch.distributed.run --nproc-per-node 8 -m gan_variant_research_amd.train_cutpp --config CFG

Without `WORLD_SIZE` in the environment `--gpus N` (N > 1) makes the process a launcher (`launch_ranks`): it starts N fresh processes
of the same command, one per GPU, with the environment torch.distributed.run would give them (RANK / LOCAL_RANK / WORLD_SIZE /
LOCAL_WORLD_SIZE / MASTER_ADDR / MASTER_PORT), relays rank 0's standard output, and brings every rank down when one fails.  The
launcher makes no GPU call, and nothing that has initialised the GPU is ever exec'ed.  With `WORLD_SIZE` present the process is a
rank (`join`): it takes `cuda:LOCAL_RANK`, creates and uses its compute streams once (HipOps.bind_queues), then creates
the process group (`nccl` on a GPU device, `gloo` on a CPU device -- the tests' hook) and destroys it on the way out.
"""
from __future__ import annotations

import contextlib
import os
import socket
import subprocess
import sys
import threading
import time
from typing import List, Optional, Sequence

import torch

MAX_RANKS = 8                                   # one node: eight GPUs
FAIL_RANK_ENV = "TRAIN_LAUNCH_CHECK_FAIL_RANK"  # test hook, read by --launch-check only: that rank exits with code 3


def add_arguments(parser) -> None:
    parser.add_argument("--gpus", type=int, default=1, help="data-parallel ranks, one per GPU; the batch size of the config is per GPU (build-only flag)")
    parser.add_argument("--launch-check", action="store_true",
                        help="no GPU work: every rank joins a gloo group on the host, rank 0 prints the rank count (tests the --gpus N launcher)")


def visible_gpus() -> int:
    """torch.cuda.device_count() asked of a short-lived child, so that this process opens no GPU."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"[launch] could not count the GPUs: {r.stderr.strip()[-500:]}")
    return int(r.stdout.strip().splitlines()[-1])


def check_rank_count(n: int, check_devices: bool = True) -> None:
    if n < 1:
        raise SystemExit(f"--gpus {n}: at least one rank")
    if n > MAX_RANKS:
        raise SystemExit(f"--gpus {n}: at most {MAX_RANKS} ranks (one node) are started")
    if check_devices:
        have = visible_gpus()
        if n > have:
            raise SystemExit(f"--gpus {n} but this machine shows {have} GPU(s); no rank was started")


def _package_root() -> str:
    """The directory `import gan_variant_research_amd` resolves from: the children get it in front of PYTHONPATH."""
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _die_with_launcher():
    """Runs in a child between fork and exec (Linux): the rank gets SIGTERM when the launcher dies, however that happens."""
    import ctypes
    import signal
    ctypes.CDLL(None).prctl(1, signal.SIGTERM)          # PR_SET_PDEATHSIG


def launch_ranks(command: Sequence[str], argv: Sequence[str], n: int, check_devices: bool = True) -> None:
    """Starts `python command... argv...` n times (the drivers: command = ["-m", their module]), one rank per GPU; returns when all
    have exited with 0, raises SystemExit naming the first rank that did not (the others are terminated, and killed after 20 s)."""
    check_rank_count(n, check_devices)
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    path = os.pathsep.join(p for p in (_package_root(), os.environ.get("PYTHONPATH")) if p)
    procs: List[subprocess.Popen] = []
    reader = None
    tied = {"preexec_fn": _die_with_launcher} if sys.platform.startswith("linux") else {}
    old_term = None
    if threading.current_thread() is threading.main_thread():       # a terminated launcher stops its ranks like an interrupted one
        import signal
        old_term = signal.signal(signal.SIGTERM, lambda *_: sys.exit(143))
    try:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), PYTHONPATH=path)
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: RCCL's peer mappings need it on this driver
            procs.append(subprocess.Popen([sys.executable, *command, *argv], env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0), **tied))

        def relay():
            for ln in procs[0].stdout:
                sys.stdout.write(ln)
                sys.stdout.flush()
        reader = threading.Thread(target=relay, daemon=True)
        reader.start()
        failed = None
        while failed is None and any(p.poll() is None for p in procs):
            time.sleep(0.2)
            failed = next((p for p in procs if p.poll() not in (None, 0)), None)
        failed = failed or next((p for p in procs if p.returncode != 0), None)
    except BaseException:           # the launcher itself is interrupted: nothing it started stays behind
        _stop(procs)
        raise
    finally:
        if old_term is not None:
            signal.signal(signal.SIGTERM, old_term)
    if failed is not None:          # one rank died: the others would wait in a collective, stop exactly the processes started here
        _stop(procs)
    if reader is not None:
        reader.join(timeout=10)
    if failed is not None:
        raise SystemExit(f"[launch] rank {procs.index(failed)} exited with code {failed.returncode}; the other ranks were stopped")


def _stop(procs) -> None:
    for p in procs:
        if p.poll() is None:
            p.terminate()
    deadline = time.monotonic() + 20
    for p in procs:
        try:
            p.wait(timeout=max(0.0, deadline - time.monotonic()))
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


class Rank:
    """What a driver needs to know about its place: `group` is None in the plain single-process run."""

    def __init__(self, rank=0, world=1, local=0, group=None, device=None, ops=None):
        self.rank, self.world, self.local, self.group, self.device, self.ops = rank, world, local, group, device, ops

    @property
    def first(self) -> bool:
        return self.rank == 0

    def rows(self, batch: int) -> slice:
        """This rank's rows of a global batch of world * batch."""
        return slice(self.rank * batch, (self.rank + 1) * batch)


def world_from_env(gpus: int) -> Optional[int]:
    """WORLD_SIZE when the environment names one (a launcher started this process), else None.  `--gpus` is then its default or equal."""
    if "WORLD_SIZE" not in os.environ:
        return None
    world = int(os.environ["WORLD_SIZE"])
    if gpus > 1 and world != gpus:
        raise SystemExit(f"--gpus {gpus} but the launcher started {world} ranks (WORLD_SIZE={world})")
    return world


@contextlib.contextmanager
def _stdout_on_stderr():
    """RCCL and gloo print a banner on STDOUT when a communicator is created: file descriptor 1 points at stderr until it exists, so
    that rank 0's relayed output stays the driver's own."""
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def launch_check() -> None:
    """--launch-check: a gloo group on the host, no GPU work; rank 0 prints the rank count."""
    import json
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if os.environ.get(FAIL_RANK_ENV) == str(rank):
        sys.exit(3)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    with _stdout_on_stderr():
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank)])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    try:
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "max_rank": int(t.item())}), flush=True)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@contextlib.contextmanager
def join(world: Optional[int], device: Optional[str], ops=None):
    """The rank's context.  world None: the plain run -- no group, `device` as given (None: "cuda"), `ops` as given.  Otherwise the
    rank of the environment on cuda:LOCAL_RANK (or the CPU device of the tests) inside a process group, which is destroyed on the
    way out, also when an exception propagates."""
    if world is None:
        yield Rank(device=torch.device(device if device is not None else "cuda"), ops=ops)
        return
    import torch.distributed as dist
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type == "cuda":
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        if ops is None:
            from .runtime import HipOps
            ops = HipOps(dev)
        if hasattr(ops, "bind_queues"):
            ops.bind_queues()               # the compute streams exist and have run once BEFORE RCCL creates its own
        with _stdout_on_stderr():
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)     # RCCL over xGMI
            warm = torch.zeros(1, device=dev)
            dist.all_reduce(warm)                                                          # creates the communicator
            torch.cuda.synchronize(dev)
    else:
        with _stdout_on_stderr():
            dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        yield Rank(rank, world, local, dist.group.WORLD, dev, ops)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def state_digest(optimisers) -> str:
    """sha256 over flat_p, flat_m, flat_v of every optimiser, in order: equal on all ranks after any number of steps."""
    import hashlib
    h = hashlib.sha256()
    for opt in optimisers:
        for t in (opt.flat_p, opt.flat_m, opt.flat_v):
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()
