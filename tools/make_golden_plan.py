"""Records what both fused trainers plan and compute BEFORE the planner's bf16 and e4m3 paths were merged, for
tests/test_plan_parent_launches.py and tests/test_plan_parent_gpu.py.

Both records were made on the commit before the merge (this file copied into its tree) and are never recomputed from the code under
test:

  python tools/make_golden_plan.py launches           -> tests/golden/plan_parent_launches.json
      LaunchLog.hashed() of every launch the trainers plan (tests.emulator_fp8wgrad.RecOps; nothing is stepped), for the RECORDS below
      (stored without repetition, see pack / unpack):
      the CUT trainer (both identity modes) on Fp8WgradEmuOps, the CycleGAN trainer on BasicFp8EmuOps.  Together they reach every arm of
      the residual blocks' backward: chain or no chain, e4m3 weight gradient taken / refused (maps under 128 pixels) / grouped (several
      whole images per split, batch 64), both taggings of the e4m3 gradient buffer sets;
  python tools/make_golden_plan.py gpu [--out FILE]   -> tests/golden/plan_parent_gpu.json
      on the MI355X: one iteration of each trainer at 64x64, batch 2, with fp8 + fp8_wgrad -- the losses as float.hex() and the SHA-256
      of every optimiser's parameter block.  Each iteration is run twice from fresh trainers and must give the same bits before anything
      is written.
"""
from __future__ import annotations

import base64
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import emulator_basic_fp8 as EB  # noqa: E402
from tests import emulator_fp8wgrad as EC  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# name -> (trainer, image size, batch, fp8, fp8_wgrad)
RECORDS = {
    "cut_64_b2_bf16": ("cut", 64, 2, False, False),
    "cut_64_b2_fp8": ("cut", 64, 2, True, False),
    "cut_64_b2_fp8_wgrad": ("cut", 64, 2, True, True),
    "cut_32_b2_fp8_wgrad": ("cut", 32, 2, True, True),
    "basic_64_b2_bf16": ("basic", 64, 2, False, False),
    "basic_64_b2_fp8": ("basic", 64, 2, True, False),
    "basic_64_b2_fp8_wgrad": ("basic", 64, 2, True, True),
    "basic_64_b64_fp8_wgrad": ("basic", 64, 64, True, True),
}
GPU_S, GPU_B = 64, 2


def plan(name):
    """The trainer of RECORDS[name] built on a recording op layer -> its LaunchLog."""
    which, S, B, fp8, fp8_wgrad = RECORDS[name]
    if which == "cut":
        return EC.build_step_programs(EC.Fp8WgradEmuOps(), S, B, fp8, fp8_wgrad)[1]
    return EB.build_programs(EB.BasicFp8EmuOps(), S, B, True, fp8, fp8_wgrad)[1]


def pack(rec):
    """{record: LaunchLog.hashed()} in the compact, lossless form of the golden file (the records share most of their launches):
    "ops" = the distinct "stream name" strings; "op" / "digest" = every distinct [stream, name, digest] in order of first appearance, as an
    index into "ops" and as base64 of the digests' bytes (6 each); "records" = each record's sequence as runs of consecutive entries,
    flat: first, count, first, count, ..."""
    ops, table, runs = [], {}, {}
    for name, seq in rec.items():
        r = runs[name] = []
        for s, n, d in seq:
            if s + " " + n not in ops:
                ops.append(s + " " + n)
            i = table.setdefault((ops.index(s + " " + n), d), len(table))
            if r and r[-2] + r[-1] == i:
                r[-1] += 1
            else:
                r += [i, 1]
    digest = base64.b64encode(bytes.fromhex("".join(d for _, d in table))).decode()
    return {"ops": ops, "op": [o for o, _ in table], "digest": digest, "records": runs}


def unpack(blob):
    """Inverse of pack: {record: [[stream, name, digest], ...]}."""
    hexd = base64.b64decode(blob["digest"]).hex()
    entry = [blob["ops"][o].split(" ") + [hexd[12 * i:12 * i + 12]] for i, o in enumerate(blob["op"])]
    return {name: [entry[i] for first, count in zip(r[::2], r[1::2]) for i in range(first, first + count)] for name, r in blob["records"].items()}


def launches(out):
    rec = {name: plan(name).hashed() for name in RECORDS}
    assert unpack(pack(rec)) == rec
    with open(out, "w") as f:
        json.dump(pack(rec), f, separators=(",", ":"))
    print({k: len(v) for k, v in rec.items()}, "->", out)


def gpu_iteration(which, dev="cuda:0"):
    """One fp8 + fp8_wgrad iteration of a fresh trainer at GPU_S x GPU_S, batch GPU_B -> its bit-level record."""
    from gan_variant_research_amd.runtime import HipOps
    ops = HipOps(torch.device(dev))
    if which == "basic":
        tr = EB.make_trainer(dev, ops, GPU_S, GPU_B, True, True, True)
        a, b = EB.inputs(GPU_S, GPU_B)
        losses = tr.train_iteration(a.to(dev), b.to(dev))
        torch.cuda.synchronize()
        return EB.state_digest(tr, losses)
    tr = EC.make_trainer(dev, ops, GPU_S, GPU_B, True, True)
    losses = EC.run_steps(tr, GPU_S, GPU_B, 1, dev)[0]
    torch.cuda.synchronize()
    h = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    return {"losses": {k: float(v).hex() for k, v in losses.items()}, "params": {"G": h(tr.opt_G.flat_p), "D": h(tr.opt_D.flat_p)}}


def gpu(out):
    rec = {}
    for which in ("cut", "basic"):
        first, second = gpu_iteration(which), gpu_iteration(which)
        print(which, first)
        if first != second:      # not bit-reproducible on this commit: no golden for it (the oracle tolerance tests still cover the mode)
            print(which, "NOT REPRODUCIBLE, dropped; second run:", second)
            continue
        rec[which] = first
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("->", out)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if what == "launches":
        launches(out or os.path.join(GOLDEN, "plan_parent_launches.json"))
    elif what == "gpu":
        gpu(out or os.path.join(GOLDEN, "plan_parent_gpu.json"))
    else:
        sys.exit(__doc__)
