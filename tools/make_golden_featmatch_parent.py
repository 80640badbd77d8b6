"""Records every step program cut.CutTrainer builds BEFORE loss_weights.featmatch was read, for tests/test_featmatch_parent_launches.py.

The record was made on the commit before that change (this file copied into its tree) and is never recomputed from the code under test:

  python tools/make_golden_featmatch_parent.py [--out FILE]      -> tests/golden/featmatch_parent_launches.json

Each case of CASES builds a trainer at 32 x 32, batch 2, fp32, on tests.emulator_dfamily.DFamilyEmuOps behind a recording wrapper (RecOps):
every op constructor of the layer tags the launches it returns with its own name and a summary of its arguments -- scalars as they are, a
view as its geometry (B, H, W, C, halo, dtype), a tensor as its element count and dtype, descriptors (ConvCall, WgradCall) field by field.
Per mode of the trainer (identity pass merged or not) and per step program the record holds that (name, arguments) pair of every launch in
order; beside them the size of `losses` and the keys of the loss dict.  Launches and programs repeat across the cases, so the file stores
each distinct launch and each distinct program once and the cases refer to them by index.

  absent-*    the shipped small config with `featmatch` removed from loss_weights
  zero-*      the key present and 0
  *-k1 / *-k3     one / three discriminator scales;  *-sn: with spectral norm
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_variant_research_amd import cut as C  # noqa: E402
from gan_variant_research_amd.runtime import View  # noqa: E402
from tests import cases  # noqa: E402
from tests.emulator_dfamily import DFamilyEmuOps  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "featmatch_parent_launches.json")
S, B = 32, 2
PLAIN = ("side", "fork", "bind")          # these hand out op layers, not launches
PROGRAMS = ("prog_gfwd", "prog_d_compute", "prog_g_features", "prog_g_adversarial", "prog_g_features_bwd", "prog_g_compute", "prog_g_identity",
            "prog_fake_out", "prog_d_update", "prog_r1_compute", "prog_r1_update", "prog_g_update", "prog_palette")


def summary(a):
    """What the record keeps of one constructor argument (see the module text)."""
    if isinstance(a, View):
        return ["view", a.B, a.H, a.W, a.C, a.halo, a.dtype]
    if isinstance(a, torch.Tensor):
        return ["tensor", a.numel(), str(a.dtype)]
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if dataclasses.is_dataclass(a):
        return [type(a).__name__] + [[f.name, summary(getattr(a, f.name))] for f in dataclasses.fields(a)]
    if isinstance(a, (list, tuple)):
        return [summary(x) for x in a]
    if isinstance(a, dict):
        return {str(k): summary(a[k]) for k in sorted(a, key=str)}
    return "callable" if callable(a) else type(a).__name__


class RecOps(DFamilyEmuOps):
    """The emulator with every op constructor tagging what it returns: `_entry` = the constructor's name, `_args` = summary of its arguments."""

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name.startswith("_") or name in PLAIN or not callable(attr) or not hasattr(type(self), name):
            return attr

        def tagged(*a, **k):
            out = attr(*a, **k)
            args = summary(list(a) + [[key, k[key]] for key in sorted(k)])
            for o in (out if isinstance(out, (list, tuple)) else [out]):
                if callable(o):
                    try:
                        o._entry, o._args = name, args
                    except AttributeError:
                        pass
            return out
        return tagged


def config(key, K, sn):
    cfg = cases.small_config()
    cfg["diffaugment"]["enable"] = False
    cfg["model"]["discriminator"].update(num_scales=K, use_spectral_norm=sn)
    if key is None:
        cfg["loss_weights"].pop("featmatch", None)
    else:
        cfg["loss_weights"]["featmatch"] = key
    return cfg


CASES = {f"{kn}-k{K}{'-sn' if sn else ''}": (key, K, sn) for kn, key in (("absent", None), ("zero", 0.0)) for K in (1, 3) for sn in (False, True)}


def _launches(prog):
    if prog is None:
        return None
    return [[getattr(op, "_entry", getattr(op, "__name__", type(op).__name__)), getattr(op, "_args", None)] for op in prog.ops]


def record(name):
    """Builds the trainer of CASES[name] on a recording op layer -> {"programs": {mode: {program: launches}}, "losses": n, "keys": [...]}."""
    key, K, sn = CASES[name]
    torch.set_num_threads(4)
    C.set_seed(42)
    cfg = config(key, K, sn)
    gen, disc = C.build_models(cfg, "cpu")
    tr = C.CutTrainer(gen, disc, cfg, B, S, device="cpu", amp=False, ops=RecOps())
    out = {"programs": {}, "losses": tr.losses.numel()}
    for merged in (True, False):
        tr._use_mode(merged)
        out["programs"][f"merged={merged}"] = {p: _launches(getattr(tr, p)) for p in PROGRAMS}
    # the dict of a step whose slots are all zero: its keys are what a step returns (an R1 step with the identity term on)
    out["keys"] = sorted(tr._loss_dict([0.0] * tr.losses.numel(), (0, C.identity_weight_at(0, cfg), True)))
    return json.loads(json.dumps(out))


def pack(records):
    """{case: record} -> the stored form: distinct launches and distinct programs once, the cases hold indices."""
    launches, programs, li, pi = [], [], {}, {}

    def intern(table, index, item):
        k = json.dumps(item, sort_keys=True)
        if k not in index:
            index[k] = len(table)
            table.append(item)
        return index[k]
    cases_ = {}
    for name, rec in records.items():
        progs = {mode: {p: (None if ls is None else intern(programs, pi, [intern(launches, li, l) for l in ls])) for p, ls in ps.items()}
                 for mode, ps in rec["programs"].items()}
        cases_[name] = {"programs": progs, "losses": rec["losses"], "keys": rec["keys"]}
    return {"launches": launches, "programs": programs, "cases": cases_}


def unpack(stored, name):
    """The record of one case, as record() returns it."""
    c = stored["cases"][name]
    progs = {mode: {p: (None if i is None else [stored["launches"][j] for j in stored["programs"][i]]) for p, i in ps.items()}
             for mode, ps in c["programs"].items()}
    return {"programs": progs, "losses": c["losses"], "keys": c["keys"]}


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    stored = pack({name: record(name) for name in CASES})
    with open(out, "w") as f:
        json.dump(stored, f, separators=(",", ":"))
    print(len(stored["launches"]), "distinct launches,", len(stored["programs"]), "distinct programs,", os.path.getsize(out), "bytes ->", out)
