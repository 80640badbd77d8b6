"""Records the launches cut.CutTrainer builds for the PatchNCE term BEFORE patchnce.nce_includes_all_negatives_from_minibatch was read, for
tests/test_nce_all_parent_launches.py.

The record was made on the commit before that change (this file copied into its tree) and is never recomputed from the code under test:

  python tools/make_golden_nce_parent.py [--out FILE]      -> tests/golden/nce_parent_launches.json

Each case of CASES builds a trainer at 32 x 32, batch 2, on tests.emulator.EmuOps behind a recording wrapper (RecOps): every op constructor
of the layer tags the launches it returns with its own name.  Per mode of the trainer (identity pass merged or not) the record holds the
entry point of every launch of the G-features program and of the features-backward program (which holds the hooks' launches), in order; and
per gan_patchnce_* call the entry point, P, C, temperature, weight, the geometry of its views and the size of its workspace, with the
arguments of every gan_patchnce_ws_floats call.

  absent      the shipped small config with the key removed from `patchnce`
  false       the key present and false
  no-nce      loss_weights.patchnce = 0 with the key false: no PatchNCE launch at all
"""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_variant_research_amd import cut as C  # noqa: E402
from tests import cases  # noqa: E402
from tests.emulator import EmuOps  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "nce_parent_launches.json")
KEY = "nce_includes_all_negatives_from_minibatch"
S, B = 32, 2
PLAIN = ("side", "fork", "bind")          # these hand out op layers, not launches


def _geom(v):
    return [v.B, v.H, v.W, v.C, v.halo, v.dtype]


class RecOps(EmuOps):
    """EmuOps whose op constructors tag what they return with the constructor's name, and whose patchnce_* calls are logged."""

    def __init__(self, log):
        super().__init__()
        self.log = log

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name.startswith("_") or name in PLAIN or not callable(attr) or not hasattr(type(self), name):
            return attr

        def tagged(*a, **k):
            out = attr(*a, **k)
            for o in (out if isinstance(out, (list, tuple)) else [out]):
                if callable(o):
                    try:
                        o._entry = name
                    except AttributeError:
                        pass
            return out
        return tagged

    def patchnce_ws_floats(self, Bn, P, Cc):
        self.log["ws_floats"].append([Bn, P, Cc])
        return super().patchnce_ws_floats(Bn, P, Cc)

    def patchnce_fwd(self, src, tgt, ids, P, Cc, temperature, weight, loss, ws):
        self.log["nce"].append(["patchnce_fwd", P, Cc, temperature, weight, _geom(src), _geom(tgt), ids.numel(), loss.numel(), ws.numel()])
        return super().patchnce_fwd(src, tgt, ids, P, Cc, temperature, weight, loss, ws)

    def patchnce_bwd(self, tgt, ids, P, Cc, temperature, weight, gtgt, ws):
        self.log["nce"].append(["patchnce_bwd", P, Cc, temperature, weight, _geom(tgt), _geom(gtgt), ids.numel(), ws.numel()])
        return super().patchnce_bwd(tgt, ids, P, Cc, temperature, weight, gtgt, ws)


def _config(key, nce=True):
    cfg = cases.small_config()
    cfg["diffaugment"]["enable"] = False
    if key is None:
        cfg["patchnce"].pop(KEY, None)
    else:
        cfg["patchnce"][KEY] = key
    if not nce:
        cfg["loss_weights"]["patchnce"] = 0.0
    return cfg


CASES = {"absent": (None, True), "false": (False, True), "no-nce": (False, False)}


def _entries(prog):
    return None if prog is None else [getattr(op, "_entry", getattr(op, "__name__", type(op).__name__)) for op in prog.ops]


def record(name):
    """Builds the trainer of CASES[name] on a recording op layer -> {"nce": [...], "ws_floats": [...], "programs": {...}}."""
    key, nce = CASES[name]
    log = {"nce": [], "ws_floats": [], "programs": {}}
    torch.set_num_threads(4)
    C.set_seed(42)
    cfg = _config(key, nce)
    gen, disc = C.build_models(cfg, "cpu")
    tr = C.CutTrainer(gen, disc, cfg, B, S, device="cpu", amp=False, ops=RecOps(log))
    for merged in (True, False):
        tr._use_mode(merged)
        log["programs"][f"merged={merged}"] = {"features": _entries(tr.prog_g_features), "features_bwd": _entries(tr.prog_g_features_bwd)}
    return json.loads(json.dumps(log))


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    rec = {name: record(name) for name in CASES}
    with open(out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print({k: (len(v["nce"]), len(v["programs"]["merged=True"]["features"])) for k, v in rec.items()}, "->", out)
