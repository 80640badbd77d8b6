"""Records the reference's low-frequency Lab statistics into tests/golden/palette_lab.npz:

    python tools/make_palette_golden.py --reference PATH        (PATH: the root of the reference checkout)

The reference's GAN_Variant1/dataio/transforms.py is loaded from PATH at run time (it imports torchvision and PIL at the top; stub
modules stand in for them in sys.modules, none of the three functions used here touches them) and `denormalize`, `rgb_to_lab` and
`get_low_freq_stats` are evaluated on the seeded inputs of tests/palette_cases.py: FIXTURE_INPUTS: per input (mean, std) in float64 and in
float32, and the autograd gradient, in both precisions, of the palette loss of tests/palette_ref64.py (the loss formula is this
project's; the statistic under it is the reference's) against the fixed prior stored with it.  Only the data file is committed.
A record is written only if tests/palette_ref64.py reproduces the reference's float64 values to 1e-12 relative; otherwise the tool stops."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import palette_cases as N  # noqa: E402
from tests import palette_ref64 as R  # noqa: E402


def load_reference(path):
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "PIL", "PIL.Image"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                mod = sys.modules[name] = types.ModuleType(name)
                mod.__path__ = []                                     # a package, so that its stub submodules import
                if "." in name:
                    setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)
    spec = importlib.util.spec_from_file_location("reference_transforms", os.path.join(path, "GAN_Variant1", "dataio", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args(argv)
    ref = load_reference(args.reference)
    pm, ps = torch.tensor(N.FIXTURE_PRIOR[0], dtype=torch.float64), torch.tensor(N.FIXTURE_PRIOR[1], dtype=torch.float64)
    out = {"prior_mean": pm.numpy(), "prior_std": ps.numpy()}
    for tag, (shape, T, seed) in N.FIXTURE_INPUTS.items():
        x = N.fixture_input(shape, seed)
        out[f"{tag}.x"] = x.numpy()
        out[f"{tag}.T"] = np.int32(T)
        for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
            xi = x.clone().to(dt).requires_grad_(True)
            m, s = ref.get_low_freq_stats(ref.rgb_to_lab(ref.denormalize(xi)), T)
            loss = R.loss_from_stats(m, s, pm.to(dt), ps.to(dt))
            (g,) = torch.autograd.grad(loss, xi)
            assert bool(torch.isfinite(g).all()), f"{tag}: the reference's autograd gradient is not finite on this input"
            out[f"{tag}.mean.{name}"], out[f"{tag}.std.{name}"] = m.detach().numpy(), s.detach().numpy()
            out[f"{tag}.loss.{name}"], out[f"{tag}.grad.{name}"] = loss.detach().numpy(), g.numpy()
        m64, s64 = R.stats(x, T)
        g64 = R.grad(x, T, pm, ps)
        for a, b, what in ((m64.numpy(), out[f"{tag}.mean.f64"], "mean"), (s64.numpy(), out[f"{tag}.std.f64"], "std"), (g64.numpy(), out[f"{tag}.grad.f64"], "grad")):
            err = float(np.abs(a - b).max() / np.abs(b).max())
            print(f"{tag} {what}: statement vs reference (float64) {err:.3g} relative")
            if not err <= 1e-12:
                raise SystemExit(f"{tag}: the float64 statement differs from the reference's {what}")
    path = os.path.join(ROOT, "tests", "golden", "palette_lab.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
