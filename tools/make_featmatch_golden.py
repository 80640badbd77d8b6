"""Records what the reference's MultiscaleDiscriminator.get_intermediate_features returns, for tests/test_featmatch_cpu.py / _gpu.py:

  python tools/make_featmatch_golden.py --reference PATH [--out FILE]      -> tests/golden/featmatch_reference.npz

PATH is the reference's root: its GAN_Variant1/models/discriminator_patchgan.py is loaded from there and nothing of it is kept but data.
Two seeded discriminators (ndf 8, n_layers 3), a 2 x 3 x 32 x 32 input `x` and a 1 x 3 x 64 x 64 input `x64` (the second scale of a 32 x 32
input is 16 x 16, which the reference's last 4 x 4 convolution refuses: it runs every module, the logits' too):

  ms2     2 scales, no spectral norm, on x64:   ms2.sd.<key>, ms2.feat.<scale>.<layer>
  sn1     1 scale, spectral norm:       sn1.sd.<key> (weight_orig, weight_u, weight_v, bias as constructed, before any forward),
                                        sn1.eval.feat.0.<layer>   eval mode: the stored u, v, no power iteration
                                        sn1.train.feat.0.<layer>  train mode: one power iteration from the stored u, v
          both on x
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "featmatch_reference.npz")
NDF, N_LAYERS, SHAPE = 8, 3, (2, 3, 32, 32)


def load_reference(path):
    spec = importlib.util.spec_from_file_location("ref_discriminator_patchgan", os.path.join(path, "GAN_Variant1", "models", "discriminator_patchgan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[sys.argv.index("--reference") + 1])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    torch.manual_seed(20261021)
    x, x64 = torch.rand(SHAPE) * 2 - 1, torch.rand(1, SHAPE[1], 64, 64) * 2 - 1
    rec = {"x": x.numpy(), "x64": x64.numpy()}

    def feats(tag, d, inp=x):
        with torch.no_grad():
            nested = d.get_intermediate_features(inp.clone())
        assert len(nested) == d.num_scales and all(len(f) == N_LAYERS + 1 for f in nested)
        for s, fs in enumerate(nested):
            for j, t in enumerate(fs):
                rec[f"{tag}.feat.{s}.{j}"] = t.numpy().copy()

    d = ref.MultiscaleDiscriminator(3, NDF, N_LAYERS, 2, False)
    rec.update({f"ms2.sd.{k}": v.numpy().copy() for k, v in d.state_dict().items()})
    feats("ms2", d, x64)
    d = ref.MultiscaleDiscriminator(3, NDF, N_LAYERS, 1, True)
    sd = {k: v.clone() for k, v in d.state_dict().items()}
    rec.update({f"sn1.sd.{k}": v.numpy().copy() for k, v in sd.items()})
    d.eval()
    feats("sn1.eval", d)
    d.load_state_dict(sd)
    d.train()
    feats("sn1.train", d)
    np.savez_compressed(out, **rec)
    print(len(rec), "arrays,", os.path.getsize(out), "bytes ->", out)


if __name__ == "__main__":
    main()
