"""TEST INFRASTRUCTURE: cut.CutTrainer with optim.{G,D}.weight_decay, against an op layer: tests/test_cut_trainer_wd_cpu.py runs the bodies on
tests/emulator_optim_wd.py, tests/test_cut_trainer_wd_gpu.py on HipOps.  Smallest step configuration of tests/cases.py (small_config, fp32)
at 64 x 64, batch 1.  The generator update of a step is held to the float64 statement of tests/optim_wd_ref64.py with the bounds of
tests/optim_wd_cases.py: the norm over the whole gradient block, the elements on the first and last SAMPLE elements of every tensor (the
update is elementwise once the coefficient is known, and the family tests cover every chunk position)."""
import copy
import math

import pytest
import torch

from gan_variant_research_amd import cut as C
from tests import cases
from tests import optim_cases as P
from tests import optim_ref64 as R
from tests import optim_wd_cases as Q
from tests.pointwise_cases import same_bits, t32

S, B, SAMPLE = 64, 1, 2048
WD_G, WD_D = 0.1, 0.05


def config(wd_g=WD_G, wd_d=WD_D, decoupled=False):
    cfg = cases.small_config()
    cfg["diffaugment"]["enable"] = False
    cfg["optim"]["G"]["weight_decay"], cfg["optim"]["D"]["weight_decay"] = wd_g, wd_d
    if decoupled:
        cfg["mi355x"] = {"decoupled_weight_decay": True}
    return cfg


def trainer(ops, device, cfg):
    torch.set_num_threads(4)
    C.set_seed(42)
    gen, disc = C.build_models(cfg, "cpu")
    return C.CutTrainer(gen, disc, cfg, B, S, device=device, amp=False, ops=ops)


def batch(device):
    g = torch.Generator().manual_seed(1234)
    return (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(device), (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(device)


def step(tr, k, device):
    torch.manual_seed(9000 + k)
    rnd = tr.sample_randomness()
    photos, monets = batch(device)
    out = tr.train_step(k, photos, monets, rnd)
    _sync(tr)
    return out


def _sync(tr):
    if tr.device.type == "cuda":
        torch.cuda.synchronize()


def first_launch(prog):
    return getattr(prog.ops[0], "__name__", "")


def snapshot(opt):
    return dict(p=opt.flat_p.detach().cpu().clone(), m=opt.flat_m.detach().cpu().clone(), v=opt.flat_v.detach().cpu().clone(),
                ema=opt.flat_ema.detach().cpu().clone() if opt.flat_ema is not None else None, steps=opt.steps.cpu().clone())


def check_update(tr, opt, before, max_norm, what):
    """opt's state after its update against the float64 statement applied to `before`, with the gradient block the step left and the
    coefficient the kernel wrote"""
    after, g = snapshot(opt), opt.flat_g.detach().cpu().clone()
    norm = opt.norm_out.cpu()[:3]
    wrote_norm, wrote_coef, wrote_found = (float(x) for x in norm)
    f = t32
    o = {**Q.DEFAULT, "lr": opt.lr, "lr_dev": opt.lr, "b1": opt.betas[0], "b2": opt.betas[1], "eps": opt.eps, "max_norm": max_norm, "ema": opt.flat_ema is not None,
         "ema_decay": opt.ema_decay if opt.ema_decay is not None else 0.0, "wd": opt.weight_decay, "decoupled": opt.decoupled}
    K = sum(opt.sizes)
    live = torch.zeros(g.numel(), dtype=torch.bool)
    for i, n in enumerate(opt.sizes):
        live[int(opt.offsets[i]):int(opt.offsets[i]) + n] = True
    assert not bool(g[~live].any()), "the padding of the gradient block is not zero"
    S64 = float((g.double() ** 2).sum())
    worst = {"norm": P.ratio(torch.tensor(wrote_norm), math.sqrt(S64), P.norm_bound(S64, K, opt.nchunks))}
    want_coef = R.coef64(wrote_norm, f(max_norm))
    worst["coef"] = P.ratio(torch.tensor(wrote_coef), want_coef, 2.02 * P.U * abs(want_coef))
    assert wrote_found == 0.0 and math.isfinite(wrote_norm) and wrote_norm > 0
    idx = lambda i: (lambda o_, n: torch.cat([torch.arange(o_, o_ + min(n, SAMPLE)), torch.arange(o_ + max(n - SAMPLE, min(n, SAMPLE)), o_ + n)]))(int(opt.offsets[i]), opt.sizes[i])
    tb, ta = [], []
    for i in range(len(opt.names)):
        ix = idx(i)
        tb.append(dict(p=before["p"][ix], g=g[ix], m=before["m"][ix], v=before["v"][ix], ema=before["ema"][ix] if before["ema"] is not None else None,
                       step=int(before["steps"][i])))
        ta.append(dict(p=after["p"][ix], g=g[ix], m=after["m"][ix], v=after["v"][ix], ema=after["ema"][ix] if after["ema"] is not None else None,
                       step=int(after["steps"][i])))
    rate = f(opt.lr)
    args = (rate, f(o["b1"]), f(o["b2"]), f(o["eps"]), f(max_norm), 1.0, None, f(o["ema_decay"]), False, f(o["wd"]), bool(o["decoupled"]))
    Q.check_elements(o, what, 0, tb, ta, args, rate, wrote_coef, False, rate, worst)
    print(f"[cut-wd] {what}: error / bound = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the derived bound (error / bound): {bad}"
    moved = (after["p"][live] != before["p"][live]).float().mean()
    assert float(moved) > 0.9, f"{what}: only {float(moved):.2f} of the parameters moved"


def body_config_and_update(make_ops, device, decoupled, with_r1_step):
    """-> the trainer after step 1 (for the checkpoint body)"""
    cfg = config(decoupled=decoupled)
    tr = trainer(make_ops(), device, cfg)
    assert (tr.opt_G.weight_decay, tr.opt_D.weight_decay, tr.opt_G.decoupled, tr.opt_D.decoupled) == (WD_G, WD_D, decoupled, decoupled)
    for prog in (tr.prog_g_update, tr.prog_d_update):
        assert first_launch(prog) == "gan_adam_step_wd", f"{prog.name} launches {first_launch(prog)!r}"
    if with_r1_step:        # step 0 runs R1 with the skip table: the skipped tensors must not move, decay or no decay
        seen = {}
        run = tr.prog_r1_update.run

        def wrapped():
            _sync(tr)
            seen["before"] = snapshot(tr.opt_D)
            run()
            _sync(tr)
            seen["after"] = snapshot(tr.opt_D)
        tr.prog_r1_update.run = wrapped
        step(tr, 0, device)
        tr.prog_r1_update.run = run
        assert first_launch(tr.prog_r1_update) == "gan_adam_step_wd" and tr._r1_skip and "before" in seen
        skipped = [tr.opt_D.names.index(k) for k in tr._r1_skip]
        for i, k in enumerate(tr.opt_D.names):
            sl = slice(int(tr.opt_D.offsets[i]), int(tr.opt_D.offsets[i]) + tr.opt_D.sizes[i])
            same = all(same_bits(seen["after"][q][sl], seen["before"][q][sl]) for q in ("p", "m", "v"))
            if i in skipped:
                assert bool(seen["before"]["p"][sl].any()), f"{k}: a skipped tensor of zeros shows nothing"
                assert same and int(seen["after"]["steps"][i]) == int(seen["before"]["steps"][i]), f"{k} is in the R1 skip table and was written"
            else:
                assert not same and int(seen["after"]["steps"][i]) == int(seen["before"]["steps"][i]) + 1, f"{k} is live in the R1 update and did not move"
    before = snapshot(tr.opt_G)
    step(tr, 1, device)                 # no R1; the gradient block of the generator survives the step
    check_update(tr, tr.opt_G, before, cfg["grad_clip_g"], f"G-update decoupled={decoupled}")
    return tr, cfg


def body_checkpoint(make_ops, device, tr, cfg, tmp_path):
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path, 2)
    ck = torch.load(path, weights_only=True)
    g0, d0 = ck["opt_G"]["param_groups"][0], ck["opt_D"]["param_groups"][0]
    assert g0["weight_decay"] == WD_G and d0["weight_decay"] == WD_D and "decoupled_weight_decay" not in g0
    shapes = [tr.opt_G.params[n].shape for n in tr.opt_G.names]
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(s)) for s in shapes], lr=2e-4, betas=(0.5, 0.999), weight_decay=WD_G)
    ref_opt.load_state_dict(ck["opt_G"])
    assert ref_opt.param_groups[0]["weight_decay"] == WD_G and int(ref_opt.state[ref_opt.param_groups[0]["params"][0]]["step"]) == int(tr.opt_G.steps[0])
    tr2 = trainer(make_ops(), device, copy.deepcopy(cfg))
    tr2.load_checkpoint(path)
    for t in (tr, tr2):
        step(t, 2, device)
    for a, b in ((tr.opt_G, tr2.opt_G), (tr.opt_D, tr2.opt_D)):
        sa, sb = snapshot(a), snapshot(b)
        assert all(same_bits(sa[k], sb[k]) for k in ("p", "m", "v")) and torch.equal(sa["steps"], sb["steps"]), "the resumed trainer took another step"
        assert sa["ema"] is None or same_bits(sa["ema"], sb["ema"])
    other = trainer(make_ops(), device, config(wd_g=0.2))
    with pytest.raises(ValueError, match="hyper-parameters differ"):
        other.load_checkpoint(path)
    plain = trainer(make_ops(), device, config(wd_g=0.0, wd_d=0.0))
    assert first_launch(plain.prog_g_update) == first_launch(plain.prog_d_update) == first_launch(plain.prog_r1_update) == "gan_adam_step"
    assert plain.checkpoint(0)["opt_G"]["param_groups"][0] == {"lr": 2e-4, "betas": (0.5, 0.999), "eps": 1e-8, "weight_decay": 0.0, "amsgrad": False,
                                                               "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                                                               "params": list(range(len(plain.opt_G.names)))}
    with pytest.raises(ValueError, match="hyper-parameters differ"):
        plain.load_checkpoint(path)
