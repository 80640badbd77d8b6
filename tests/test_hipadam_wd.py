"""training.HipAdam / HipAdamW with weight decay against torch.optim.Adam / AdamW: on tests/emulator_optim_wd.py without a GPU, and the same
bodies on the HIP kernels under the gpu mark.  Every step is compared from the optimiser's own state before it (the float64 torch optimiser is
given that state, both take one step), so nothing compounds and the bound is the one-step replay of tests/optim_wd_cases.py with the
coefficient 1 (no clipping here) and the learning rate of that step."""
import pytest
import torch

from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd import training as T
from gan_variant_research_amd.runtime import HipOps
from tests import optim_cases as P
from tests import optim_wd_cases as Q
from tests.emulator_optim_wd import WdEmuOps
from tests.pointwise_cases import same_bits, t32

SHAPES = [(5,), (3, 4), (16385,), (7,)]          # the third crosses a chunk; the last never gets a gradient
# every scalar is an fp32 number, so torch's float64 step and the kernel start from the same hyper-parameters (with beta2 = 0.999 the fp32 1 - beta2
# alone is 1.3e-5 away from torch's, include/mi355x_gan.h) and the bound is the replay's alone
LR, BETAS, EPS, WD = 2.0 ** -7, (0.5, 0.75), 2.0 ** -27, 0.125
BACKENDS = [pytest.param(("cpu", lambda device: WdEmuOps()), id="emulator"),
            pytest.param(("cuda:0", lambda device: HipOps(device)), id="hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def backend(request, monkeypatch):
    """-> (device, counts): every op layer the optimiser builds counts its adam_step, adam_step_wd and make_adam_table calls"""
    device, factory = request.param
    counts = {"adam_step": 0, "adam_step_wd": 0, "make_adam_table": 0}

    def counting(dev):
        ops = factory(dev)
        for name in counts:
            def wrap(*a, _f=getattr(ops, name), _n=name, **k):
                counts[_n] += 1
                return _f(*a, **k)
            setattr(ops, name, wrap)
        return ops
    monkeypatch.setattr(AG, "_OPS_FACTORY", counting)
    return device, counts


def _params(device, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(device)) for s in SHAPES]


def _grads(ps, g, skip_last=True):
    for i, p in enumerate(ps):
        p.grad = None if (skip_last and i == len(ps) - 1) else torch.randn(p.shape, generator=g).to(p.device)


def _twin_step(mine, ps, make_torch, decoupled, wd_of, what, sched=None):
    """one step of `mine` and of a fresh float64 torch optimiser that starts from mine's state -> worst error / bound"""
    p64 = [torch.nn.Parameter(p.detach().cpu().double()) for p in ps]
    topt = make_torch(p64)
    for group, tgroup in zip(mine.param_groups, topt.param_groups):
        tgroup["lr"] = group["lr"]
    before = []
    for p, q in zip(ps, p64):
        st = mine.state.get(p, {})
        m = st["exp_avg"].detach().cpu().clone() if "exp_avg" in st else torch.zeros(p.shape)
        v = st["exp_avg_sq"].detach().cpu().clone() if "exp_avg_sq" in st else torch.zeros(p.shape)
        k = int(st["step"]) if "step" in st else 0
        q.grad = p.grad.detach().cpu().double() if p.grad is not None else None
        if q.grad is not None:
            topt.state[q] = {"step": torch.tensor(float(k)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
        before.append(dict(p=p.detach().cpu().clone().reshape(-1), g=None if p.grad is None else p.grad.detach().cpu().clone().reshape(-1),
                           m=m.reshape(-1), v=v.reshape(-1), ema=None, step=k))
    rates = [float(g["lr"]) for g in mine.param_groups]
    mine.step()
    topt.step()
    if ps[0].is_cuda:
        torch.cuda.synchronize()
    worst = 0.0
    owner = {id(p): gi for gi, g in enumerate(mine.param_groups) for p in g["params"]}
    for p, q, tb in zip(ps, p64, before):
        if tb["g"] is None:
            assert same_bits(p.detach().cpu().reshape(-1), tb["p"]), f"{what}: a parameter without a gradient was written"
            assert "exp_avg" not in mine.state.get(p, {}) or same_bits(mine.state[p]["exp_avg"].cpu().reshape(-1), tb["m"])
            continue
        gi = owner[id(p)]
        wd = wd_of(gi)
        o = {**Q.DEFAULT, "b1": BETAS[0], "b2": BETAS[1], "eps": EPS, "wd": wd, "decoupled": decoupled, "ema": False}
        t64 = {k: (x.double() if torch.is_tensor(x) else x) for k, x in tb.items()}
        rate = t32(rates[gi])
        pi, mi, vi, _ = Q.replay_wd(t64, o, 1.0, rate) if wd != 0.0 else P.replay(t64, o, 1.0, rate)
        st = mine.state[p]
        assert int(st["step"]) == tb["step"] + 1 == int(topt.state[q]["step"])
        for got, want, e in ((p.detach(), q.detach(), pi), (st["exp_avg"], topt.state[q]["exp_avg"], mi), (st["exp_avg_sq"], topt.state[q]["exp_avg_sq"], vi)):
            worst = max(worst, P.ratio(got.cpu().reshape(-1), want.reshape(-1), e.e))
    print(f"[hipadam-wd] {what}: error / bound = {worst:.3g}")
    assert worst <= 1.0, f"{what}: error / bound = {worst}"
    return worst


KINDS = {
    "adam-l2": (lambda ps: T.HipAdam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD),
                lambda ps: torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD), False),
    "adamw": (lambda ps: T.HipAdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD),
              lambda ps: torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD), True),
    "adam-decoupled": (lambda ps: T.HipAdam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, decoupled_weight_decay=True),
                       lambda ps: torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, decoupled_weight_decay=True), True),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_three_steps_equal_torch(backend, kind):
    device, counts = backend
    mk_mine, mk_torch, decoupled = KINDS[kind]
    ps = _params(device)
    mine = mk_mine(ps)
    g = torch.Generator().manual_seed(11)
    for s in range(3):
        _grads(ps, g)
        _twin_step(mine, ps, mk_torch, decoupled, lambda gi: WD, f"{kind} step {s}")
    assert counts["adam_step_wd"] == 1 and counts["adam_step"] == 0 and counts["make_adam_table"] == 1


def test_torchs_default_decay_and_the_refused_arguments(backend):
    device, _ = backend
    ps = _params(device)
    assert T.HipAdamW(ps).defaults["weight_decay"] == 1e-2 and T.HipAdamW(ps).defaults["decoupled_weight_decay"] is True
    assert T.HipAdam(ps).defaults["weight_decay"] == 0.0 and T.HipAdam(ps).defaults["decoupled_weight_decay"] is False
    with pytest.raises(NotImplementedError, match="amsgrad"):
        T.HipAdam(ps, amsgrad=True)
    with pytest.raises(ValueError, match="weight_decay"):
        T.HipAdam(ps, weight_decay=-1.0)
    lin = torch.nn.Linear(2, 2)
    assert type(T.get_optimizer(lin, {"type": "adamw", "weight_decay": 0.3})) is T.HipAdamW
    opt = T.get_optimizer(lin, {"weight_decay": 0.2})
    assert type(opt) is T.HipAdam and opt.param_groups[0]["weight_decay"] == 0.2 and not opt.param_groups[0]["decoupled_weight_decay"]
    with pytest.raises(NotImplementedError):
        T.get_optimizer(lin, {"type": "sgd"})


def test_a_group_without_decay_reaches_adam_step_and_one_with_decay_adam_step_wd(backend):
    device, counts = backend
    ps = _params(device)
    groups = lambda q: [{"params": q[:2], "weight_decay": 0.0}, {"params": q[2:], "weight_decay": WD}]
    mine = T.HipAdam(groups(ps), lr=LR, betas=BETAS, eps=EPS)
    g = torch.Generator().manual_seed(12)
    for s in range(2):
        _grads(ps, g)
        _twin_step(mine, ps, lambda q: torch.optim.Adam(groups(q), lr=LR, betas=BETAS, eps=EPS), False, lambda gi: (0.0, WD)[gi], f"two groups step {s}")
    assert counts == {"adam_step": 1, "adam_step_wd": 1, "make_adam_table": 2}, counts


@pytest.mark.parametrize("kind", ["adam-l2", "adamw"])
def test_a_scheduler_that_moves_the_rate_every_step_keeps_one_plan_and_one_table(backend, kind):
    device, counts = backend
    mk_mine, mk_torch, decoupled = KINDS[kind]
    ps = _params(device)
    mine = mk_mine(ps)
    rule = lambda e: 2.0 ** -e          # fp32 numbers again
    sched = torch.optim.lr_scheduler.LambdaLR(mine, rule)
    g = torch.Generator().manual_seed(13)
    seen = []
    for s in range(5):
        _grads(ps, g)
        seen.append(mine.param_groups[0]["lr"])
        _twin_step(mine, ps, mk_torch, decoupled, lambda gi: WD, f"{kind} LambdaLR step {s}")
        sched.step()
    assert seen == pytest.approx([LR * rule(e) for e in range(5)]) and len(set(seen)) == 5
    assert len(mine._plans) == 1 and counts["make_adam_table"] == 1 and counts["adam_step_wd"] == 1, (len(mine._plans), counts)
    (pl,) = mine._plans.values()
    assert float(pl.lr_dev) == t32(seen[-1])


@pytest.mark.parametrize("kind", list(KINDS))
def test_state_dict_round_trips_with_torch(backend, kind):
    device, _ = backend
    mk_mine, mk_torch, decoupled = KINDS[kind]
    ps = _params(device)
    mine = mk_mine(ps)
    g = torch.Generator().manual_seed(14)
    _grads(ps, g, skip_last=False)
    mine.step()
    sd = mine.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == WD and sd["param_groups"][0]["decoupled_weight_decay"] is decoupled
    topt = mk_torch([torch.nn.Parameter(p.detach().clone()) for p in ps])
    topt.load_state_dict(sd)
    q0 = topt.param_groups[0]["params"][0]
    assert float(topt.state[q0]["step"]) == 1.0 and same_bits(topt.state[q0]["exp_avg"].cpu(), mine.state[ps[0]]["exp_avg"].cpu())
    for p in topt.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    topt.step()
    back = mk_mine(_params(device, seed=1))
    back.load_state_dict(topt.state_dict())
    p0 = back.param_groups[0]["params"][0]
    assert back.param_groups[0]["weight_decay"] == WD and bool(back.param_groups[0]["decoupled_weight_decay"]) is decoupled
    assert back.state[p0]["step"].dtype == torch.int32 and int(back.state[p0]["step"]) == 2
    _grads(back.param_groups[0]["params"], g, skip_last=False)
    back.step()
    assert int(back.state[p0]["step"]) == 3


@pytest.mark.parametrize("decoupled", [False, True])
def test_the_custom_op_takes_the_decay_and_keeps_one_plan_across_rates(backend, decoupled, monkeypatch):
    """mi355x_gan::fused_clip_adam_ema_(..., weight_decay, decoupled) is training.fused_adam_launch (held to float64 by the `launch` cases of
    tests/optim_wd_cases.py) bit for bit, and a second call at another rate reuses the table and the launch"""
    from gan_variant_research_amd import ops_library as L  # noqa: F401  (registers the ops)
    device, counts = backend
    monkeypatch.setattr(T, "_FUSED_PLANS", {})
    g = torch.Generator().manual_seed(15)
    mk = lambda: [torch.randn(s, generator=torch.Generator().manual_seed(16 + i)).to(device) for i, s in enumerate(SHAPES)]
    grads = [[torch.randn(s, generator=g).to(device) for s in SHAPES] for _ in range(2)]
    outs = []
    for via_op in (True, False):
        ps, m, v, ema = mk(), [torch.zeros(s, device=device) for s in SHAPES], [torch.zeros(s, device=device) for s in SHAPES], mk()
        steps = torch.zeros(len(SHAPES), dtype=torch.int32, device=device)
        for k, lr in enumerate((LR, LR / 2)):
            a = (ps, [x.clone() for x in grads[k]], m, v, ema, steps, lr, BETAS[0], BETAS[1], EPS, 1.0, 1.0, 0.75)
            if via_op:
                norm, found = torch.ops.mi355x_gan.fused_clip_adam_ema_(*a, None, False, WD, decoupled)
            else:
                norm, found = T.fused_adam_launch(*a, weight_decay=WD, decoupled=decoupled)
        outs.append([x.cpu() for x in ps + m + v + ema] + [steps.cpu().float(), norm.cpu()])
    assert all(same_bits(a, b) for a, b in zip(*outs)) and outs[0][-2].tolist() == [2.0] * len(SHAPES)
    assert len(T._FUSED_PLANS) == 2 and counts == {"adam_step": 0, "adam_step_wd": 2, "make_adam_table": 2}, (len(T._FUSED_PLANS), counts)
    plain = mk()
    before = [x.clone() for x in plain]
    torch.ops.mi355x_gan.fused_clip_adam_ema_(plain, grads[0], [torch.zeros_like(x) for x in plain], [torch.zeros_like(x) for x in plain], [],
                                              torch.zeros(len(SHAPES), dtype=torch.int32, device=device), LR, BETAS[0], BETAS[1], EPS, 1.0, 1.0, 0.0)
    assert counts["adam_step"] == 1 and not any(same_bits(a.cpu(), b.cpu()) for a, b in zip(plain, before)), "the defaulted arguments mean no decay"
