"""runtime.stream_key / cached_plan: every plan is keyed on the stream that is current on its TENSORS' device, the stream the op layer
bakes into the launches (HipOps._s), not on the current device's.

Without a GPU this is held in two halves.  stream_key itself, against a fake torch.cuda.current_stream that records the device it is asked
about: it asks for the device it was given and answers 0 for a CPU device without asking (torch refuses a CPU device there, so CPU tensors
cannot reach the fake).  And the four sites that key a plan -- ops_library's plans, losses' plans, HipAdam._plan, fused_adam_launch -- on
the emulator, with stream_key replaced by a recorder: each hands it the device of the tensors it was called with, and a second handle for
that device gives a second plan.  With two GPUs the whole is run for real: two streams of a GPU that is not current get two plans, and
both results are right."""
import pytest
import torch

from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd import losses as LS
from gan_variant_research_amd import ops_library as L
from gan_variant_research_amd import runtime as R
from gan_variant_research_amd import training as T
from tests.cases import U_F32, assert_within_bound, conv_ref64
from tests.emulator import EmuOps


def test_stream_key_asks_for_the_current_stream_of_the_device_it_is_given(monkeypatch):
    asked = []

    class Handle:
        def __init__(self, device):
            self.cuda_stream = 1000 + torch.device(device).index

    def current_stream(device=None):
        asked.append(device)
        return Handle(device)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    assert R.stream_key(torch.device("cuda", 1)) == 1001 and R.stream_key("cuda:0") == 1000
    assert asked == [torch.device("cuda", 1), torch.device("cuda", 0)]
    assert R.stream_key(torch.device("cpu")) == 0 and R.stream_key("cpu") == 0 and len(asked) == 2
    cache = {}
    a = R.cached_plan(cache, ("k",), torch.device("cuda", 1), object)
    assert R.cached_plan(cache, ("k",), torch.device("cuda", 1), object) is a and R.cached_plan(cache, ("k",), torch.device("cuda", 0), object) is not a
    assert sorted(cache) == [("k", 1000), ("k", 1001)] and asked[2:] == [torch.device("cuda", 1)] * 2 + [torch.device("cuda", 0)]


def _sites():
    """name -> (the plan cache, a call on CPU tensors that plans once per stream handle)"""
    x, w = torch.randn(1, 8, 8, 8), torch.randn(8, 8, 3, 3)
    ps = [torch.nn.Parameter(torch.randn(5))]
    opt = T.HipAdam(ps)

    def hipadam():
        ps[0].grad = torch.ones(5)
        opt.step()
    state = [[torch.randn(5)], [torch.zeros(5)], [torch.zeros(5)]]
    steps = torch.zeros(1, dtype=torch.int32)
    return {"ops_library": (lambda: L._PLANS, lambda: torch.ops.mi355x_gan.conv2d_fwd(x, w, None, 1, 1, L.PAD_ZERO, 0)),
            "losses": (lambda: LS._PLANS, lambda: LS.l1_loss(x, x + 1.0)),
            "HipAdam._plan": (lambda: opt._plans, hipadam),
            "fused_adam_launch": (lambda: T._FUSED_PLANS, lambda: T.fused_adam_launch(state[0], [torch.ones(5)], state[1], state[2], [], steps, 2e-4, 0.5,
                                                                                       0.999, 1e-8, 0.0, 1.0, 0.0))}


@pytest.mark.parametrize("site", ["ops_library", "losses", "HipAdam._plan", "fused_adam_launch"])
def test_every_site_keys_its_plan_on_the_stream_of_the_tensors_device(monkeypatch, site):
    asked, handle = [], [7]

    def recorder(device):
        asked.append(device)
        return handle[0]
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: EmuOps())
    for mod, name, val in ((L, "_PLANS", {}), (LS, "_PLANS", {}), (T, "_FUSED_PLANS", {}), (R, "stream_key", recorder), (T, "stream_key", recorder)):
        monkeypatch.setattr(mod, name, val)
    cache, call = _sites()[site]
    call()
    call()
    assert len(cache()) == 1 and all(k[-1] == 7 for k in cache())
    handle[0] = 8          # another stream became current on that device
    call()
    assert len(cache()) == 2 and sorted(k[-1] for k in cache()) == [7, 8]
    assert len(asked) == 3 and all(torch.device(d) == torch.device("cpu") for d in asked), asked


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (a plan on one that is not current)")
def test_two_streams_of_a_gpu_that_is_not_current_get_two_plans(monkeypatch):
    monkeypatch.setattr(L, "_PLANS", {})
    assert torch.cuda.current_device() == 0
    dev = torch.device("cuda", 1)
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(1, 8, 8, 8, generator=g), torch.randn(8, 8, 3, 3, generator=g)
    ref, A, K = conv_ref64("fwd", 3, 1, 1, False, False, w.double(), x=x.double())
    xd, wd = x.to(dev), w.to(dev)
    got = []
    for s in (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)):
        with torch.cuda.device(1):
            torch.cuda.set_stream(s)
        assert torch.cuda.current_device() == 0 and torch.cuda.current_stream(dev) == s
        got.append(torch.ops.mi355x_gan.conv2d_fwd(xd, wd, None, 1, 1, L.PAD_ZERO, 0))
    torch.cuda.synchronize(dev)
    with torch.cuda.device(1):
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
    assert len(L._PLANS) == 2 and len({k[-1] for k in L._PLANS}) == 2
    for y in got:
        assert_within_bound(y.cpu(), ref, A, K, U_F32, "conv2d_fwd on a stream of cuda:1")
