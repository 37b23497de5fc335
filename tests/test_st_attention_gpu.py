"""GPU tests of the HIP gcn_unit_attention (ST-TR spatial attention) against the reference's fixtures
(tests/golden/make_golden_st_attention.py) and the fp64 restatement in tests/st_attention_ref.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import st_attention_ref as R
from _util import ZERO_GRAD, parity_gate
from entry_points import incidence as _incidence, st_unit as _unit  # noqa: F401 (_incidence: borrowed by the edge tests)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
CASES = {"v22_256_256": (22, 256, 256, 6), "v46_131_256": (46, 131, 256, 4), "v46_256_512": (46, 256, 512, 2),
         "v22_512_512": (22, 512, 512, 2)}


def _fixture():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "st_attention_reference.npz")
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _pick(z, key, t):
    a = t.detach().double().cpu().reshape(-1)
    if key + "@idx" in z:
        return a[torch.from_numpy(z[key + "@idx"])], torch.from_numpy(z[key + "@val"]).double()
    return a, torch.from_numpy(z[key].astype(np.float64))


def _mask_gen(mask):
    """torch.bernoulli replaced for one call: returns the recorded mask (on the requested device)."""
    orig = torch.bernoulli

    def bern(p, *a, **k):
        torch.bernoulli = orig
        assert p.numel() == mask.numel()
        return mask.to(p.device, p.dtype)
    return orig, bern


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_and_gradients_match_reference(name):
    V, cin, cout, T = CASES[name]
    z = _fixture()
    seed = sum(map(ord, name))
    m = _unit(cin, cout, V, R.make_state(cin, cout, V, seed))
    x = R.make_input(2, cin, T, V, seed + 1).to(DEV)
    m.eval()
    with torch.no_grad():
        parity_gate(*_pick(z, f"{name}/y_eval", m(x)), what=f"{name} eval")
    m.train()
    mask = torch.from_numpy(z[f"{name}/mask"].astype(np.float32))
    orig, bern = _mask_gen(mask)
    torch.bernoulli = bern
    try:
        xg = x.clone().requires_grad_(True)
        y = m(xg)
    finally:
        torch.bernoulli = orig
    parity_gate(*_pick(z, f"{name}/y_train", y), what=f"{name} train")
    for k, v in m.state_dict().items():
        if "running" in k:
            parity_gate(*_pick(z, f"{name}/after/{k}", v), what=f"{name} {k}")
        if "num_batches" in k:
            assert int(v) == int(z[f"{name}/after/{k}"][0]) == 4
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 3)).to(DEV)
    y.backward(dy)
    gscale = max(float(m.bn.bias.grad.abs().max()), 1e-6)
    for k, p in m.named_parameters():
        got, ref = _pick(z, f"{name}/grad/{k}", p.grad)
        if k in ZERO_GRAD:
            assert (got - ref).abs().max() <= 1e-4 * gscale, k
        else:
            parity_gate(got, ref, strict=False, what=f"{name} grad {k}")
    parity_gate(*_pick(z, f"{name}/grad/x", xg.grad), strict=False, what=f"{name} dx")


@pytest.mark.parametrize("N,cin,cout,T,V", [(4, 131, 256, 40, 46), (3, 512, 512, 20, 46), (5, 64, 128, 33, 25)])
def test_eval_forward_vs_fp64_many_workgroups(N, cin, cout, T, V):
    sd = R.make_state(cin, cout, V, 7)
    x = R.make_input(N, cin, T, V, 8)
    m = _unit(cin, cout, V, sd).eval()
    with torch.no_grad():
        y = m(x.to(DEV))
    ref, _ = R.forward64({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double(), False)
    parity_gate(y, ref, what="eval vs fp64")


def test_gradients_vs_fp64_autograd_and_rng_state():
    N, cin, cout, T, V = 3, 256, 256, 10, 46
    sd = R.make_state(cin, cout, V, 11)
    x = R.make_input(N, cin, T, V, 12)
    m = _unit(cin, cout, V, sd).train()
    xg = x.to(DEV).requires_grad_(True)
    torch.manual_seed(99)
    y = m(xg)
    state_after = torch.cuda.get_rng_state(DEV)
    torch.manual_seed(99)                                  # the reference's draw: one bernoulli of N*T*Nh*V on the device
    mask = torch.bernoulli(0.5 * torch.ones(N * T * 8 * V, device=DEV))
    assert torch.equal(torch.cuda.get_rng_state(DEV), state_after)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(13))
    y.backward(dy.to(DEV))
    yr, new, g, dx = R.grads64(sd, x, dy, True, mask.cpu())
    parity_gate(y, yr, what="train y")
    for k, v in new.items():
        parity_gate(m.state_dict()[k], v, what=k)
    for k, p in m.named_parameters():
        if k in ZERO_GRAD:
            assert float(p.grad.abs().max()) <= 1e-4 * float(g["bn.bias"].abs().max())
        else:
            parity_gate(p.grad, g[k], strict=False, what=f"grad {k}")
    parity_gate(xg.grad, dx, strict=False, what="dx")


def test_without_drop_connect_and_frozen_batchnorm_under_autograd():
    N, cin, cout, T, V = 2, 131, 128, 12, 22
    sd = R.make_state(cin, cout, V, 21)
    x = R.make_input(N, cin, T, V, 22)
    m = _unit(cin, cout, V, sd).eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    xg = x.to(DEV).requires_grad_(True)
    y = m(xg)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(23))
    y.backward(dy.to(DEV))
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed in eval mode"
    yr, _, g, dx = R.grads64(sd, x, dy, training=False)
    parity_gate(y, yr, what="frozen y")
    for k, p in m.named_parameters():
        parity_gate(p.grad, g[k], strict=False, what=f"frozen grad {k}")
    parity_gate(xg.grad, dx, strict=False, what="frozen dx")


def test_second_identical_step_gives_same_bits():
    N, cin, cout, T, V = 4, 256, 512, 8, 46
    sd = R.make_state(cin, cout, V, 31)
    x = R.make_input(N, cin, T, V, 32).to(DEV)
    outs = []
    for _ in range(2):
        m = _unit(cin, cout, V, sd).train()
        torch.manual_seed(5)
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.backward(torch.ones_like(y))
        outs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    # BatchNorm2d's batch sums are fp64 atomics (train_bn.hip): order-dependent in the last fp64 bits only, which the fp32
    # results do not show in practice; everything else is fixed-order
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_data_parallel_replicas_receive_gradients():
    from torch.nn.parallel import parallel_apply
    from test_data_parallel import _replicas
    N, cin, cout, T, V = 4, 128, 128, 6, 22
    sd = R.make_state(cin, cout, V, 41)
    m = _unit(cin, cout, V, sd).train()
    x = R.make_input(N, cin, T, V, 42).to(DEV)
    with torch.enable_grad():
        reps = _replicas(m, 2)
        outs = parallel_apply(reps, [(x[:2],), (x[2:],)])
        sum(o.sum() for o in outs).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 or k in ZERO_GRAD, k
    st = m.__dict__["_staging"]
    assert len(st._slots) == 1                      # staged once, on the master, for the one device


class _StrUnit(nn.Module):
    """TCN_GCN_unit of model/ST_TR/ST_TR_new.py in the STR configuration: attention unit, Unit2D(k=9, stride 2) and the
    down Unit2D(k=1, stride 2); y = tcn1(gcn1(x)) + down1(x)."""

    def __init__(self, cin, cout, V):
        from stgcn_amd import Unit2D
        super().__init__()
        self.gcn1 = _unit(cin, cout, V)
        self.tcn1 = Unit2D(cout, cout, kernel_size=9, stride=2)
        self.down1 = Unit2D(cin, cout, kernel_size=1, stride=2)

    def forward(self, x):
        return self.tcn1(self.gcn1(x)) + self.down1(x)


def test_str_unit_trains_end_to_end_against_restatement():
    from stgcn_amd import set_math_mode
    N, cin, cout, T, V = 2, 131, 256, 12, 46
    torch.manual_seed(3)
    u = _StrUnit(cin, cout, V).to(DEV).train()
    set_math_mode(u, "f32")
    sd = R.make_state(cin, cout, V, 51)
    u.gcn1.load_state_dict(sd)
    x = R.make_input(N, cin, T, V, 52)
    tcn_sd = {k: v.detach().cpu().double() for k, v in u.tcn1.state_dict().items()}
    down_sd = {k: v.detach().cpu().double() for k, v in u.down1.state_dict().items()}
    xg = x.to(DEV).requires_grad_(True)
    torch.manual_seed(4)
    y = u(xg)
    torch.manual_seed(4)
    mask = torch.bernoulli(0.5 * torch.ones(N * T * 8 * V, device=DEV)).cpu()
    y.sum().backward()

    def unit2d(p, z, stride, K):
        w = p["conv.weight"]
        c = torch.nn.functional.conv2d(z, w, p["conv.bias"], stride=(stride, 1), padding=((K - 1) // 2, 0))
        mu, var = c.mean((0, 2, 3), keepdim=True), c.var((0, 2, 3), unbiased=False, keepdim=True)
        return torch.relu((c - mu) / torch.sqrt(var + 1e-5) * p["bn.weight"].view(1, -1, 1, 1) + p["bn.bias"].view(1, -1, 1, 1))
    sd64 = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    x64 = x.double().clone().requires_grad_(True)
    g1, _ = R.forward64(sd64, x64, True, mask.double())
    yr = unit2d(tcn_sd, g1, 2, 9) + unit2d(down_sd, x64, 2, 1)
    yr.sum().backward()
    parity_gate(y, yr.detach(), what="STR unit y")
    parity_gate(xg.grad, x64.grad, strict=False, what="STR unit dx")
    for k, p in u.gcn1.named_parameters():
        if k not in ZERO_GRAD:
            parity_gate(p.grad, sd64[k].grad, strict=False, what=f"STR unit grad {k}")
