"""The drop-in modules under nn.DataParallel, the wrapper every trainer of the reference puts around its model
(SHREC/ST_TS/train_sttran.py:84, LMDHG/ST_TS/LMDHG_sttran.py:79, STR_TTR/train_STR_TTR.py:82).

torch/nn/parallel/replicate.py gives each replica ``_parameters = {}`` and holds the weights as plain attributes, and builds
new replicas on every forward.  The modules must still train (gradients reach the master), run the fused stem in eval, and
keep their staged weights on the master across forwards.  ``_replicas`` builds what replicate.py builds, for replicas that
all sit on the master's own device, so the host tests and one-GPU boxes can drive them (``parallel_apply``: one Python
thread per replica, all entering the C ABI at once).  The last test runs torch.nn.DataParallel itself as the trainer does.
"""
import copy
import pickle
from collections import Counter, OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF
from torch.nn.parallel import parallel_apply

from _util import parity_gate

N, T, V, CLASSES = 8, 20, 22, 5


class _Net(nn.Module):
    """Stand-in caller: the stem of ST_GCN_AltFormer (ST_GCN_AltFormer.py:62-72) and a pooled linear head."""

    def __init__(self, A):
        from stgcn_amd import Unit2D, unit_agcn
        super().__init__()
        self.gcn0 = unit_agcn(3, 128, A)
        self.tcn0 = Unit2D(128, 128, kernel_size=9)
        self.fc = nn.Linear(128, CLASSES)

    def forward(self, x, stem_only=False):            # x: (N, T, V, 3), the loader's layout
        z = self.tcn0(self.gcn0(x.permute(0, 3, 1, 2).contiguous()))
        return z if stem_only else self.fc(z.mean((2, 3)))


def _make_net(seed):
    from stgcn_amd.graphs import SHREGraph
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    net = _Net(torch.from_numpy(SHREGraph("spatial").A.astype(np.float32)))
    with torch.no_grad():                             # default init has bn.weight = 1e-6: make the main branch visible
        net.gcn0.PA.data = torch.randn(3, V, V, generator=gen) * 0.05
        for bn in (net.gcn0.bn, net.gcn0.down[1], net.tcn0.bn):
            bn.weight.copy_(torch.rand(128, generator=gen) + 0.5)
            bn.running_mean.copy_(torch.randn(128, generator=gen) * 0.3)
            bn.running_var.copy_(torch.rand(128, generator=gen) + 0.5)
    return net, gen


def _replicas(net, n):
    """``n`` replicas of ``net`` as torch/nn/parallel/replicate.py makes them, all on ``net``'s device: every module through
    ``_replicate_for_data_parallel()`` with its children re-linked; each parameter an attribute holding ``p.clone()`` (under
    autograd a graph edge back to the master, as Broadcast's output is) and recorded in ``_former_parameters``; the first
    replica shares the master's buffers, the others hold copies.  Call it under the grad mode of the forward."""
    modules = list(net.modules())
    index = {m: i for i, m in enumerate(modules)}
    out = []
    for j in range(n):
        copies = [m._replicate_for_data_parallel() for m in modules]
        for m, r in zip(modules, copies):
            r._former_parameters = OrderedDict()
            for key, child in m._modules.items():
                if child is None:
                    r._modules[key] = None
                else:
                    setattr(r, key, copies[index[child]])
            for key, p in m._parameters.items():
                if p is None:
                    r._parameters[key] = None
                    continue
                pc = p.clone()
                setattr(r, key, pc)
                r._former_parameters[key] = pc
            for key, b in m._buffers.items():
                if b is not None:
                    setattr(r, key, b if j == 0 else b.clone())
        out.append(copies[0])
    return out


# ---------------------------------------------------------------------------------------
# host: what a replica decides, without a GPU
# ---------------------------------------------------------------------------------------
def test_replica_wants_grad_like_its_master():
    from stgcn_amd.modules import _wants_grad
    net, _ = _make_net(1)
    x = torch.zeros(2, 3, 8, V)
    with torch.enable_grad():
        reps = _replicas(net, 2)
    for rep in reps:
        for name in ("gcn0", "tcn0"):
            mod, master = getattr(rep, name), getattr(net, name)
            assert list(mod.parameters()) == []       # the premise: replicate.py leaves a replica without parameters
            with torch.enable_grad():
                assert _wants_grad(master, x), name
                assert _wants_grad(mod, x), f"{name} replica: the training forward would skip autograd"
            with torch.no_grad():
                assert not _wants_grad(mod, x), name


def test_replica_cache_key_covers_the_masters_tensors():
    from stgcn_amd.modules import _master, _state_tensors
    net, gen = _make_net(2)
    with torch.enable_grad():
        rep = _replicas(net, 2)[1]
    dev = torch.device("cuda", 0)                     # (only a dictionary key here)
    for name in ("gcn0", "tcn0"):
        mod, master = getattr(rep, name), getattr(net, name)
        assert _master(mod) is master and _master(master) is master
        want = list(master.parameters()) + list(master.buffers())
        assert len(want) == (31 if name == "gcn0" else 7)
        assert {id(t) for t in _state_tensors(master)} == {id(t) for t in want}
        assert [t.shape for t in _state_tensors(mod)] == [t.shape for t in _state_tensors(master)]
        assert mod._cache_key(dev) == master._cache_key(dev)
    keys = (rep.gcn0._cache_key(dev), rep.tcn0._cache_key(dev))
    with torch.no_grad():
        net.gcn0.conv_d[2].bias.add_(1.0)             # an in-place edit on the master (an optimizer step)
    assert rep.gcn0._cache_key(dev) != keys[0]
    net.tcn0.bn.running_var.data = torch.rand(128, generator=gen) + 0.5    # a buffer swapped by .data assignment
    assert rep.tcn0._cache_key(dev) != keys[1]


def test_replica_without_backward_still_refuses_autograd():
    """Unit2D(dim=3) has no HIP backward: a replica must refuse a grad-requiring call as its master does.  _check_input
    first refuses CPU tensors, so the input is a stand-in that reports itself as a CUDA tensor."""
    from stgcn_amd import Unit2D
    from stgcn_amd.modules import _check_input
    tcn = Unit2D(8, 8, kernel_size=3, dim=3)
    with torch.enable_grad():
        rep = _replicas(tcn, 2)[1]
    x = SimpleNamespace(is_cuda=True, dtype=torch.float32, requires_grad=False, dim=lambda: 4)
    for mod in (tcn, rep):
        with torch.enable_grad(), pytest.raises(NotImplementedError):
            _check_input(mod, x, backward_ok=mod.dim == 2)
        with torch.no_grad():
            _check_input(mod, x, backward_ok=mod.dim == 2)


def test_replica_takes_its_masters_fused_output_only():
    from stgcn_amd import FusedStemOutput, Unit2D
    net, _ = _make_net(3)
    with torch.no_grad():
        rep = _replicas(net, 2)[1]
    z = torch.randn(2, 128, 4, V)
    assert torch.equal(rep.tcn0(FusedStemOutput.wrap(z, net.tcn0)), z)
    with pytest.raises(RuntimeError, match="ANOTHER Unit2D"):
        Unit2D(128, 128, kernel_size=9)(FusedStemOutput.wrap(z, net.tcn0))
    with pytest.raises(RuntimeError, match="ANOTHER Unit2D"):
        rep.tcn0(FusedStemOutput.wrap(z, Unit2D(128, 128, kernel_size=9)))


def test_copies_of_a_module_start_with_their_own_staging():
    from stgcn_amd.modules import _store
    net, _ = _make_net(4)
    for mod in (net.gcn0, net.tcn0):
        for other in (copy.deepcopy(mod), pickle.loads(pickle.dumps(mod))):
            assert _store(other) is not _store(mod)
    with torch.no_grad():
        rep = _replicas(net, 1)[0]
    assert _store(rep.gcn0) is _store(net.gcn0) and _store(rep.tcn0) is _store(net.tcn0)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


_STRUCTURAL_ZERO = {"gcn0.down.0.bias": "gcn0.down.0.weight", "tcn0.conv.bias": "tcn0.conv.weight"}


def _check_stem_grads(got, want):
    """Every stem parameter has a gradient within 1e-4 of the reference's.  Biases in front of a batch-statistics BatchNorm
    (conv_d, down, the temporal conv) and conv_a's (soft-max ignores a shift of its column) have zero gradient: both sides
    are rounding noise there, held against the scale of the matching weight's gradient (as _compare_grads does)."""
    for name, g in got.items():
        if not name.startswith(("gcn0.", "tcn0.")):
            continue
        assert g is not None, f"{name}: no gradient reached the master"
        w = _STRUCTURAL_ZERO.get(name)
        if w is None and name.endswith(".bias") and name.startswith(("gcn0.conv_a.", "gcn0.conv_d.")):
            w = name[:-len("bias")] + "weight"
        if w is None:
            parity_gate(g, want[name], 1e-4, name)
        else:
            err = (g - want[name]).abs().max().item()
            assert err <= 1e-4 * max(want[name].abs().max().item(), want[w].abs().max().item()), f"{name}: {err:.3e}"


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["f32", "default"])
def test_replicas_train_the_stem_through_parallel_apply(math, dev):
    """Training mode, two replicas of 4 clips on one device, run in two threads: the master's stem gradients are the sum of
    the halves' gradients of unwrapped copies, and its BatchNorm statistics are those of the first half (replica 0 shares
    the master's buffers, the other replica's updates are discarded — nn.BatchNorm2d under DataParallel)."""
    from stgcn_amd import set_math_mode
    net, gen = _make_net(10)
    net = net.to(dev).train()
    if math != "default":
        set_math_mode(net, math)
    refs = [copy.deepcopy(net) for _ in range(2)]
    x = torch.randn(N, T, V, 3, generator=gen).to(dev)
    y = torch.randint(0, CLASSES, (N,), generator=gen).to(dev)
    halves = [(x[:N // 2],), (x[N // 2:],)]
    labels = [y[:N // 2], y[N // 2:]]
    outs = parallel_apply(_replicas(net, 2), halves, devices=[dev, dev])
    sum(TF.cross_entropy(o, lab) for o, lab in zip(outs, labels)).backward()
    for ref, (xh,), lab in zip(refs, halves, labels):
        TF.cross_entropy(ref(xh), lab).backward()
    r0, r1 = _grads(refs[0]), _grads(refs[1])
    _check_stem_grads(_grads(net), {k: r0[k] + r1[k] for k in r0})
    ref_buffers = dict(refs[0].named_buffers())
    for name, b in net.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(ref_buffers[name]) == 1, name
        else:
            parity_gate(b, ref_buffers[name], 1e-4, name)


@pytest.mark.gpu
def test_replicas_take_the_fused_stem_and_keep_their_staging(dev, monkeypatch):
    """Eval under no_grad with stem fusion on the master: both replicas run the fused kernel and match the unwrapped fused
    model bit for bit; the next forward (new replicas, as DataParallel makes on every call) restages nothing and does not
    upload A again."""
    from stgcn_amd import FusedStemOutput, Unit2D, enable_stem_fusion
    from stgcn_amd import functional as F
    net, gen = _make_net(20)
    net = net.to(dev).eval()
    enable_stem_fusion(net.gcn0, net.tcn0)
    ref = copy.deepcopy(net)                          # (its own staging; the pairing travels with the copy)
    x = torch.randn(N, T, V, 3, generator=gen).to(dev)
    halves = [(x[:N // 2],), (x[N // 2:],)]
    kw = ({"stem_only": True},) * 2
    calls = Counter()
    for name in ("stem_forward", "stem_prepare", "tcn_pack"):
        def counted(*a, _f=getattr(F, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(F, name, counted)
    with torch.no_grad():
        want = [ref(h, stem_only=True) for (h,) in halves]
        assert calls["stem_forward"] == 2
        calls.clear()
        first = parallel_apply(_replicas(net, 2), halves, kw, devices=[dev, dev])
    assert calls["stem_forward"] == 2 and calls["stem_prepare"] == 1, dict(calls)
    from stgcn_amd.modules import _store
    slot = _store(net.gcn0).slot(x.device)
    A_dev, st = slot["A_dev"], slot["st"]
    calls.clear()
    with torch.no_grad():
        second = parallel_apply(_replicas(net, 2), halves, kw, devices=[dev, dev])
    assert calls["stem_forward"] == 2 and calls["stem_prepare"] == 0 and calls["tcn_pack"] == 0, dict(calls)
    assert slot["A_dev"] is A_dev and slot["st"] is st
    for out in (first, second):
        for o, w in zip(out, want):
            assert torch.equal(o, w)
    other = Unit2D(128, 128, kernel_size=9).to(dev).eval()
    with torch.no_grad():
        rep = _replicas(net, 2)[1]
        fused = rep.gcn0(halves[0][0].permute(0, 3, 1, 2).contiguous())
        assert isinstance(fused, FusedStemOutput)
        with pytest.raises(RuntimeError, match="ANOTHER Unit2D"):
            other(fused)
        assert torch.equal(rep.tcn0(fused), want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_dataparallel_training_step_as_the_trainer_runs_it(gpus, dev):
    """train_sttran.py:84,89-102,185-191: DataParallel(model).cuda(), a CPU batch into model(data), CrossEntropyLoss,
    zero_grad, backward.  One device is DataParallel's short-circuit; two are the real broadcast and reduce, compared with
    the per-shard gradients of unwrapped copies."""
    if torch.cuda.device_count() < gpus:
        pytest.skip(f"needs {gpus} GPUs")
    net, gen = _make_net(30)
    refs = [copy.deepcopy(net).to(dev).train() for _ in range(gpus)]
    model = torch.nn.DataParallel(net, device_ids=list(range(gpus))).cuda()
    model.train()
    data = torch.randn(N, T, V, 3, generator=gen)
    label = torch.randint(0, CLASSES, (N,), generator=gen)
    criterion = nn.CrossEntropyLoss()
    score = model(data)
    loss = criterion(score, label.cuda())
    model.zero_grad()
    loss.backward()
    for ref, xs, ys in zip(refs, data.chunk(gpus), label.chunk(gpus)):   # DataParallel's scatter: equal chunks on dim 0
        (TF.cross_entropy(ref(xs.to(dev)), ys.to(dev), reduction="sum") / N).backward()
    per = [_grads(r) for r in refs]
    _check_stem_grads(_grads(net), {k: sum(g[k] for g in per) for k in per[0]})
    ref_buffers = dict(refs[0].named_buffers())
    for name, b in net.named_buffers():
        if not name.endswith("num_batches_tracked"):
            parity_gate(b, ref_buffers[name], 1e-4, name)
