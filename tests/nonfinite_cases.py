"""The case table, the planting helpers and the conditions of the non-finite contract: what the HIP paths must do
with an input that holds ONE non-finite value.  Shared by tests/test_nonfinite_host.py (the references make every case
meaningful, no GPU) and tests/test_nonfinite_gpu.py (the HIP paths meet the conditions).  Not a conftest.py: a plain module.

A case plants one value at one position of one input, runs the fp64 restatement the existing tests use for the entry point
(oracle.stgcn_oracle, altformer_ref, altformer_train_ref, st_attention_ref; the torch path in fp64 on the CPU for whole modules)
and the HIP path on the same planted input.  Against the reference OF THE PLANTED INPUT:

  (a) nothing hidden: wherever the reference is non-finite the HIP output is non-finite (NaN and Inf are not told apart) -
      every planted value, every arithmetic, every output (statistics, running buffers, gradients, bf16-stored outputs);
  (b) nothing leaked (planted NaN): wherever the reference is finite the HIP output is finite and passes the entry point's own
      gate there (tests/_util.py::MATH_GATES; the scale is max|ref| over the finite elements) - so the two masks are equal;
  (c) planted +-inf: the split arithmetics turn an Inf operand into NaN (bf16x3: lo = x - hi = inf - inf; bf16 and f16mx
      alike) where the reference's relu(-inf) = 0 is finite, so (b) holds as written for 'f32' and 'f32_valu' only; the other
      modes owe (a) plus (b) on the units the planted element cannot reach in the reference (the other clips / sequences /
      rows).  'f16mx' has no Inf cases: its scales follow the input magnitude (max|x| per clip), so an Inf input is outside
      what the mode defines.

Training with batch statistics owes (a) only: in the reference one NaN reaches everything.

Out of scope: non-finite PARAMETERS (the prepacked blobs and their restaging are a topic of their own) and the
eval-with-gradients backward."""
import functools
import math

import torch
import torch.nn.functional as TF

import altformer_ref as ar
import altformer_train_ref as tr
import entry_points as ep
import st_attention_ref as R
from _util import MATH_GATES
from entry_points import hipF as _F, math_flag as _math

BF16_OUT_GATE = 4e-3          # a bf16-stored output: half an ulp of the stored value on top of the arithmetic (max-norm)
SPLIT_MATHS = ("bf16x3", "bf16", "mixed")     # arithmetics that split or round their operands: an Inf operand becomes NaN


def _nan_all_ones():
    return torch.tensor([-1], dtype=torch.int32).view(torch.float32)[0]


# the canonical NaN; the NaN with an all-ones payload (0xFFFFFFFF, the hostile allocator's fill: a round-to-bf16 done by integer
# addition would wrap it to zero); the infinities
VALUES = {"nan": torch.tensor(float("nan")), "nan_ones": _nan_all_ones(), "+inf": torch.tensor(float("inf")),
          "-inf": torch.tensor(float("-inf"))}
assert VALUES["nan_ones"].view(torch.int32).item() == -1 and bool(torch.isnan(VALUES["nan_ones"]))


def plant(x, index, value):
    """A copy of ``x`` (fp32, CPU) with VALUES[value] - the exact bits - at ``index``."""
    y = x.clone()
    y.view(torch.int32)[tuple(index)] = VALUES[value].view(torch.int32)
    return y


# ---- positions --------------------------------------------------------------------------------------------------------------
def clip_positions(shape, K=9):
    """Where kernels over (N, C, T, V) go wrong: first / last element (clip 0, the last clip), joint V-1 beside the padded
    columns, the first frame of the second 128- and 256-pixel time tile (a frame of one tile that is the halo of its
    neighbour), joints 23 | 24 either side of the wide-frame kernel's split."""
    N, C, T, V = shape
    pos = [("first", (0, 0, 0, 0)), ("last", (N - 1, C - 1, T - 1, V - 1)), ("joint_V-1", (0, C // 2, T // 2, V - 1))]
    for pixels in (128, 256):
        t = max(1, pixels // V)
        if t < T - 1:
            pos.append((f"halo_t{t}", (N - 1, 0, t, V // 2)))
    if V == 46:
        pos += [("joint_23", (0, 0, T // 2, 23)), ("joint_24", (N - 1, C - 1, T // 2, 24))]
    return pos


def token_positions(shape):
    """(B, L, D) inputs of the heads: token 0 (LayerNorm centres on the row's first element), token L-1 (off the 32-key tile
    where L is), features 0 and D-1."""
    B, L, D = shape
    pos = [("first", (0, 0, 0)), ("last", (B - 1, L - 1, D - 1)), ("token_0", (B // 2, 0, D // 2)), ("token_L-1", (B // 2, L - 1, 1)),
           ("feature_0", (B - 1, L // 2, 0)), ("feature_D-1", (0, L // 2, D - 1))]
    return pos


def row_positions(shape):
    M, K = shape
    return [("first", (0, 0)), ("last", (M - 1, K - 1)), ("feature_0", (M // 2, 0)), ("feature_K-1", (M // 2, K - 1))]


# ---- the table --------------------------------------------------------------------------------------------------------------
class Prepared:
    """What ``Case.prepare()`` returns.  ``x``: the clean fp32 CPU input; ``positions``: [(label, index)]; ``reference(x)``:
    {name: fp64 tensor} on the CPU; ``on(dev)``: prepares the HIP side once and returns ``run(x) -> {name: tensor}`` with the
    same names (the shape of an entry_points.Setup).  Every output's axis 0 is the unit axis (clip, sequence or row) unless ``global_outputs`` names it (parameter
    gradients, statistics: no unit); the unit a planted element belongs to is ``index[0]``.  ``gates``: {name: (rel, strict)},
    ``gate`` for the rest."""

    def __init__(self, x, positions, reference, on, gate, gates=None, global_outputs=()):
        self.x, self.positions, self.reference, self.on = x, positions, reference, on
        self.gate, self.gates, self.global_outputs = gate, gates or {}, set(global_outputs)


def shared(setup, positions, gate, *args):
    """A family both contracts cover: the ``prepare`` of tests/entry_points.py's ``setup(*args)``."""
    s = setup(*args)
    return Prepared(s.x, positions(s.x.shape), s.reference, s.on, gate)


class Case:
    """``math``: the arithmetic that decides what a planted Inf owes (c); ``training``: only (a) applies."""

    def __init__(self, id, prepare, math, training=False, kernel=None, without=()):
        self.id, self._prepare, self.math, self.training, self.kernel = id, prepare, math, training, kernel
        self.without = set(without) | ({"+inf", "-inf"} if math == "f16mx" else set())   # (c): f16mx defines no Inf input

    @functools.lru_cache(maxsize=None)
    def prepare(self):
        return self._prepare()

    def plants(self):
        """[(label, index, value)]: every position with the canonical NaN, the other values at the first and the last."""
        pos = self.prepare().positions
        out = [(label, idx, "nan") for label, idx in pos]
        for v in ("nan_ones", "+inf", "-inf"):
            if v in self.without:
                continue
            out += [(label, idx, v) for label, idx in pos if label in ("first", "last")]
        return out

    def owes(self, value):
        """'a' | 'units' | 'full' - see the module docstring."""
        if self.training:
            return "a"
        if value.endswith("inf") and self.math in SPLIT_MATHS:
            return "units"
        return "full"


CASES = []


def add(id, math, prepare, *args, training=False, kernel=None, without=()):
    CASES.append(Case(id, functools.partial(prepare, *args), math, training, kernel, without))


def nonfinite(t):
    return ~torch.isfinite(t.detach().double().cpu())


# ---- the conditions -----------------------------------------------------------------------------------------------------------
def check(case, prep, index, value, out, ref, what):
    """(a) - (c) for one plant; prints each figure before it asserts."""
    owes = case.owes(value)
    for name, r in ref.items():
        o = out[name]
        assert o is not None, f"{what}: output {name} is missing"
        o, r = o.detach().double().cpu().reshape(r.shape), r.detach().double()
        bad_r, bad_o = ~torch.isfinite(r), ~torch.isfinite(o)
        hidden = int((bad_r & ~bad_o).sum())
        print(f"{what} {name}: reference non-finite {int(bad_r.sum())}/{r.numel()}, HIP {int(bad_o.sum())}, hidden {hidden} [{owes}]")
        assert hidden == 0, f"{what} {name}: (a) {hidden} of {int(bad_r.sum())} non-finite reference elements came out finite"
        if owes == "a":
            continue
        if owes == "units":
            if name in prep.global_outputs:
                continue
            keep = torch.ones(r.shape[0], dtype=torch.bool)
            keep[index[0]] = False
            o, r, bad_o, bad_r = o[keep], r[keep], bad_o[keep], bad_r[keep]
        leaked = int((bad_o & ~bad_r).sum())
        assert leaked == 0, f"{what} {name}: (b) {leaked} elements are non-finite where the reference is finite"
        fin = ~bad_r
        if not bool(fin.any()):
            continue
        rel, strict = prep.gates.get(name, prep.gate)
        scale = r[fin].abs().max().item()
        err = (o[fin] - r[fin]).abs().max().item()
        print(f"{what} {name}: on the finite elements max|err| / max|ref| = {err / max(scale, 1e-30):.3e} (gate {rel:g})")
        assert err <= rel * max(scale, 1e-30), f"{what} {name}: (b) max abs err {err:.3e} > {rel:g} * max|ref| ({scale:.3e})"
        if strict:
            assert torch.allclose(o[fin], r[fin], rtol=rel, atol=rel * 0.1 * scale), f"{what} {name}: (b) allclose(rtol={rel}) failed"


def reference_makes_sense(case, prep, index, value, clean, ref, what):
    """The host file's three conditions on one plant."""
    for name, r in clean.items():
        assert bool(torch.isfinite(r).all()), f"{what}: the clean reference's {name} is not finite"
    assert any(bool(nonfinite(r).any()) for r in ref.values()), f"{what}: the planted value reaches no output of the reference"
    if case.owes(value) == "a":
        return
    ok = False
    for name, r in ref.items():
        if name in prep.global_outputs:
            continue
        fin = torch.isfinite(r).reshape(r.shape[0], -1)
        touched = fin[index[0]]
        ok = ok or (bool(touched.any()) and not bool(touched.all())) or bool(fin.all(dim=1).any())
    assert ok, f"{what}: claims (b), but no touched unit keeps a finite element and no unit is wholly finite"


# ---- what the rows take from the shape lists of tests/entry_points.py --------------------------------------------------------------
def two_clips(shape):
    """A shape of the shared lists with a second clip where it has one: (b) across clips needs another clip."""
    return (max(shape[0], 2),) + tuple(shape[1:])


def tcn_case_math(cin, cout, K, stride, T, V, math, along_v):
    """The arithmetic the call runs in (Unit2D's rule sends what the matrix-core kernels do not cover to the VALU kernel)."""
    F = _F()
    mode, kernel = ep._tcn_mode(cin, cout, K, stride, T, V, math, along_v)
    return ("f32_valu" if mode == F.MATH_F32_VALU else math), kernel


# ---- eval forward: the stem -------------------------------------------------------------------------------------------------------
_stem_setup = functools.lru_cache(maxsize=None)(ep.stem)       # one per shape: shared by the arithmetic modes and the two forms
STEM_VARIANTS = [("nctv", "nctv", False), ("nctv", "ntvc", False), ("ntvc", "nctv", False), ("ntvc", "ntvc", True), ("nctv", "nctv", True)]


def prepare_stem_fused(shape, math):
    """The fused kernels through F.stem_forward: (N,3,T,V) and (N,T,V,3) in, (N,C,T,V) and (N,T,V,C) out, fp32 and bf16 stored."""
    s = _stem_setup(*shape)
    tag = lambda i, o, b: f"[{i}->{o},{'bf16' if b else 'f32'}]"       # noqa: E731

    def reference(x):
        r = s.reference(x)
        out = {}
        for v in STEM_VARIANTS:
            out["out" + tag(*v)], out["P" + tag(*v)] = r["out"], r["P"]
        return out

    def on(dev):
        mode = _math(math)
        staged = s.on(dev)
        prep = staged.prepare(mode)

        def run(x):
            out = {}
            for v in STEM_VARIANTS:
                out["out" + tag(*v)], P = staged.forward(x, prep, mode, *v)
                out["P" + tag(*v)] = P.clone()
            return out
        return run
    rel, strict = MATH_GATES[math]
    gates = {}
    for v in STEM_VARIANTS:
        gates["P" + tag(*v)] = MATH_GATES["f32"]
        if v[2]:
            gates["out" + tag(*v)] = (max(rel, BF16_OUT_GATE), False)
    return Prepared(s.x, clip_positions(s.x.shape), reference, on, (rel, strict), gates)


def prepare_stem_two_stage(shape, math):
    """tcn0(gcn0(x)) through the modules without fusion: the graph conv's expansion, then the temporal conv's kernel."""
    s = _stem_setup(*shape)
    gcn, tcn = s.gcn, s.tcn

    def reference(x):
        r = s.reference(x)
        return {"z": r["out"], "P": r["P"], "gcn_out": r["gcn_out"]}

    def on(dev):
        from stgcn_amd import set_math_mode
        gcn.to(dev).eval(), tcn.to(dev).eval()
        set_math_mode(tcn, math)
        assert not getattr(gcn, "_fused_with", None)

        def run(x):
            with torch.no_grad():
                y = gcn(x.to(dev))
                z = tcn(y)
            return {"z": z, "P": gcn.last_attention, "gcn_out": y}
        return run
    return Prepared(s.x, clip_positions(s.x.shape), reference, on, MATH_GATES[math], {"P": MATH_GATES["f32"], "gcn_out": MATH_GATES["f32"]})


# ---- heads, inference ---------------------------------------------------------------------------------------------------------
def _pool_input(S, L, D):
    g = torch.Generator().manual_seed(S + L + D)
    return torch.randn(S, L, D, generator=g) * (0.25 + 3.75 * torch.rand(S, 1, D, generator=g)) + torch.randn(S, 1, 1, generator=g)


def prepare_vit_pool(S, L, D, mode):
    x = _pool_input(S, L, D)

    def reference(x):
        return {"out": x.double().max(dim=1).values if mode == "max" else x.double().mean(dim=1)}

    def on(dev):
        F = _F()
        return lambda x: {"out": F.vit_pool(x.to(dev), mode)}
    return Prepared(x, token_positions(x.shape), reference, on, MATH_GATES["f32"])


def prepare_vit_pool_classify(N, L, D, classes, mode):
    x = _pool_input(N, L, D)
    g = torch.Generator().manual_seed(N + L + D + classes)
    lw, lb = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, b = (torch.rand(classes, D, generator=g) * 2 - 1) / D ** 0.5, torch.randn(classes, generator=g) * 0.5

    def reference(x):
        pooled = x.double().max(dim=1).values if mode == "max" else x.double().mean(dim=1)
        return {"logits": TF.layer_norm(pooled, (D,), lw.double(), lb.double(), 1e-5) @ W.double().T + b.double()}

    def on(dev):
        F = _F()
        lwd, lbd, Wd, bd = (t.to(dev) for t in (lw, lb, W, b))
        return lambda x: {"logits": F.vit_pool_classify(x.to(dev), lwd, lbd, 1e-5, Wd, bd, mode=mode)}
    return Prepared(x, token_positions(x.shape), reference, on, MATH_GATES["f32"])


def _stem_output(N, T, V, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(N, 128, T, V, generator=g))        # the stem ends in a ReLU


def _with_setting(m, setting):
    """'per_block' | 'whole' | 'low_latency' | 'low_latency_split' | 'bf16' on a head or a whole model."""
    import stgcn_amd
    from stgcn_amd.altformer import set_head_math, set_low_latency
    stgcn_amd.set_hip_min_tokens(m, 0)
    if setting == "whole":
        stgcn_amd.set_whole_head(m)
    elif setting.startswith("low_latency"):
        set_low_latency(m, min_tokens=0, split_attention=setting.endswith("split"))
    elif setting == "bf16":
        set_head_math(m, "bf16")
    return m


def prepare_head(cls_name, setting):
    """A small head (tests/entry_points.py::small_head) from the stem output to the logits; the reference is the same
    module's torch path in fp64 on the CPU.  ``setting``: 'per_block' | 'whole' | 'low_latency' | 'low_latency_split' | 'bf16'."""
    import copy
    head = ep.small_head(torch.device("cpu"), cls_name)
    ref_head = copy.deepcopy(head).double()
    z = _stem_output(3, 40, 22)

    def reference(z):
        with torch.no_grad():
            return {"logits": ref_head(z.double())}

    def on(dev):
        h = _with_setting(copy.deepcopy(head).to(dev).eval(), setting)

        def run(z):
            zd = z.to(dev)
            with torch.no_grad():
                assert h.runs_whole(zd) == (setting == "whole")
                return {"logits": h(zd)}
        return run
    return Prepared(z, clip_positions(z.shape), reference, on, MATH_GATES["bf16"] if setting == "bf16" else MATH_GATES["f32"])


def prepare_model(style, setting):
    """ST_GCN_AltFormer, 3 clips at T = 20, one clip poisoned: its logits are non-finite, the others' meet the gate."""
    import copy
    import stgcn_amd
    torch.manual_seed(77)
    model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=20, num_joints=22, style=style, graph="graph.SHRE",
                                       graph_args={"labeling_mode": "spatial"}).eval()
    g = torch.Generator().manual_seed(78)
    with torch.no_grad():
        model.gcn0.PA.data = torch.randn(3, 22, 22, generator=g) * 0.05
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    from oracle import stgcn_oracle as so
    gp = so.agcn_params_from_state(model.gcn0.state_dict(), model.gcn0.A).to(torch.float64)
    tp = so.tcn_params_from_state(model.tcn0.state_dict()).to(torch.float64)
    ref_head = copy.deepcopy(model.modelA if style == "ST" else model.modelB).double()
    x = torch.randn(3, 20, 22, 3, generator=g)           # the loader's (N, T, V, C) batch

    def reference(x):                                    # the stem has no CPU path of its own: the oracle's, then the head's torch path
        with torch.no_grad():
            return {"logits": ref_head(so.stem_forward(x.permute(0, 3, 1, 2).double(), gp, tp))}

    def on(dev):
        m = _with_setting(copy.deepcopy(model).to(dev).eval(), setting)

        def run(x):
            with torch.no_grad():
                return {"logits": m(x.to(dev))}
        return run
    N, T, V, C = x.shape
    pos = [("first", (0, 0, 0, 0)), ("last", (N - 1, T - 1, V - 1, C - 1)), ("middle_clip", (1, T // 2, V - 1, 1))]
    return Prepared(x, pos, reference, on, MATH_GATES["bf16"] if setting == "bf16" else MATH_GATES["f32"])


# ---- training: only (a) ---------------------------------------------------------------------------------------------------------
def prepare_tcn_saved(cin, cout, K, stride, N, T, V, math):
    """stgcn_tcn_forward_train with save=True: the pre-BatchNorm branch z and the saved batch mean / inverse deviation the
    backward reads, and the running buffers it updates in place."""
    from oracle import stgcn_oracle as so
    g = torch.Generator().manual_seed(cin + cout + K + T + V)
    W, b = torch.randn(cout, cin, K, generator=g) * 0.05, torch.randn(cout, generator=g) * 0.1
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    x = torch.randn(N, cin, T, V, generator=g)

    def reference(x):
        z = so.temporal_conv(x.double(), W.double(), b.double(), stride)
        n = z.numel() / cout
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        invstd = torch.rsqrt(var + so.BN_EPS)
        y = torch.relu((z - mean.view(1, -1, 1, 1)) * (invstd * gamma.double()).view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1))
        return {"y": y, "z": z, "save_mean": mean, "save_invstd": invstd, "running_mean": so.BN_MOMENTUM * mean,
                "running_var": (1 - so.BN_MOMENTUM) + so.BN_MOMENTUM * var * (n / (n - 1))}

    def on(dev):
        F = _F()
        Wd, bd, gd, btd = (t.to(dev) for t in (W, b, gamma, beta))

        def run(x):
            rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
            y, z, mean, invstd = F.tcn_forward_train(x.to(dev), Wd, bd, (gd, btd, rm, rv), stride, _math(math), save=True)
            return {"y": y, "z": z, "save_mean": mean, "save_invstd": invstd, "running_mean": rm, "running_var": rv}
        return run
    return Prepared(x, clip_positions(x.shape, K), reference, on, MATH_GATES[math])


def prepare_stem_train(math):
    """loss.backward() through tcn0(gcn0(x)) in .train(), as test_stem_training_step_vs_oracle."""
    from stgcn_amd import set_math_mode
    from oracle import stgcn_oracle as so
    import copy
    gcn, tcn, gp, tp, gen = ep.random_stem(22, None, 1200, ep.CPU)
    set_math_mode(tcn, math)
    gp, tp = gp.to(torch.float64), tp.to(torch.float64)
    leaves = ep.agcn_oracle_leaves(gp)
    tleaves = {"t_w": tp.conv_w, "t_bn_w": tp.bn.weight, "t_bn_b": tp.bn.bias}
    for t in tleaves.values():
        t.requires_grad_(True)
    leaves.update(tleaves)
    names = sorted(leaves)
    x = torch.randn(3, 3, 20, 22, generator=gen)
    G = torch.randn(3, 128, 20, 22, generator=gen)

    def reference(x):
        aux = {}
        zr = so.tcn_forward(so.agcn_forward(x.double(), gp, training=True), tp, training=True, aux=aux)
        grads = torch.autograd.grad((zr * G.double()).sum(), [leaves[k] for k in names])
        return {"z": zr.detach(), **{"d" + k: v for k, v in zip(names, grads)}, "tcn.running_mean": aux["bn"]["running_mean"].detach(),
                "tcn.running_var": aux["bn"]["running_var"].detach()}

    def on(dev):
        gm, tm = gcn.to(dev), tcn.to(dev)

        def run(x):
            g2, t2 = copy.deepcopy(gm).train(), copy.deepcopy(tm).train()
            g2.A = gm.A
            z = t2(g2(x.to(dev)))
            (z * G.to(dev)).sum().backward()
            got = {"d" + k: v for k, v in ep.agcn_module_grads(g2).items()}
            got.update({"dt_w": t2.conv.weight.grad.flatten(1).reshape(128, 128, 9), "dt_bn_w": t2.bn.weight.grad, "dt_bn_b": t2.bn.bias.grad})
            return {"z": z.detach(), **got, "tcn.running_mean": t2.bn.running_mean, "tcn.running_var": t2.bn.running_var}
        return run
    return Prepared(x, clip_positions(x.shape), reference, on, MATH_GATES[math])


def prepare_st_attention_train(N, cin, cout, T, V):
    """gcn_unit_attention's training step without drop-connect, through the module."""
    sd = R.make_state(cin, cout, V, 11)
    x = R.make_input(N, cin, T, V, 12)
    dy = torch.randn(N, cout, T, V, generator=torch.Generator().manual_seed(13))

    def reference(x):
        yr, new, g, dx = R.grads64(sd, x, dy, training=True, mask=None)
        return {"y": yr, "dx": dx, **{"d" + k: v for k, v in g.items()}, **new}

    def on(dev):
        m = ep.st_unit(cin, cout, V, sd, drop_connect=False).train()
        sdd, dyd = {k: v.to(dev) for k, v in sd.items()}, dy.to(dev)     # staged once: nothing in ``run`` comes from the host

        def run(x):
            m.load_state_dict(sdd)                  # the running statistics of the previous plant
            for p in m.parameters():
                p.grad = None
            xg = x.to(dev).requires_grad_(True)
            y = m(xg)
            y.backward(dyd)
            return {"y": y.detach(), "dx": xg.grad, **{"d" + k: p.grad for k, p in m.named_parameters()},
                    **{k: v.clone() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}}
        return run
    return Prepared(x, clip_positions(x.shape), reference, on, MATH_GATES["f32"])


def prepare_vit_block_train(B, L, D, mode, attention_bf16=False):
    """One block's training forward and backward (vit_block_forward_train / vit_block_backward) against autograd through
    altformer_train_ref.block64."""
    heads, hidden = ar.HEADS, 2 * D
    x, sd = ep.block_inputs(B, L, D, hidden)
    dy = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L + D))

    def reference(x):
        y, g = tr.grads64(x, sd, dy, scale=(D // heads) ** -0.5)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def on(dev):
        from stgcn_amd import _capi
        from stgcn_amd.altformer import HEAD_TRAIN_MATH
        F = _F()
        ps = [sd[k].to(dev) for k in tr.PARAMS]
        math = HEAD_TRAIN_MATH[mode] | (_capi.VIT_TRAIN_ATTN_BF16 if attention_bf16 else 0)
        args = (heads, ar.EPS, (D // heads) ** -0.5, math)
        dyd = dy.to(dev)

        def run(x):
            xd = x.to(dev)
            y, saved = F.vit_block_forward_train(xd, ps, *args)
            g = F.vit_block_backward(xd, ps, saved, dyd, *args)
            return {"y": y, "dx": g["x"], **{"d" + k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS)}}
        return run
    return Prepared(x, token_positions(x.shape), reference, on, MATH_GATES["bf16" if mode == "bf16" or attention_bf16 else "f32"])


# ---- the rows of the table ------------------------------------------------------------------------------------------------------
def _build_table():
    F = _F()
    for s in ep.AGCN_SHAPES + [(2, 16, 32, 5, 7)]:      # the last: the only one on agcn_expand_generic_kernel
        s = two_clips(s)
        add("agcn-" + "x".join(map(str, s)), "f32", shared, ep.agcn, clip_positions, MATH_GATES["f32"], *s)
    for ci, co, K, st, T, V, N, m, ob, av in ep.TCN_SHAPES:
        eff, kernel = tcn_case_math(ci, co, K, st, T, V, m, av)
        add(f"tcn-{ci}x{co}x{K}x{st}x{T}x{V}x{N}-{m}" + ("-bf16out" if ob else "") + ("-alongV" if av else ""), eff, shared,
            ep.tcn, clip_positions, (BF16_OUT_GATE, False) if ob else MATH_GATES[m], ci, co, K, st, T, V, N, m, ob, av, kernel=kernel)
    for s in ep.STEM_SHAPES:
        for m in ep.STEM_MATHS:
            if F.stem_supported(3, s[3], s[1], s[2], 9, 3, _math(m)):
                add("stem_fused-" + "x".join(map(str, two_clips(s))) + "-" + m, m, prepare_stem_fused, two_clips(s), m,
                    kernel=ep._stem_kernel(s, m))
    for s in [(3, 37, 22, 128), (2, 9, 46, 128), (2, 30, 64, 128)]:
        for m in ("f32", "bf16x3", "bf16"):
            add("stem_two_stage-" + "x".join(map(str, s)) + "-" + m, m, prepare_stem_two_stage, s, m)
    for o in ("ST", "TS"):
        for lay in ("nctv", "ntvc"):
            add(f"patch_embed-{o}-{lay}", "f32", shared, ep.patch_embed, clip_positions, (1e-4, False), o, lay)
    for s in [(2, 131, 128, 12, 22), (2, 256, 512, 3, 46)]:
        add("st_attention-" + "x".join(map(str, s)), "f32", shared, ep.st_attention, clip_positions, MATH_GATES["f32"], *s)
    for (M, K, Nout), m in [((129, 96, 100), "f32"), ((129, 96, 100), "bf16x3"), ((33, 256, 200), "bf16x3")]:
        add(f"vit_linear-{M}x{K}x{Nout}-{m}", m, shared, ep.vit_linear, row_positions, MATH_GATES[m], M, K, Nout, m)
    for form, B, L, hd in [("resident", 3, 33, 32), ("resident", 3, 65, 64), ("resident", 2, 180, 32), ("stream", 2, 257, 32),
                           ("split", 2, 33, 32), ("split", 2, 180, 64)]:
        add(f"vit_attention-{form}-{B}x{L}-hd{hd}", "f32", shared, ep.vit_attention, token_positions, MATH_GATES["f32"], form, B, L, hd)
    for mode in ("f32", "mixed", "bf16"):
        add(f"vit_block-3x33x256-{mode}", mode, shared, ep.vit_block, token_positions, MATH_GATES["bf16" if mode == "bf16" else "f32"], 3, 33, 256, 8, 512, mode)
    for mode in ("mean", "max"):
        lost = ("-inf",) if mode == "max" else ()      # a maximum over tokens drops one -inf in the reference too: nothing to keep
        for S, L, D in [(3, 33, 256), (2, 180, 64)]:
            add(f"vit_pool-{S}x{L}x{D}-{mode}", "f32", prepare_vit_pool, S, L, D, mode, without=lost)
        add(f"vit_pool_classify-3x65x256x14-{mode}", "f32", prepare_vit_pool_classify, 3, 65, 256, 14, mode, without=lost)
    for cls_name in ("ST", "TS"):
        add(f"head-{cls_name}-whole", "mixed", prepare_head, cls_name, "whole")
    for style in ("ST", "TS"):
        for setting in ("per_block", "whole", "low_latency", "low_latency_split", "bf16"):
            add(f"model-{style}-{setting}", "bf16" if setting == "bf16" else "mixed", prepare_model, style, setting)
    # training: only (a)
    add("agcn_train-moment_form-3x128-3x20x22", "f32", shared, ep.agcn_train, clip_positions, MATH_GATES["f32"], 3, 128, 3, 20, 22, False,
        training=True)
    add("agcn_train-generic-64x64-2x12x22-dx", "f32", shared, ep.agcn_train, clip_positions, MATH_GATES["f32"], 64, 64, 2, 12, 22, True,
        training=True)
    for (ci, co, K, st, N, T, V), m in [((64, 128, 9, 1, 2, 21, 22), "bf16x3"), ((64, 128, 9, 2, 2, 21, 22), "bf16x3"),
                                        ((32, 64, 2, 1, 2, 7, 22), "bf16x3"), ((32, 64, 9, 1, 2, 7, 22), "f32_valu")]:
        add(f"tcn_train-{ci}x{co}x{K}x{st}x{N}x{T}x{V}-{m}", m, shared, ep.tcn_train, clip_positions, MATH_GATES[m], ci, co, K, st, N, T, V, m,
            training=True)
    for m in ("bf16x3", "f32_valu"):
        add(f"tcn_saved-64x128x9x1x2x21x22-{m}", m, prepare_tcn_saved, 64, 128, 9, 1, 2, 21, 22, m, training=True)
    add("stem_train-bf16x3", "bf16x3", prepare_stem_train, "bf16x3", training=True)
    add("st_attention_train-2x131x128x12x22", "f32", prepare_st_attention_train, 2, 131, 128, 12, 22, training=True)
    for mode in ("f32", "bf16x3", "bf16"):
        add(f"vit_block_train-3x33x256-{mode}", mode, prepare_vit_block_train, 3, 33, 256, mode, training=True)
    add("vit_block_train-3x33x256-f32-attention_bf16", "f32", prepare_vit_block_train, 3, 33, 256, "f32", True, training=True)
    add("vit_block_train-2x257x256-f32-streaming", "f32", prepare_vit_block_train, 2, 257, 256, "f32", training=True)


_build_table()
assert len({c.id for c in CASES}) == len(CASES)
