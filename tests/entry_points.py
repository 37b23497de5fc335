"""How the tests set up the HIP entry points: seeded modules, inputs and fp64 restatements, in one place.  The case tables of
the library-wide contracts - buffer discipline (tests/test_buffer_discipline_gpu.py), non-finite inputs
(tests/nonfinite_cases.py) and streams (tests/stream_order.py) - build their rows from the setups below, the other test files
borrow the helpers.  A plain module:
it imports no test module, and needs a GPU only where a function takes a device.

A ``Setup`` is made on the CPU from seeds: ``x`` is the clean fp32 input, ``reference(x)`` the fp64 restatement the entry
point's own tests use, {name: tensor}; ``on(dev)`` stages the device side once and returns ``run(x)`` with the same names
(``x`` on either side: an upload of a tensor that is on the device already is no copy).  What only one contract needs - positions
and planted values, gates, bit-equality between outputs - stays in that contract's file."""
import copy
import types

import torch
import torch.nn.functional as TF

import altformer_ref as ar
import altformer_train_ref as tr
import st_attention_ref as R
from _util import kink_free_cotangent

CPU = torch.device("cpu")
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


class Setup:
    def __init__(self, x, reference, on, **more):
        self.x, self.reference, self.on = x, reference, on
        self.__dict__.update(more)


def hipF():
    from stgcn_amd import functional as F
    return F


def math_flag(name):
    F = hipF()
    return {"f32": F.MATH_F32, "bf16x3": F.MATH_BF16X3, "bf16": F.MATH_BF16, "f32_valu": F.MATH_F32_VALU, "f16mx": F.MATH_F16MX}[name]


# ---- the graph conv and the stem ------------------------------------------------------------------------------------------------
AGCN_SHAPES = [(2, 3, 64, 9, 25), (1, 64, 64, 7, 22), (1, 3, 128, 30, 64)]       # (N, Cin, Cout, T, V); the second: identity residual


def random_stem(V, graph, seed, dev, cin=3, c=128):
    """A seeded unit_agcn + Unit2D pair in eval mode on ``dev``, their oracle parameters and the generator, for shapes the fixtures
    do not hold (ragged tiles, odd V)."""
    from stgcn_amd import Unit2D, unit_agcn
    from oracle import stgcn_oracle as so
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    A = torch.rand(3, V, V, generator=gen) * (torch.rand(3, V, V, generator=gen) < 0.15) if graph is None else graph
    gcn = unit_agcn(cin, c, A.clone())
    tcn = Unit2D(c, c, kernel_size=9)
    with torch.no_grad():
        gcn.PA.data = torch.randn(3, V, V, generator=gen) * 0.05
        for m in list(gcn.modules()) + list(tcn.modules()):
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.2)
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 1.5 + 0.25)
            if isinstance(m, torch.nn.Conv2d):
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
        for cv in list(gcn.conv_a) + list(gcn.conv_b):
            cv.weight.mul_(3.0)
    gcn.A = A.clone()
    gp = so.agcn_params_from_state(gcn.state_dict(), gcn.A)
    tp = so.tcn_params_from_state(tcn.state_dict())
    return gcn.to(dev).eval(), tcn.to(dev).eval(), gp, tp, gen


def agcn(N, cin, cout, T, V):
    """F.agcn_forward and F.agcn_attention on a seeded unit_agcn."""
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = random_stem(V, None, 3000 + cin + cout + T + V, CPU, cin=cin, c=cout)
    gp = gp.to(torch.float64)
    x = torch.randn(N, cin, T, V, generator=gen)

    def reference(x):
        aux = {}
        y = so.agcn_forward(x.double(), gp, aux=aux)
        return {"y": y, "P": aux["P"], "P_attention": aux["P"]}

    def on(dev):
        F = hipF()
        gcn.to(dev).eval()
        st = gcn._staged(dev)
        gcn._folded(st)

        def run(x):
            xd = x.to(dev)
            y, P = F.agcn_forward(xd, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"], st["bdown"],
                                  st["bn_scale"], st["bn_shift"], st["down_scale"], st["down_shift"])
            return {"y": y, "P": P, "P_attention": F.agcn_attention(xd, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"])}
        return run
    return Setup(x, reference, on, module=gcn)


# (N, T, V, C).  (1, 30, 64) is in the list of the ragged test, where the modules fall back to two stages: no fused kernel covers
# 64 joints, so stem_supported leaves it out here.  (2, 2, 52) is test_stem_layout_fusion_is_bit_exact's shape for the 128-pixel
# kernel (stem_mfma_bf16_kernel), which no other shape of the list reaches.
STEM_SHAPES = [(3, 37, 22, 128), (2, 9, 46, 128), (1, 1, 22, 128), (2, 23, 7, 128), (1, 30, 64, 128), (17, 20, 22, 128), (3, 40, 22, 256),
               (2, 2, 52, 128)]
STEM_MATHS = ("f32", "bf16x3", "bf16", "f16mx")
STEM_KERNELS = {"stem_mfma_f32_kernel", "stem_mfma_bf16_kernel", "stem_bf16_v4_kernel", "stem_bf16_v6_kernel", "stem_f16mx_kernel"}


def _stem_kernel(shape, math):
    from stgcn_amd import _capi
    F = hipF()
    N, T, V, C = shape
    return _capi.lib().stgcn_stem_kernel_name(3, C, T, V, 9, 3, F._flags(math_flag(math), False)).decode()


def stem(N, T, V, C):
    """The stem of one shape, shared by the arithmetic modes: ``gcn`` / ``tcn`` are the modules, ``reference(x)`` the oracle's
    {"out", "P", "gcn_out"}.  ``on(dev)`` stages both modules and returns what the fused entry points take: ``st`` / ``ts`` (the
    staged parameters), ``prepare(mode)`` (F.stem_prepare's blob) and ``forward(x, prep, mode, in_layout, out_layout, bf16)``
    (F.stem_forward from (N,3,T,V) or (N,T,V,3) memory to (N,C,T,V) or (N,T,V,C), fp32 or bf16 stored) -> (out, P)."""
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = random_stem(V, None, 100 + T + V, CPU, c=C)
    gp, tp = gp.to(torch.float64), tp.to(torch.float64)
    x = torch.randn(N, 3, T, V, generator=gen)

    def reference(x):
        aux = {}
        ref = so.stem_forward(x.double(), gp, tp, aux=aux)
        return {"out": ref, "P": aux["gcn"]["P"], "gcn_out": aux["gcn_out"]}

    def on(dev):
        F = hipF()
        gcn.to(dev).eval(), tcn.to(dev).eval()
        st, ts = gcn._staged(dev), tcn._staged(dev)
        gcn._folded(st)

        def prepare(mode):
            return F.stem_prepare(st["Wd"], st["bd"], st["Wdown"], st["bdown"], st["bn_scale"], st["bn_shift"], st["down_scale"],
                                  st["down_shift"], ts["W"], ts["scale"], mode)

        def forward(x, prep, mode, in_layout="nctv", out_layout="nctv", bf16=False):
            xd = x.to(dev)
            if in_layout == "ntvc":
                xd = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            return F.stem_forward(xd, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], prep, ts["shift"], C, 9, mode, bf16,
                                  channels_last_out=out_layout == "ntvc")
        return types.SimpleNamespace(st=st, ts=ts, prepare=prepare, forward=forward)
    return Setup(x, reference, on, gcn=gcn, tcn=tcn)


def agcn_oracle_leaves(gp):
    leaves = {"PA": gp.PA, "bn_w": gp.bn.weight, "bn_b": gp.bn.bias}
    if gp.down_w is not None:
        leaves.update({"down_w": gp.down_w, "down_b": gp.down_b, "dbn_w": gp.down_bn.weight, "dbn_b": gp.down_bn.bias})
    for i in range(gp.num_subset):
        leaves.update({f"a_w{i}": gp.conv_a_w[i], f"a_b{i}": gp.conv_a_b[i], f"b_w{i}": gp.conv_b_w[i],
                       f"b_b{i}": gp.conv_b_b[i], f"d_w{i}": gp.conv_d_w[i], f"d_b{i}": gp.conv_d_b[i]})
    for t in leaves.values():
        t.requires_grad_(True)
    return leaves


def agcn_module_grads(gcn):
    g = {"PA": gcn.PA.grad, "bn_w": gcn.bn.weight.grad, "bn_b": gcn.bn.bias.grad}
    if gcn._has_down():
        g.update({"down_w": gcn.down[0].weight.grad.flatten(1), "down_b": gcn.down[0].bias.grad,
                  "dbn_w": gcn.down[1].weight.grad, "dbn_b": gcn.down[1].bias.grad})
    for i in range(gcn.num_subset):
        g.update({f"a_w{i}": gcn.conv_a[i].weight.grad.flatten(1), f"a_b{i}": gcn.conv_a[i].bias.grad,
                  f"b_w{i}": gcn.conv_b[i].weight.grad.flatten(1), f"b_b{i}": gcn.conv_b[i].bias.grad,
                  f"d_w{i}": gcn.conv_d[i].weight.grad.flatten(1), f"d_b{i}": gcn.conv_d[i].bias.grad})
    return g


def agcn_compare_grads(got, ref, rel):
    """Every gradient within rel*max|ref| of its tensor.  Three bias gradients are structurally zero — conv_a's (a bias
    on `a` shifts every column of the Gram matrix by a constant, which soft-max over that column ignores), conv_d's
    and down's (a bias in front of a batch-statistics BatchNorm): both sides are rounding noise there, so those are
    held against the scale of the matching weight gradient instead."""
    bad = []
    for k in sorted(ref):
        g, r = got[k].reshape(ref[k].shape).double().cpu(), ref[k].double().cpu()
        assert torch.isfinite(g).all(), f"d{k}: non-finite gradient"
        scale = r.abs().max().item()
        if k.startswith("a_b") or k.startswith("d_b"):       # (d_b, down_b: a bias in front of a batch-statistics
            scale = max(scale, ref[k[0] + "_w" + k[3:]].abs().max().item())   # BatchNorm has zero gradient as well)
        if k == "down_b":
            scale = max(scale, ref["down_w"].abs().max().item())
        err = (g - r).abs().max().item()
        if err > rel * max(scale, 1e-30):
            bad.append(f"d{k}: err {err:.3e} vs {rel:g}*{scale:.3e}")
    assert not bad, "; ".join(bad)


def agcn_train(cin, cout, N, T, V, want_dx, kink_free=False, frozen=False):
    """unit_agcn's training step through the module (autograd.Function -> agcn_forward_train -> agcn_backward_train), as
    test_unit_agcn_backward_vs_oracle (the moment form of the stem class), test_unit_agcn_generic_backward_vs_oracle and, with
    ``frozen`` statistics, test_eval_mode_backward_unit_agcn_vs_oracle; ``leaves`` names the parameter gradients "d" + leaf.
    ``kink_free``: the cotangent is _util.kink_free_cotangent of the first ``reference(x)`` - the clean input's.  ``on(dev, fresh)``:
    every run steps a fresh copy of the module and reports its running buffers after the step, or (``fresh=False``) the module
    itself with its gradients cleared; ``tile``: the cotangent repeated that often along the clips, for a tiled batch
    (tests/large_extent.py).  ``module`` / ``cotangent`` ([G], filled by the first ``reference``): for callers that step the
    module themselves."""
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = random_stem(V, None, 2000 + cin + cout + T + V, CPU, cin=cin, c=cout)
    gp = gp.to(torch.float64)
    leaves = agcn_oracle_leaves(gp)
    names = sorted(leaves)
    x = torch.randn(N, cin, T, V, generator=gen)
    G = [None if kink_free else torch.randn(N, cout, T, V, generator=gen)]

    def reference(x):
        xr = x.double().requires_grad_(True)
        aux = {}
        yr = so.agcn_forward(xr, gp, training=not frozen, aux=aux)
        if G[0] is None:
            G[0] = kink_free_cotangent(yr, gen)
        grads = torch.autograd.grad((yr * G[0].double()).sum(), [leaves[k] for k in names] + [xr])
        out = {"y": yr.detach(), "P": aux["P"].detach(), **{"d" + k: v for k, v in zip(names, grads[:-1])}}
        if not frozen:
            out["bn.running_mean"], out["bn.running_var"] = (aux["bn"][k].detach() for k in ("running_mean", "running_var"))
            if cin != cout:
                out["down.running_mean"], out["down.running_var"] = (aux["down_bn"][k].detach() for k in ("running_mean", "running_var"))
        if want_dx:
            out["dx"] = grads[-1]
        return out

    def on(dev, fresh=True, tile=1):
        master = gcn.to(dev).train(not frozen)
        Gd = G[0].to(dev).repeat(tile, 1, 1, 1)

        def run(x):
            m = master
            if fresh:
                m = copy.deepcopy(master)
                m.A = master.A
            for p in m.parameters():
                p.grad = None
            xg = x.to(dev).requires_grad_(want_dx)
            y = m(xg)
            (y * Gd).sum().backward()
            out = {"y": y.detach(), "P": m.last_attention, **{"d" + k: v for k, v in agcn_module_grads(m).items()}}
            if fresh:
                out["bn.running_mean"], out["bn.running_var"] = m.bn.running_mean, m.bn.running_var
                if cin != cout:
                    out["down.running_mean"], out["down.running_var"] = m.down[1].running_mean, m.down[1].running_var
            if want_dx:
                out["dx"] = xg.grad
            return out
        return run
    return Setup(x, reference, on, leaves=names, module=gcn, cotangent=G)


# ---- the temporal conv ----------------------------------------------------------------------------------------------------------
# (Cin, Cout, K, stride, T, V, N, math, bf16 output, along V).  The last frame-axis shape is not in the five of the ragged test: it is
# the smallest one the eight-wave kernel (tcn_bf16_v4_kernel) serves, so that all six kernels occur (test_tcn_cases_...).
TCN_SHAPES = [(ci, co, K, s, T, V, 2, m, False, False)
              for ci, co, K, s, T, V in [(128, 128, 9, 1, 41, 22), (32, 128, 9, 1, 23, 22), (64, 128, 9, 2, 40, 22), (48, 96, 9, 1, 20, 22),
                                         (128, 128, 4, 1, 19, 22)] for m in ("f32", "bf16x3", "bf16")]
TCN_SHAPES += [(3, 70, 9, 1, 7, 46, 3, "f32_valu", False, False),
               (16, 16, 5, 2, 5, 25, 2, "f32_valu", False, True),
               (64, 64, 9, 1, 33, 25, 5, "bf16x3", True, False), (128, 256, 9, 1, 70, 25, 6, "bf16x3", True, False),   # odd T*V, half-size y
               (16, 128, 9, 1, 40, 7, 2, "bf16x3", False, False)]
TCN_KERNELS = {"tcn_valu_kernel", "tcn_valu_joint_axis_kernel", "tcn_mfma_f32_kernel", "tcn_mfma_bf16_kernel", "tcn_bf16_v4_kernel",
               "tcn_bf16_v6_kernel"}


def _tcn_mode(cin, cout, K, stride, T, V, math, along_v):
    """The arithmetic the call runs in (Unit2D's rule: what the matrix-core kernels do not cover goes to the VALU kernel) and the
    kernel the library names for it."""
    from stgcn_amd import _capi
    F = hipF()
    mode = math_flag(math)
    if not along_v and math != "f32_valu" and not F.tcn_supported(cin, cout, T, V, K, stride, mode):
        mode = F.MATH_F32_VALU
    fl = F._flags(mode, False) | (_capi.CONV_ALONG_V if along_v else 0)
    return mode, _capi.lib().stgcn_tcn_kernel_name(cin, cout, T, V, K, stride, fl).decode()


def tcn(cin, cout, K, stride, T, V, N, math, out_bf16, along_v):
    """F.tcn_forward_packed and (along the frame axis) the one-shot F.tcn_forward on a seeded Unit2D; every output has the dtype
    asked for.  ``on(dev, pack_every_run)``: the weights are packed once, or by every run (F.tcn_pack allocates too)."""
    from stgcn_amd import Unit2D
    from oracle import stgcn_oracle as so
    gen = torch.Generator().manual_seed(cin + cout + K + T)
    torch.manual_seed(5)
    m = Unit2D(cin, cout, kernel_size=K, stride=stride, dim=3 if along_v else 2)
    with torch.no_grad():
        m.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
        m.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        m.bn.running_mean.copy_(torch.randn(cout, generator=gen) * 0.3)
        m.bn.running_var.copy_(torch.rand(cout, generator=gen) + 0.25)
    x = torch.randn(N, cin, T, V, generator=gen)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    if along_v:                                                    # test_unit2d_dim3: the same op on the (T,V)-transposed tensor
        sd["conv.weight"] = sd["conv.weight"].permute(0, 1, 3, 2)
    tp = so.tcn_params_from_state(sd, stride=stride).to(torch.float64)

    def reference(x):
        y = so.tcn_forward(x.double().transpose(2, 3), tp).transpose(2, 3) if along_v else so.tcn_forward(x.double(), tp)
        return {"y_packed": y} if along_v else {"y_packed": y, "y_one_shot": y}

    def on(dev, pack_every_run=False):
        F = hipF()
        st = m.to(dev).eval()._staged(dev)
        mode, _ = _tcn_mode(cin, cout, K, stride, T, V, math, along_v)
        pack = lambda: F.tcn_pack(st["W"], st["scale"], mode)       # noqa: E731
        Wp = None if pack_every_run else pack()

        def run(x):
            xd = x.to(dev)
            out = {"y_packed": F.tcn_forward_packed(xd, Wp if Wp is not None else pack(), st["shift"], cout, K, stride, mode, out_bf16,
                                                    along_v=along_v)}
            if not along_v:
                out["y_one_shot"] = F.tcn_forward(xd, st["W"], st["scale"], st["shift"], stride, mode, out_bf16)
            assert all(y.dtype == (torch.bfloat16 if out_bf16 else torch.float32) for y in out.values())
            return out
        return run
    return Setup(x, reference, on)


def tcn_train(cin, cout, K, stride, N, T, V, math, bias=True, kink_free=False):
    """Unit2D's training step through the module (tcn_forward_train -> tcn_backward_train), as test_unit2d_backward_vs_oracle.
    ``kink_free`` and ``on(dev, fresh)``: as agcn_train's.  ``module`` / ``cotangent`` ([G], filled by the first ``reference``):
    for callers of the functional pair."""
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    torch.manual_seed(900 + cin + K + V)
    gen = torch.Generator().manual_seed(901 + cin + K + V)
    master = Unit2D(cin, cout, kernel_size=K, stride=stride, bias=bias)
    with torch.no_grad():
        master.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        master.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        if bias:
            master.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
    set_math_mode(master, math)
    tp = so.tcn_params_from_state(master.state_dict(), stride=stride).to(torch.float64)
    leaves = [tp.conv_w, tp.bn.weight, tp.bn.bias]
    for t in leaves:
        t.requires_grad_(True)
    x = torch.randn(N, cin, T, V, generator=gen)
    G = [None if kink_free else torch.randn(N, cout, hipF().tcn_out_frames(T, K, stride), V, generator=gen)]

    def reference(x):
        xr = x.double().requires_grad_(True)
        aux = {}
        yr = so.tcn_forward(xr, tp, training=True, aux=aux)
        if G[0] is None:
            G[0] = kink_free_cotangent(yr, gen)
        g = torch.autograd.grad((yr * G[0].double()).sum(), leaves + [xr])
        return {"y": yr.detach(), "dW": g[0], "dgamma": g[1], "dbeta": g[2], "dx": g[3],
                "running_mean": aux["bn"]["running_mean"].detach(), "running_var": aux["bn"]["running_var"].detach()}

    def on(dev, fresh=True):
        master.to(dev).train()
        Gd = G[0].to(dev)

        def run(x):
            m = copy.deepcopy(master) if fresh else master
            for p in m.parameters():
                p.grad = None
            xd = x.to(dev).requires_grad_(True)
            y = m(xd)
            (y * Gd).sum().backward()
            out = {"y": y.detach(), "dW": m.conv.weight.grad.reshape(cout, cin, K), "dgamma": m.bn.weight.grad, "dbeta": m.bn.bias.grad,
                   "dx": xd.grad}
            if fresh:
                out["running_mean"], out["running_var"] = m.bn.running_mean, m.bn.running_var
            if bias:
                out["dbias"] = m.conv.bias.grad
            return out
        return run
    return Setup(x, reference, on, module=master, cotangent=G)


# ---- patch embedding, ST-TR's spatial attention unit ----------------------------------------------------------------------------
def patch_embed(order, layout, N=2, C=128, T=9, V=25, E=256):
    """F.patch_embed with and without the positional embedding, from (N,C,T,V) or channels-last memory; outputs as (N, -1, L, E):
    axis 0 is the clip."""
    g = torch.Generator().manual_seed(61 + (order == "TS"))
    z = torch.randn(N, C, T, V, generator=g)
    W, b = torch.randn(E, C, generator=g) / C ** 0.5, torch.randn(E, generator=g) * 0.1
    pos = torch.randn(1, T if order == "TS" else V, E, generator=g) * 0.05
    L = V if order == "ST" else T

    def reference(z):
        tok = z.permute(0, 2, 3, 1).reshape(N * T, V, C) if order == "ST" else z.permute(0, 3, 2, 1).reshape(N * V, T, C)
        e = tok.double() @ W.double().T + b.double()
        return {"e": (e + pos.double()).reshape(N, -1, L, E), "e_no_pos": e.reshape(N, -1, L, E)}

    def on(dev):
        F = hipF()
        Wd, bd, pd = W.to(dev), b.to(dev), pos.to(dev)

        def run(z):
            zd = z.to(dev)
            if layout == "ntvc":
                zd = zd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            return {"e": F.patch_embed(zd, Wd, bd, pd, order=order).reshape(len(zd), -1, L, E),
                    "e_no_pos": F.patch_embed(zd, Wd, bd, None, order=order).reshape(len(zd), -1, L, E)}
        return run
    return Setup(z, reference, on)


def incidence(V):
    g = torch.Generator().manual_seed(V)
    return (torch.rand(3, V, V, generator=g) > 0.8).float()


def st_unit(cin, cout, V, sd=None, drop_connect=True):
    """gcn_unit_attention in the reference scripts' configuration, on the GPU."""
    from stgcn_amd import gcn_unit_attention
    m = gcn_unit_attention(cin, cout, incidence(V), **R.unit_kwargs(V, drop_connect))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def st_attention(N, cin, cout, T, V):
    """gcn_unit_attention's eval forward through the module."""
    sd = R.make_state(cin, cout, V, 7)
    x = R.make_input(N, cin, T, V, 8)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}

    def reference(x):
        return {"y": R.forward64(sd64, x.double(), False)[0]}

    def on(dev):
        m = st_unit(cin, cout, V, sd).eval()
        m._folded(m._staged(dev))

        def run(x):
            with torch.no_grad():
                return {"y": m(x.to(dev))}
        return run
    return Setup(x, reference, on)


# ---- the AltFormer heads --------------------------------------------------------------------------------------------------------
TILE_FORMS = {(128, 128): 0, (64, 64): 0x20000, (32, 64): 0x30000}
# The criterion each arithmetic of the training path holds on every gradient of every block case (DESIGN §15 has the
# measured table): True = both criteria of parity_gate, False = the max-norm criterion only.
TRAIN_STRICT = {"f32": True, "mixed": True, "bf16x3": False}


def vit_linear(M, K, Nout, math):
    """F.vit_linear in every tile form: "on" + tile with LayerNorm, bias, GELU and residual, "off" + tile the bare product.
    ``W``, ``b``, ``R``, ``ln``: the CPU operands, for callers that choose the epilogue themselves."""
    g = torch.Generator().manual_seed(M + K + Nout)
    x = torch.randn(M, K, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    W = (torch.rand(Nout, K, generator=g) * 2 - 1) / K ** 0.5
    b = torch.randn(Nout, generator=g) * 0.5
    Rr = torch.randn(M, Nout, generator=g)
    lw, lb = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)

    def reference(x):
        xn = ar.layer_norm64(x.double(), lw.double(), lb.double())
        on, off = TF.gelu(xn @ W.double().T + b.double()) + Rr.double(), x.double() @ W.double().T
        return {f"{k}{tile}": v for tile in TILE_FORMS for k, v in (("on", on), ("off", off))}

    def on(dev):
        F = hipF()
        mode = math_flag(math)
        Wd, bd, Rd, lwd, lbd = (t.to(dev) for t in (W, b, Rr, lw, lb))

        def run(x):
            xd, out = x.to(dev), {}
            for tile, fl in TILE_FORMS.items():
                assert F.vit_linear_tile(M, K, Nout, mode | fl) == tile
                out[f"on{tile}"] = F.vit_linear(xd, Wd, bd, ln=(lwd, lbd, ar.EPS), residual=Rd, gelu=True, math=mode | fl)
                out[f"off{tile}"] = F.vit_linear(xd, Wd, None, math=mode | fl)
            return out
        return run
    return Setup(x, reference, on, W=W, b=b, R=Rr, ln=(lw, lb))


def peaked_qkv(B, L, heads, hd, seed, amp=2.3):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 3, heads, hd, generator=g)
    qkv[:, :, :2] *= amp                         # scores ~ N(0, amp^4): with 2.3 they reach about +-28 at head_dim ** -0.5
    return qkv.reshape(B, L, 3 * heads * hd)


def attention_grad64(qkv, dout, heads, scale):
    """(out, dqkv) by fp64 autograd of the restated attention, where the tensors are."""
    q = qkv.double().requires_grad_(True)
    out = ar.attention64(q, heads, scale)
    out.backward(dout.double())
    return out.detach(), q.grad


def vit_attention(form, B, L, hd):
    """One attention entry point ('resident' | 'stream' | 'split') on peaked scores, 8 heads."""
    heads = 8
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd)

    def reference(qkv):
        return {"out": ar.attention64(qkv, heads, hd ** -0.5)}

    def on(dev):
        F = hipF()
        entry = {"resident": F.vit_attention, "stream": F.vit_attention_stream, "split": F.vit_attention_split}[form]
        if form == "stream":
            assert F.vit_attention_stream_supported(L, heads, hd)
        if form == "split":
            assert F.vit_attention_split_supported(L, heads, hd)
        return lambda qkv: {"out": entry(qkv.to(dev), heads)}
    return Setup(qkv, reference, on)


def block_inputs(B, L, D, hidden):
    sd = ar.random_block_state(D, hidden, True, seed=B + L + D)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    return x, sd


def block_params(sd, dev):
    sdd = {k: v.to(dev) for k, v in sd.items()}
    pair = lambda n: (sdd[n + ".weight"], sdd[n + ".bias"])       # noqa: E731
    return (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))


def vit_block(B, L, D, heads, hidden, mode):
    """F.vit_block_forward in a HEAD_MATH mode; ``run(x, flags)`` ors ``flags`` into the math word.  ``reference(x)`` restates the
    block where ``x`` is (on the device for inputs the CPU would take tens of seconds over) and returns it on the CPU."""
    x, sd = block_inputs(B, L, D, hidden)

    def reference(x):
        return {"y": ar.block64(x, {k: v.to(x.device) for k, v in sd.items()}, heads=heads)[0].cpu()}

    def on(dev):
        from stgcn_amd.altformer import HEAD_MATH
        F = hipF()
        params = block_params(sd, dev)
        return lambda x, flags=0: {"y": F.vit_block_forward(x.to(dev), *params, heads, ar.EPS, (D // heads) ** -0.5, HEAD_MATH[mode] | flags)}
    return Setup(x, reference, on)


def run_block(blk, x, dy, mode, s1=None, s2=None):
    """A Block's training step through the functional pair -> (y, {"x" and tr.PARAMS: gradient})."""
    from stgcn_amd.altformer import HEAD_MATH
    F = hipF()
    ps = [None if p is None else p.detach() for p in blk._weights()]
    args = (blk.attn.num_heads, blk.norm1.eps, blk.attn.scale, HEAD_MATH[mode], s1, s2)
    y, saved = F.vit_block_forward_train(x, ps, *args)
    g = F.vit_block_backward(x, ps, saved, dy, *args)
    return y, {"x": g["x"], **{k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS)}}


def small_head(dev, cls_name="ST", **kw):
    from stgcn_amd import altformer
    from stgcn_amd.altformer import set_hip_min_tokens
    torch.manual_seed(11)
    cfg = dict(num_frame=40, num_joints=22, in_chans=128, embed_dim_ratio=256, depth=2, num_heads=8, mlp_ratio=2.,
               qkv_bias=True, drop_path_rate=0.1)
    cfg.update(kw)
    head = getattr(altformer, cls_name)(14, **cfg)
    with torch.no_grad():
        for n, p in head.named_parameters():
            if n.endswith("pos_embed"):
                p.copy_(0.05 * torch.randn(p.shape))
    set_hip_min_tokens(head, 0)
    return head.to(dev).eval()


# ---- entry points the non-finite table predates (the stream contract's rows, tests/stream_order.py) -----------------------------
# Backward entry points take their cotangent as ``x`` where every output is linear in it: a stale cotangent then moves them all.
def vit_patch_embed(name, layout, math):
    """F.vit_patch_embed on an embedding case of stvit_ref, from (N,C,T,V) or channels-last memory."""
    import stvit_ref as sr
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    z, W, bias, cls, pos = sr.embed_case(name)

    def reference(z):
        return {"x": sr.embed64(z.double(), W, bias, cls, pos, p1, p2)}

    def on(dev):
        F = hipF()
        Wd, bd, cd, pd = (t.to(dev) for t in (W, bias, cls, pos))

        def run(z):
            zd = z.to(dev)
            if layout == "ntvc":
                zd = zd.contiguous(memory_format=torch.channels_last)
            assert F._is_channels_last(zd) == (layout == "ntvc")
            return {"x": F.vit_patch_embed(zd, Wd, bd, cd, pd, p1, p2, math_flag(math))}
        return run
    return Setup(z, reference, on)


def vit_patch_embed_backward(name, layout, math):
    """F.vit_patch_embed_backward on an embedding case; ``x`` is dx, the gradient of the embedding's output."""
    import stvit_ends_ref as er
    import stvit_ref as sr
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    z, W, bias, cls, pos = sr.embed_case(name)

    def reference(dx):
        return er.embed_grads64(z, W, bias, cls, pos, p1, p2, dx)

    def on(dev):
        F = hipF()
        zd, Wd = z.to(dev), W.to(dev)
        if layout == "ntvc":
            zd = zd.contiguous(memory_format=torch.channels_last)
        return lambda dx: F.vit_patch_embed_backward(zd, Wd, dx.to(dev), p1, p2, math_flag(math))
    return Setup(er.make_dx(name), reference, on)


def vit_pool_classify_backward(name, mode):
    """F.vit_pool_classify_backward on a classifier case of stvit_ends_ref ('cls' | 'mean')."""
    import stvit_ends_ref as er
    import stvit_ref as sr
    x, ln_w, ln_b, W, bias, dlogits = er.classify_case(name)

    def reference(x):
        return er.classify_grads64(x, ln_w, ln_b, W, bias, dlogits, mode)[1]

    def on(dev):
        F = hipF()
        lw, lb, Wd, dl = (t.to(dev) for t in (ln_w, ln_b, W, dlogits))
        return lambda x: F.vit_pool_classify_backward(x.to(dev), lw, lb, sr.LN_EPS, Wd, dl, mode=mode)
    return Setup(x, reference, on)


def vit_block_train_drop(name, mode):
    """The dropout pair (vit_block_forward_train / vit_block_backward with ``drop``) on a layer case of stvit_train_ref."""
    import stvit_train_ref as vr
    B, L, D, heads, hidden = vr.CASES[name]
    x, dy, sd, masks = vr.make_case(name)
    scale = (D // heads) ** -0.5

    def reference(x):
        y, g = vr.grads64(x, sd, dy, masks, None, None, heads, scale)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def on(dev):
        from stgcn_amd.altformer import HEAD_TRAIN_MATH
        F = hipF()
        ps = [None if sd.get(k) is None else sd[k].to(dev) for k in tr.PARAMS]
        md, dyd = tuple(m.to(dev) for m in masks), dy.to(dev)
        args = (heads, 1e-5, scale, HEAD_TRAIN_MATH[mode], None, None)

        def run(x):
            xd = x.to(dev)
            y, saved = F.vit_block_forward_train(xd, ps, *args, drop=md)
            g = F.vit_block_backward(xd, ps, saved, dyd, *args, drop=md)
            return {"y": y, "dx": g["x"], **{"d" + k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS) if g[n] is not None}}
        return run
    return Setup(x, reference, on)


def vit_block_train_small(B, L, D, mode):
    """The ``_drop`` pair under VIT_WGRAD_SMALL | VIT_TILE_AUTO with stochastic-depth factors and no masks
    (test_row_factors_with_a_dropped_sequence); ``plans(F)``: the weight-gradient plans of the D x D and the qkv product."""
    hidden, heads = 2 * D, ar.HEADS
    x, sd = block_inputs(B, L, D, hidden)
    dy = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L + D + 21))
    s1, s2 = tr.make_scales(B, 9300 + L)
    scale = (D // heads) ** -0.5

    def reference(x):
        y, g = tr.grads64(x, sd, dy, scale=scale, s1=s1, s2=s2)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def plans(F):
        from stgcn_amd import _capi
        return F.vit_wgrad_plan(B * L, D, D, _capi.VIT_WGRAD_SMALL), F.vit_wgrad_plan(B * L, D, 3 * D, _capi.VIT_WGRAD_SMALL)

    def on(dev):
        from stgcn_amd import _capi
        from stgcn_amd.altformer import HEAD_TRAIN_MATH
        F = hipF()
        ps = [sd[k].to(dev) for k in tr.PARAMS]
        dyd, s1d, s2d = dy.to(dev), s1.to(dev), s2.to(dev)
        args = (heads, ar.EPS, scale, HEAD_TRAIN_MATH[mode] | _capi.VIT_TILE_AUTO | _capi.VIT_WGRAD_SMALL, s1d, s2d)

        def run(x):
            xd = x.to(dev)
            y, saved = F.vit_block_forward_train(xd, ps, *args, drop=(None, None, None))
            g = F.vit_block_backward(xd, ps, saved, dyd, *args, drop=(None, None, None))
            return {"y": y, "dx": g["x"], **{"d" + k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS)}}
        return run
    return Setup(x, reference, on, plans=plans)


def st_attention_math(name, math="bf16x3"):
    """gcn_unit_attention under set_st_attention_math on a unit case of st_attention_math_ref without a drop-connect mask: the eval
    forward ("eval" cases: {"y"}) or one training step ("train" cases: y, dx, every parameter gradient, the running statistics).
    The state is loaded from device copies: nothing in ``run`` comes from the host."""
    import st_attention_math_ref as MR
    c, sd, x, dy, mask, _ = MR.unit_reference(name)
    assert mask is None, "a recorded drop-connect mask is uploaded inside the step"
    training = c["mode"] == "train"
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}

    def reference(x):
        if not training:
            with torch.no_grad():
                return {"y": R.forward64(sd64, x.double(), False)[0]}
        yr, new, g, dx = R.grads64(sd, x, dy, training=True, mask=None)
        return {"y": yr, "dx": dx, **{"d" + k: v for k, v in g.items()}, **new}

    def on(dev):
        from stgcn_amd import set_st_attention_math
        m = st_unit(c["cin"], c["cout"], c["V"], sd, drop_connect=False).train(training)
        set_st_attention_math(m, math)
        sdd, dyd = {k: v.to(dev) for k, v in sd.items()}, dy.to(dev)

        def run(x):
            if not training:
                with torch.no_grad():
                    return {"y": m(x.to(dev))}
            m.load_state_dict(sdd)
            for p in m.parameters():
                p.grad = None
            xg = x.to(dev).detach().clone().requires_grad_(True)
            y = m(xg)
            y.backward(dyd)
            return {"y": y.detach(), "dx": xg.grad, **{"d" + k: p.grad for k, p in m.named_parameters()},
                    **{k: v.clone() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}}
        return run
    return Setup(x, reference, on)


def wx_product(name, math="bf16x3"):
    """F.wx_product on a product case of st_attention_math_ref; ``x`` is X (N, K, TV)."""
    import st_attention_math_ref as MR
    ref = MR.product_reference(name)
    c = ref["case"]

    def reference(X):
        out = ref["Wmk"].double() @ X.double()
        for add in (None if ref["bias"] is None else ref["bias"].view(1, -1, 1), ref["R"]):
            out = out if add is None else out + add.double()
        return {"C": out}

    def on(dev):
        F = hipF()
        up = lambda t: None if t is None else t.to(dev)       # noqa: E731
        W, bias, Rr = up(ref["W"]), up(ref["bias"]), up(ref["R"])
        return lambda X: {"C": F.wx_product(W, X.to(dev), bias, Rr, w_transposed=c["wt"], math=math_flag(math))}
    return Setup(ref["X"], reference, on)


def vit_linear_backward(M, K, Nout, math):
    """F.vit_linear_backward with GELU' and every output; ``x`` is dy (M, Nout)."""
    g = torch.Generator().manual_seed(M + K + Nout + 1)
    dy = torch.randn(M, Nout, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g))
    a = torch.randn(M, K, generator=g) + 0.5
    W = (torch.rand(Nout, K, generator=g) * 2 - 1) / K ** 0.5
    h = torch.randn(M, K, generator=g) * 1.5
    h64 = h.double().requires_grad_(True)
    TF.gelu(h64).sum().backward()

    def reference(dy):
        return {"dx": dy.double() @ W.double() * h64.grad, "dW": dy.double().T @ a.double(), "db": dy.double().sum(0)}

    def on(dev):
        F = hipF()
        ad, Wd, hd = a.to(dev), W.to(dev), h.to(dev)
        assert F.vit_linear_backward_supported(M, K, Nout, math_flag(math))
        return lambda dy: dict(zip(("dx", "dW", "db"), F.vit_linear_backward(dy.to(dev), ad, Wd, h_pre=hd, math=math_flag(math))))
    return Setup(dy, reference, on)


def vit_layernorm_backward(M, D):
    """F.vit_layernorm_backward with and without the residual gradient, against autograd of ar.layer_norm64; ``x`` is dn, the
    gradient of the LayerNorm's output.  ``operands``: (x, w, b, dres) on the CPU."""
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, D, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dn, dres = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)

    def reference(dn):
        x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
        ar.layer_norm64(x64, w64, b64).backward(dn.double())
        out = {}
        for res in (False, True):
            out[f"dx[dres={res}]"] = x64.grad + (dres.double() if res else 0)
            out[f"dweight[dres={res}]"], out[f"dbias[dres={res}]"] = w64.grad, b64.grad
        return out

    def on(dev):
        F = hipF()
        xd, wd, dresd = (t.to(dev) for t in (x, w, dres))

        def run(dn):
            out, dnd = {}, dn.to(dev)
            for res in (False, True):
                out[f"dx[dres={res}]"], out[f"dweight[dres={res}]"], out[f"dbias[dres={res}]"] = \
                    F.vit_layernorm_backward(xd, dnd, wd, ar.EPS, dres=dresd if res else None)
            return out
        return run
    return Setup(dn, reference, on)


def vit_attention_backward(B, L, hd, form="resident"):
    """F.vit_attention then its backward ('resident': vit_attention_backward; 'stream': the streaming pair at every length) on
    peaked scores, 8 heads; ``x`` is dout.  ``run`` also returns the forward's "out", which no reference names."""
    heads = 8
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd)
    dout = torch.randn(B, L, heads * hd, generator=torch.Generator().manual_seed(L + hd))

    def reference(dout):
        return {"dqkv": attention_grad64(qkv, dout, heads, hd ** -0.5)[1]}

    def on(dev):
        F = hipF()
        qd = qkv.to(dev)
        fwd, bwd = (F.vit_attention_stream, F.vit_attention_backward_stream) if form == "stream" else (F.vit_attention, F.vit_attention_backward)

        def run(dout):
            out = fwd(qd, heads)
            return {"out": out, "dqkv": bwd(qd, out, dout.to(dev), heads)}
        return run
    return Setup(dout, reference, on)


def step_stats(n, classes, special=False):
    """dist.step_stats on quarter-rounded logits (ties) with labels that agree with numpy's argmax on about 70 % of the rows;
    ``x`` is the logits.  ``special`` (n >= 8): an all-equal row, +inf, a row of -inf, a NaN and a tie with the first class.  The
    probed tensor is the first four columns of the logits seen as (n, 4, 1, 1), in place through its strides, unless
    ``on(dev, out)`` is given one.  Outputs: "pred"; "count_correct" = stats[[0, 3]]; "probe" = stats[1:3]."""
    import numpy as np
    gen = torch.Generator().manual_seed(n + classes)
    logits = (torch.randn(n, classes, generator=gen) * 4).round() / 4
    if special and n >= 8:
        logits[1] = 0.0
        logits[2, classes - 1] = float("inf")
        logits[3, :] = float("-inf")
        logits[4, 1] = float("nan")
        logits[5, 0] = logits[5].max()
    want = np.argmax(logits.numpy(), axis=1)
    labels = torch.from_numpy(want.copy())
    flip = torch.rand(n, generator=gen) < 0.3
    labels[flip] = (labels[flip] + 1) % classes

    def reference(logits, probe=None):
        am = torch.from_numpy(np.argmax(logits.numpy(), axis=1))
        probe = logits[:, :min(4, classes)].double() if probe is None else probe
        return {"pred": am.double(), "count_correct": torch.tensor([float(len(logits)), float((am == labels).sum())], dtype=torch.float64),
                "probe": torch.stack([probe.sum(), probe.square().sum()])}

    def on(dev, out=None):
        from stgcn_amd import dist as sd
        lab = labels.to(dev)

        def run(logits):
            ld = logits.to(dev)
            o = ld[:, :min(4, classes)].unsqueeze(-1).unsqueeze(-1) if out is None else out
            pred = torch.full((len(ld),), -1, dtype=torch.int64, device=dev)
            stats = sd.step_stats(o, len(ld), ld, lab, pred)
            return {"pred": pred, "count_correct": torch.stack([stats[0], stats[3]]), "probe": stats[1:3]}
        return run
    return Setup(logits, reference, on, labels=labels, want=want, gen=gen)


def bn_fold(C):
    """F.bn_fold with a conv bias; ``x`` is the running mean: the shift follows it, the scale cannot."""
    g = torch.Generator().manual_seed(C)
    w, b, cb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2, torch.randn(C, generator=g) * 0.1
    mean, var = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) * 1.5 + 0.25

    def reference(mean):
        scale = w.double() / torch.sqrt(var.double() + hipF().BN_EPS)
        return {"scale": scale, "shift": b.double() + (cb.double() - mean.double()) * scale}

    def on(dev):
        F = hipF()
        wd, bd, vd, cd = (t.to(dev) for t in (w, b, var, cb))
        return lambda mean: dict(zip(("scale", "shift"), F.bn_fold(wd, bd, mean.to(dev), vd, cd)))
    return Setup(mean, reference, on)
