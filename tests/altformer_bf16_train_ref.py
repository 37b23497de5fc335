"""fp64 emulation of the training mode ``VIT_TRAIN_BF16`` of one AltFormer block (include/stgcn_hip.h, DESIGN section 15
"bf16"): ``altformer_train_ref.block64`` with every linear an ``autograd.Function`` that rounds to nearest-even bf16 at exactly
the points the contract names, everything else fp64.

    forward  proj, fc1, fc2 : y  = r(a) r(W)^T + b                       (the qkv forward: a W^T + b, unrounded)
    dgrad    all four       : da = r(g) r(W)                             (GELU' and the row factor after it, in fp64)
    wgrad    all four       : dW = r(g)^T r(a),   db = column sums of the UNROUNDED g

g is the gradient that reaches the branch's output.  The stochastic-depth factor s of a branch belongs to its last linear
(proj, fc2), y = s (a W^T + b), and sits where the kernels put it: the dgrad rounds the unscaled g and multiplies the product
by s afterwards (the linear kernel's fp32 epilogue), da = s (r(g) r(W)); the wgrad applies it while loading, before the
rounding, dW = r(s g)^T r(a), and the bias gradient sums the unrounded s g.

``POINTS`` names the six rounding points; ``skip`` leaves one out (the tests' and ``__main__``'s leave-one-out runs), and
``dtype=torch.float32`` runs the same emulation in fp32 torch ops on the CPU, the stand-in for the kernels' fp32 noise.

    python tests/altformer_bf16_train_ref.py        reprints the constants of DESIGN section 15 "bf16"
"""
import math

import torch

import altformer_ref as ar
import altformer_train_ref as tr

POINTS = ("fwd_a", "fwd_w", "dgrad_dy", "dgrad_w", "wgrad_dy", "wgrad_a")


def r(t):
    """Round to nearest-even bf16 (through fp32, as the kernels see the value), back in the dtype of ``t``."""
    return t.float().bfloat16().to(t.dtype)


class _Linear(torch.autograd.Function):
    """y = a W^T (+ b) with the mode's rounding points; ``exact_fwd``: the forward product unrounded (the qkv linear)."""

    @staticmethod
    def forward(ctx, a, W, b, s, exact_fwd, skip):
        def rr(t, point):
            return t if point == skip else r(t)
        ctx.save_for_backward(a, W)
        ctx.rr, ctx.has_bias, ctx.s = rr, b is not None, s
        y = a @ W.T if exact_fwd else rr(a, "fwd_a") @ rr(W, "fwd_w").T
        y = y if b is None else y + b
        return y if s is None else y * s

    @staticmethod
    def backward(ctx, g):
        a, W = ctx.saved_tensors
        rr = ctx.rr
        da = rr(g, "dgrad_dy") @ rr(W, "dgrad_w")
        if ctx.s is not None:
            da, g = da * ctx.s, g * ctx.s
        g2, a2 = g.reshape(-1, g.shape[-1]), a.reshape(-1, a.shape[-1])
        dW = rr(g2, "wgrad_dy").T @ rr(a2, "wgrad_a")
        return da, dW, (g2.sum(0) if ctx.has_bias else None), None, None, None


def block_train_bf16(x, sd, heads=ar.HEADS, scale=None, eps=ar.EPS, s1=None, s2=None, skip=None, qkv_exact=True):
    """Forward of one block in the mode from tensors keyed like Block's state_dict (any float dtype, possibly requires_grad)."""
    D = x.shape[-1]
    scale = scale or (D // heads) ** -0.5
    ln1 = ar.layer_norm64(x, sd["norm1.weight"], sd["norm1.bias"], eps)
    s1, s2 = (None if s is None else s.to(x.dtype).reshape(-1, 1, 1) for s in (s1, s2))
    qkv = _Linear.apply(ln1, sd["attn.qkv.weight"], sd.get("attn.qkv.bias"), None, qkv_exact, skip)
    att = attention(qkv, heads, scale)
    x1 = x + _Linear.apply(att, sd["attn.proj.weight"], sd["attn.proj.bias"], s1, False, skip)
    h = _Linear.apply(ar.layer_norm64(x1, sd["norm2.weight"], sd["norm2.bias"], eps), sd["mlp.fc1.weight"], sd["mlp.fc1.bias"],
                      None, False, skip)
    h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2.0)))
    return x1 + _Linear.apply(h, sd["mlp.fc2.weight"], sd["mlp.fc2.bias"], s2, False, skip)


def attention(qkv, heads, scale):
    """altformer_ref.attention64 in the dtype of ``qkv`` (that function casts to fp64)."""
    B, L, D3 = qkv.shape
    hd = D3 // 3 // heads
    t = qkv.reshape(B, L, 3, heads, hd)
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    w = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    w = w / w.sum(dim=-1, keepdim=True)
    return torch.einsum("bhij,bjhd->bihd", w, v).reshape(B, L, heads * hd)


def grads_bf16(x, sd, dy, heads=ar.HEADS, scale=None, eps=ar.EPS, s1=None, s2=None, skip=None, dtype=torch.float64,
               qkv_exact=True):
    """(y, {"x": dx, <param key>: grad, ...}) of the emulation, keyed like altformer_train_ref.grads64's, as fp64 tensors."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = x.detach().to(dtype).requires_grad_(True)
    y = block_train_bf16(x, p, heads, scale, eps, s1, s2, skip, qkv_exact)
    y.backward(dy.to(dtype))
    g = {k: v.grad.double() for k, v in p.items()}
    g["x"] = x.grad.double()
    return y.detach().double(), g


def max_rel(got, want):
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def l2_ratio(cand, emu, ref):
    """||candidate - emulation|| / ||emulation - fp64||: how far a result is from the emulation, in units of the distance the
    rounding points themselves move the tensor.  Same rounding points: the fp32 noise; a point missing or extra: order 1."""
    cand, emu, ref = (torch.as_tensor(t).double().cpu() for t in (cand, emu, ref))
    return ((cand - emu).norm() / (emu - ref).norm().clamp_min(1e-300)).item()


def max_ratio(cand, emu, ref):
    cand, emu, ref = (torch.as_tensor(t).double().cpu() for t in (cand, emu, ref))
    return ((cand - emu).abs().max() / (emu - ref).abs().max().clamp_min(1e-300)).item()


EXACT_IN_EMULATION = ("mlp.fc2.bias",)   # dfc2.bias = column sums of the unrounded s2 dy: the emulation equals fp64 there


def case_inputs(name, factors):
    from stgcn_amd.altformer import Block
    B, L, D, _, _, seed = ar.BLOCK_CASES[name]
    blk = ar.build_block(Block, name)
    s1, s2 = tr.make_scales(B, seed) if factors else (None, None)
    return ar.make_input(name), blk.state_dict(), tr.make_dy(name), blk.attn.scale, s1, s2


def stream_inputs(factor=ar.QK_FACTOR):
    """The streaming-plan input of the GPU tests: one block at L = 300, D = 256, B = 3 (no fixture case is that long)."""
    B, L, D = 3, 300, 256
    g = torch.Generator().manual_seed(4242)
    sd = ar.random_block_state(D, 2 * D, seed=4243, factor=factor)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    dy = torch.randn(B, L, D, generator=g)
    s1, s2 = tr.make_scales(B, 4244)
    return x.contiguous(), sd, dy, (D // ar.HEADS) ** -0.5, s1, s2


def report(tag, x, sd, dy, scale, s1, s2, leave_one_out=True):
    kw = dict(scale=scale, s1=s1, s2=s2)
    y64, g64 = tr.grads64(x, sd, dy, **kw)
    ye, ge = grads_bf16(x, sd, dy, **kw)
    ya, ga = grads_bf16(x, sd, dy, qkv_exact=False, **kw)
    yf, gf = grads_bf16(x, sd, dy, dtype=torch.float32, **kw)
    keys = [k for k in ge if k not in EXACT_IN_EMULATION]
    print(f"{tag}: y {max_rel(ye, y64):.2e}; worst tensor {max(max_rel(ge[k], g64[k]) for k in ge):.2e} "
          f"(every linear rounded, qkv forward too: {max(max_rel(ga[k], g64[k]) for k in ga):.2e})")
    for k in sorted(ge):
        print(f"    d{k}: emulation vs fp64 {max_rel(ge[k], g64[k]):.2e}")
    print(f"    fp32 run of the emulation, worst tensor: L2 ratio {max(l2_ratio(gf[k], ge[k], g64[k]) for k in keys):.3f}, "
          f"max-norm ratio {max(max_ratio(gf[k], ge[k], g64[k]) for k in keys):.3f}; y L2 {l2_ratio(yf, ye, y64):.3f}")
    if leave_one_out:
        for point in POINTS:
            _, gs = grads_bf16(x, sd, dy, skip=point, **kw)
            worst = max(keys, key=lambda k: l2_ratio(gs[k], ge[k], g64[k]))
            print(f"    without {point}: largest L2 ratio {l2_ratio(gs[worst], ge[worst], g64[worst]):.3f} on d{worst}; "
                  f"dattn.proj.weight {l2_ratio(gs['attn.proj.weight'], ge['attn.proj.weight'], g64['attn.proj.weight']):.3f}")


if __name__ == "__main__":
    import os
    import sys
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(_here), "st-gcn-altformer_amd"))
    for _name in sorted(ar.BLOCK_CASES):
        for _factors in (False, True):
            report(f"{_name} {'with' if _factors else 'without'} factors", *case_inputs(_name, _factors),
                   leave_one_out=_factors)
    report("stream L300 D256 B3 with factors", *stream_inputs())
