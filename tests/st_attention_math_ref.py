"""The 'bf16x3' arithmetic of gcn_unit_attention's 1x1 projections, restated from its definition, and the cases the two test
files tests/test_st_attention_math_{host,gpu}.py share.  A plain module: no GPU, no test module imported.

    wh = bf16(w), wl = bf16(w - wh), the same for x;   W . X  :=  sum_k  wh.xh + wh.xl + wl.xh      (no wl.xl)

``emu3`` is that sum in fp64 (every bf16 x bf16 product is exact in fp32, so a kernel differs from it by the rounding of its
fp32 sums alone).  ``SplitProduct`` is the autograd form the unit uses: forward emu3, input gradient emu3 on W^T and dY, weight
gradient exact; ``forward64`` is st_attention_ref.forward64 with its two ``einsum("oc,bcv->bov")`` products replaced by it.
"""
import functools

import torch
import torch.nn.functional as TF

import st_attention_ref as R
from _util import kink_free_cotangent

U32 = 2.0 ** -24         # unit round-off of fp32


def split(a):
    """fp32 (or fp64, rounded to fp32 first) -> (hi, lo) as fp64 tensors holding bf16 values."""
    a32 = a.detach().to(torch.float32)
    hi = a32.to(torch.bfloat16).to(torch.float32)
    lo = (a32 - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double(), lo.double()


def emu3(W, X):
    """W (M,K), X (...,K,J) -> (...,M,J): the fp64 sum of the three split products."""
    wh, wl = split(W)
    xh, xl = split(X)
    return wh @ xh + wh @ xl + wl @ xh


def abs_sum3(W, X):
    """S[m][j] = sum_k |wh||xh| + |wh||xl| + |wl||xh|: what the rounding of an fp32 sum of the 3K products is relative to."""
    wh, wl = split(W)
    xh, xl = split(X)
    return wh.abs() @ xh.abs() + wh.abs() @ xl.abs() + wl.abs() @ xh.abs()


def three_term_fp32(W, X, order):
    """The three-term arithmetic with fp32 sums on the CPU, in two summation orders: 0 = three whole products added,
    1 = K chunks of 32 with the three terms of a chunk added to a running sum (the kernel's shape of the sum)."""
    wh, wl = (t.float() for t in split(W))
    xh, xl = (t.float() for t in split(X))
    if order == 0:
        return (wh @ xl + wl @ xh) + wh @ xh
    acc = torch.zeros(*X.shape[:-2], W.shape[0], X.shape[-1])
    for k in range(0, W.shape[1], 32):
        s = slice(k, k + 32)
        acc = acc + wh[:, s] @ xl[..., s, :]
        acc = acc + wl[:, s] @ xh[..., s, :]
        acc = acc + wh[:, s] @ xh[..., s, :]
    return acc


class SplitProduct(torch.autograd.Function):
    """einsum("oc,bcv->bov", W, X) in the three-term arithmetic (fp64 sums)."""

    @staticmethod
    def forward(ctx, W, X):
        ctx.save_for_backward(W, X)
        return emu3(W, X).to(X.dtype)

    @staticmethod
    def backward(ctx, dY):
        W, X = ctx.saved_tensors
        return torch.einsum("bov,bcv->oc", dY, X), emu3(W.t(), dY).to(dY.dtype)


class RoundedProduct(torch.autograd.Function):
    """The same with ONE bf16 rounding per operand (plain 'bf16', out of scope: its figures are quoted in DESIGN section 13)."""

    @staticmethod
    def forward(ctx, W, X):
        ctx.save_for_backward(W, X)
        return (split(W)[0] @ split(X)[0]).to(X.dtype)

    @staticmethod
    def backward(ctx, dY):
        W, X = ctx.saved_tensors
        return torch.einsum("bov,bcv->oc", dY, X), (split(W.t())[0] @ split(dY)[0]).to(dY.dtype)


def forward64(sd, x, training, mask=None, nh=R.NH, eps=R.EPS, momentum=R.MOMENTUM, product=SplitProduct.apply):
    """st_attention_ref.forward64 with ``product`` at its two projections."""
    N, C, T, V = x.shape
    Wq = sd["attention_conv.qkv_conv.weight"].flatten(1)
    Wo = sd["attention_conv.attn_out.weight"].flatten(1)
    cout = Wo.shape[0]
    dk = (Wq.shape[0] - cout) // 2
    dkh, dvh = dk // nh, cout // nh
    new = {}

    def bn(z, pre, dims):
        w, b = sd[pre + "weight"], sd[pre + "bias"]
        shape = [1] * z.dim()
        shape[1] = -1
        if training:
            mean = z.mean(dims)
            var = z.var(dims, unbiased=False)
            cnt = z.numel() / z.shape[1]
            with torch.no_grad():
                new[pre + "running_mean"] = (1 - momentum) * sd[pre + "running_mean"] + momentum * mean.detach()
                new[pre + "running_var"] = (1 - momentum) * sd[pre + "running_var"] + momentum * var.detach() * cnt / (cnt - 1)
        else:
            mean, var = sd[pre + "running_mean"], sd[pre + "running_var"]
        return (z - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * w.view(shape) + b.view(shape)

    xv = x.permute(0, 1, 3, 2).reshape(N, C * V, T)
    xn = bn(xv, "data_bn.", (0, 2)).reshape(N, C, V, T).permute(0, 1, 3, 2)
    xa = xn.permute(0, 2, 1, 3).reshape(N * T, C, V)
    qkv = product(Wq, xa) + sd["attention_conv.qkv_conv.bias"].view(1, -1, 1)
    B = N * T
    q = qkv[:, :dk].reshape(B, nh, dkh, V) * dkh ** -0.5
    k = qkv[:, dk:2 * dk].reshape(B, nh, dkh, V)
    v = qkv[:, 2 * dk:].reshape(B, nh, dvh, V)
    logits = torch.einsum("bhdi,bhdj->bhij", q, k)
    w = TF.softmax(logits, dim=-1)
    if mask is not None:
        w = w * mask.reshape(B, nh, 1, V).to(w.dtype)
        w = w / (w.sum(3, keepdim=True) + 1e-8)
    o = torch.einsum("bhij,bhej->bhei", w, v).reshape(B, cout, V)
    ao = product(Wo, o) + sd["attention_conv.attn_out.bias"].view(1, -1, 1)
    ao = ao.reshape(N, T, cout, V).permute(0, 2, 1, 3)
    z = ao + x if C == cout else ao
    return torch.relu(bn(z, "bn.", (0, 2, 3))), new


def grads_emulated(sd, x, dy, training=True, mask=None, product=SplitProduct.apply):
    """R.grads64 on the emulation: (y, running statistics, {key: grad}, dx) in fp64."""
    sd64 = {k: (v.double().clone().requires_grad_(not (k.endswith("running_mean") or k.endswith("running_var")))
                if v.is_floating_point() else v) for k, v in sd.items()}
    x64 = x.double().clone().requires_grad_(True)
    y, new = forward64(sd64, x64, training, None if mask is None else mask.double(), product=product)
    y.backward(dy.double())
    g = {k: v.grad for k, v in sd64.items() if isinstance(v, torch.Tensor) and v.grad is not None}
    return y.detach(), new, g, x64.grad


# ---- the unit cases -------------------------------------------------------------------------------------------------------------------
_UNIT_FIELDS = ("name", "N", "cin", "cout", "T", "V", "mode", "drop", "seed")
UNIT_CASES = [dict(zip(_UNIT_FIELDS, row)) for row in [
    ("ragged_k131_tv75", 2, 131, 128,  3, 25, "train", True,  201),    # K = 131 (4 chunks + 3), rows of 300 bytes
    ("skip_tv110",       2, 128, 128,  5, 22, "train", True,  202),    # the skip connection as the kernel's R
    ("k131_c256_tv264",  2, 131, 256, 12, 22, "train", True,  203),    # three column tiles, M = 384 and 131
    ("c512_v46",         2,  64, 512,  3, 46, "train", False, 204),    # M = 768, no drop-connect
    ("eval_skip_c256",   2, 256, 256,  6, 22, "eval",  False, 205),
    ("eval_k131_tv75",   2, 131, 128,  3, 25, "eval",  False, 206),
    ("skip512_tv92",     2, 512, 512,  2, 46, "train", True,  207),    # the widest layer: K = 512 = 16 chunks
]]


def unit_case(name):
    return next(c for c in UNIT_CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def unit_reference(name):
    """(case, state, x, dy, mask or None, fp64 (y, running statistics, gradients, dx)) of a unit case, computed once and
    left unchanged.  Seeds: state = seed, input = seed + 1000, mask then cotangent from one generator at seed + 2000; the
    cotangent is kink_free_cotangent of the fp64 y.  "eval" differentiates on the running statistics."""
    c = unit_case(name)
    sd = R.make_state(c["cin"], c["cout"], c["V"], c["seed"], sharp=1.0)
    x = R.make_input(c["N"], c["cin"], c["T"], c["V"], c["seed"] + 1000)
    g = torch.Generator().manual_seed(c["seed"] + 2000)
    mask = torch.bernoulli(0.5 * torch.ones(c["N"] * c["T"] * R.NH * c["V"]), generator=g) if c["drop"] else None
    training = c["mode"] == "train"
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    with torch.no_grad():
        y64, _ = R.forward64(sd64, x.double(), training, None if mask is None else mask.double())
    dy = kink_free_cotangent(y64, g)
    return c, sd, x, dy, mask, R.grads64(sd, x, dy, training=training, mask=mask)


@functools.lru_cache(maxsize=None)
def frozen_reference():
    """``frozen_mask`` of st_attention_ref.EDGE_CASES (frozen BatchNorm under autograd, drop-connect) for this arithmetic:
    its state, input and mask as they are, its cotangent drawn from the same seed but kink-free.  With the case's plain
    cotangent the emulation ALONE is 5e-3 off on every gradient: its y (8.6e-6 from fp64) puts one of 33,792 outputs on the
    other side of the ReLU, which moves the gradients by that output's whole |dL/dy| (a property of ReLU, see
    _util.kink_free_cotangent); plain fp32 (6e-7) flips none, which is why the f32 test needs no such treatment."""
    c = R.edge_case("frozen_mask")
    sd, x, _, mask = R.edge_inputs(c)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    with torch.no_grad():
        y64, _ = R.forward64(sd64, x.double(), False, mask.double(), nh=c["nh"])
    dy = kink_free_cotangent(y64, torch.Generator().manual_seed(c["seed"] + 3))
    return c, sd, x, dy, mask, R.grads64(sd, x, dy, training=False, mask=mask, nh=c["nh"])


# ---- the product cases ------------------------------------------------------------------------------------------------------------------
_PRODUCT_FIELDS = ("name", "M", "K", "TV", "N", "bias", "res", "wt")
PRODUCT_CASES = [dict(zip(_PRODUCT_FIELDS, row)) for row in [
    ("ragged_k131",   192, 131,   75, 2, True,  False, False),   # ragged K; rows 300 bytes apart
    ("ragged_m131_t", 131, 192,   75, 2, False, False, True),    # ragged M, the input-gradient orientation
    ("skip",          128, 128,  110, 2, True,  True,  False),   # bias + R
    ("wide_768x512",  768, 512,   92, 1, False, False, False),   # widest rows, 16 K chunks
    ("tiny",            5,   3,    7, 3, False, False, False),   # everything smaller than one tile
    ("many_columns",  384, 256, 2200, 1, False, False, False),   # 18 column tiles, the last one of 24 columns
]]


def product_case(name):
    return next(c for c in PRODUCT_CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def product_reference(name):
    """Seeded fp32 operands of a product case and its references: dict with W (as the call takes it: (K,M) when transposed),
    Wmk (M,K), X, bias, R, exact64, emu3 (both with the epilogue addends, in fp64), bound (the elementwise bound, below)."""
    c = product_case(name)
    g = torch.Generator().manual_seed(900 + sum(map(ord, name)))
    Wmk = torch.randn(c["M"], c["K"], generator=g) / c["K"] ** 0.5
    X = torch.randn(c["N"], c["K"], c["TV"], generator=g) * 0.8 + 0.2
    bias = torch.randn(c["M"], generator=g) * 0.1 if c["bias"] else None
    res = torch.randn(c["N"], c["M"], c["TV"], generator=g) * 0.5 if c["res"] else None
    exact = Wmk.double() @ X.double()
    emu = emu3(Wmk, X)
    S = abs_sum3(Wmk, X)
    terms = 3 * c["K"]
    for add in (None if bias is None else bias.view(1, -1, 1), res):
        if add is not None:
            exact, emu, S, terms = exact + add.double(), emu + add.double(), S + add.double().abs(), terms + 1
    # |C - emu3| <= terms * 2^-24 * S: an fp32 sum of n exactly representable terms, in whatever order, is within
    # (n - 1) u sum|terms| (1 + O(nu)) of the true sum.  terms = 3K for the bare product (the issue's bound); an epilogue
    # addend (bias, R) is one more fp32 addition and joins both the count and S.
    return dict(case=c, W=Wmk.t().contiguous() if c["wt"] else Wmk, Wmk=Wmk, X=X, bias=bias, R=res, exact64=exact, emu3=emu,
                bound=terms * U32 * S)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())
