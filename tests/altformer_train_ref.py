"""fp64 restatement of one AltFormer block WITH stochastic depth's per-sequence factors, differentiated by fp64 autograd, and
the seeded recipes the gradient fixture (tests/golden/make_golden_altformer_train.py) and the training tests share.

    x1 = x  + s1[b] * (MHA(LN1(x)) Wproj^T + bproj)
    y  = x1 + s2[b] * (GELU(LN2(x1) W1^T + b1) W2^T + b2)          s1, s2: 0 or 1 / keep per sequence, None = 1
"""
import math

import torch

import altformer_ref as ar

PARAMS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
          "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
N_SAMPLES = 2000          # gradients larger than ar.DENSE_LIMIT are stored as this many seeded samples


def make_dy(name):
    """The seeded upstream gradient of a block case."""
    B, L, D, _, _, seed = ar.BLOCK_CASES[name]
    return torch.randn(B, L, D, generator=torch.Generator().manual_seed(seed + 21))


def make_scales(B, seed, keep=0.9):
    """Two seeded stochastic-depth vectors (B,): 0 for dropped sequences, 1 / keep for the others; at least one dropped and
    one kept sequence in each."""
    g = torch.Generator().manual_seed(seed + 31)
    out = []
    for _ in range(2):
        m = torch.empty(B).bernoulli_(keep, generator=g)
        m[int(torch.randint(0, B, (1,), generator=g))] = 0.0
        if B > 1 and m.sum() == 0:
            m[0] = 1.0
        out.append(m / keep)
    return out


def block64(x, sd, heads=ar.HEADS, scale=None, eps=ar.EPS, s1=None, s2=None):
    """fp64 forward of one block from a dict of (fp64, possibly requires_grad) tensors keyed like Block's state_dict."""
    D = x.shape[-1]
    scale = scale or (D // heads) ** -0.5
    ln1 = ar.layer_norm64(x, sd["norm1.weight"], sd["norm1.bias"], eps)
    qkv = ln1 @ sd["attn.qkv.weight"].T
    if sd.get("attn.qkv.bias") is not None:
        qkv = qkv + sd["attn.qkv.bias"]
    a = ar.attention64(qkv, heads, scale) @ sd["attn.proj.weight"].T + sd["attn.proj.bias"]
    x1 = x + (a if s1 is None else a * s1.double().reshape(-1, 1, 1))
    h = ar.layer_norm64(x1, sd["norm2.weight"], sd["norm2.bias"], eps) @ sd["mlp.fc1.weight"].T + sd["mlp.fc1.bias"]
    h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2.0)))
    m = h @ sd["mlp.fc2.weight"].T + sd["mlp.fc2.bias"]
    return x1 + (m if s2 is None else m * s2.double().reshape(-1, 1, 1))


def grads64(x, sd, dy, heads=ar.HEADS, scale=None, eps=ar.EPS, s1=None, s2=None):
    """(y, {"x": dx, <param key>: grad, ...}) in fp64 by autograd of block64."""
    p = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    x = x.detach().double().requires_grad_(True)
    y = block64(x, p, heads, scale, eps, s1, s2)
    y.backward(dy.double())
    g = {k: v.grad for k, v in p.items()}
    g["x"] = x.grad
    return y.detach(), g


def module_grads(blk, x, dy):
    """(y, gradients) of an nn.Module block by torch autograd in the module's dtype, keyed like grads64's."""
    x = x.detach().clone().requires_grad_(True)
    for p in blk.parameters():
        p.grad = None
    y = blk(x)
    y.backward(dy.to(y.dtype))
    g = {k: p.grad for k, p in blk.named_parameters()}
    g["x"] = x.grad
    return y.detach(), g
