"""fp64 references of the backward of the ST-ViT head's two ends, by fp64 autograd through the restatements the suite already
pins to the reference's ViT (stvit_ref.embed64; altformer_ref.layer_norm64), plus the seeded recipes their tests share.

    embedding : x = embed64(z, W, bias, cls, pos);  (dW, dbias, dcls, dpos, dz) = autograd of <x, dx>
    classifier: logits = LN(x[:, 0] or x.mean(1)) Whead^T + bhead;  (dx, dln_weight, dln_bias, dW, dbias) = autograd of <logits, dlogits>
"""
import torch

import altformer_ref as ar
import stvit_ref as sr

EMBED_OUTPUTS = ("dW", "dbias", "dcls", "dpos", "dz")
CLASSIFY_OUTPUTS = ("dx", "dln_weight", "dln_bias", "dW", "dbias")
# (N, L, D, classes): fewer columns than a workgroup has lanes and an odd clip count; the real head
CLASSIFY_CASES = {"small": (3, 7, 192, 14), "real": (2, 100, 512, 14)}


def make_dx(name):
    """The gradient of an embedding case's output, seeded: every row of every clip, the class rows included, has its own scale."""
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    n = (T // p1) * (V // p2)
    g = torch.Generator().manual_seed(6000 + n + E)
    return torch.randn(N, n + 1, E, generator=g) * (0.25 + 3.75 * torch.rand(N, n + 1, 1, generator=g))


def embed_grads64(z, W, bias, cls, pos, p1, p2, dx):
    """{dW, dbias, dcls, dpos, dz} in fp64."""
    leaves = [t.detach().double().requires_grad_(True) for t in (z, W, bias, cls, pos)]
    sr.embed64(*leaves, p1, p2).backward(dx.double())
    z64, W64, b64, c64, p64 = leaves
    return {"dW": W64.grad, "dbias": b64.grad, "dcls": c64.grad, "dpos": p64.grad, "dz": z64.grad}


def classify_case(name):
    """(x, ln_weight, ln_bias, W, bias, dlogits), seeded: rows of x with their own scale and offset."""
    N, L, D, classes = CLASSIFY_CASES[name]
    g = torch.Generator().manual_seed(7000 + L + D)
    x = torch.randn(N, L, D, generator=g) * (0.25 + 3.75 * torch.rand(N, L, 1, generator=g)) + torch.randn(N, L, 1, generator=g)
    ln_w, ln_b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W = (torch.rand(classes, D, generator=g) * 2 - 1) / D ** 0.5
    bias = (torch.rand(classes, generator=g) * 2 - 1) / D ** 0.5
    return x, ln_w, ln_b, W, bias, torch.randn(N, classes, generator=g)


def classify64(x, ln_w, ln_b, W, bias, pool):
    pooled = x.mean(dim=1) if pool == "mean" else x[:, 0]
    return ar.layer_norm64(pooled, ln_w, ln_b, sr.LN_EPS) @ W.T + bias


def classify_grads64(x, ln_w, ln_b, W, bias, dlogits, pool):
    """(logits, {dx, dln_weight, dln_bias, dW, dbias}) in fp64."""
    leaves = [t.detach().double().requires_grad_(True) for t in (x, ln_w, ln_b, W, bias)]
    logits = classify64(*leaves, pool)
    logits.backward(dlogits.double())
    return logits.detach(), dict(zip(CLASSIFY_OUTPUTS, (t.grad for t in leaves)))
