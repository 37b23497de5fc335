"""fp64 restatement of one transformer block of the AltFormer heads, written from the formulas, plus the seeded recipes the
fixture tests/golden/make_golden_altformer.py and the tests share (block cases, inputs, parameter preparation).

    a  = LN1(x);  qkv = a Wqkv^T + bqkv, split into q, k, v and heads;  w = softmax over keys of scale * q k^T
    x1 = x + (heads of w v, concatenated) Wproj^T + bproj
    y  = x1 + GELU(LN2(x1) W1^T + b1) W2^T + b2          (LayerNorm: biased variance, eps inside the root; GELU: erf form)
"""
import math
from functools import partial

import torch

EPS = 1e-6           # the heads build their LayerNorms with eps = 1e-6
HEADS = 8
QK_FACTOR = 4.0      # the q and k rows of attn.qkv.weight are multiplied by this: scores reach 26-30, the soft-max is peaked

# one case per stage of the heads (B sequences of L tokens, dim D, hidden 2 D):      name: (B, L, D, qkv_bias, qk_scale, seed)
BLOCK_CASES = {
    "st_spatial_L22_D256": (24, 22, 256, True, None, 9101),
    "st_temporal_L180_D512": (8, 180, 512, True, None, 9102),
    "st_temporal_L150_D512_scale": (8, 150, 512, True, 0.2, 9103),
    "ts_temporal_L180_D256_nobias": (12, 180, 256, False, None, 9104),
    "ts_spatial_L46_D512": (16, 46, 512, True, None, 9105),
    "ts_spatial_L22_D512": (16, 22, 512, True, None, 9106),
}
DENSE_LIMIT = 20_000    # outputs up to this many elements are stored whole, larger ones as samples


def norm_layer():
    return partial(torch.nn.LayerNorm, eps=EPS)


def build_block(block_cls, name):
    """The block of a case: built by ``block_cls`` from the case's seed, then prepared (prepare_block)."""
    B, L, D, qkv_bias, qk_scale, seed = BLOCK_CASES[name]
    torch.manual_seed(seed)
    blk = block_cls(dim=D, num_heads=HEADS, mlp_ratio=2., qkv_bias=qkv_bias, qk_scale=qk_scale, norm_layer=norm_layer())
    prepare_block(blk, seed)
    return blk.eval()


def prepare_block(blk, seed, factor=QK_FACTOR):
    """Peaked soft-max (q, k rows of the qkv weight times ``factor``) and LayerNorms that are not the identity affine map
    (weight 1 + 0.2 n, bias 0.1 n from a generator seeded with seed + 7), so that every parameter matters."""
    g = torch.Generator().manual_seed(seed + 7)
    D = blk.norm1.weight.numel()
    with torch.no_grad():
        blk.attn.qkv.weight[:2 * D] *= factor
        for ln in (blk.norm1, blk.norm2):
            ln.weight.copy_(1 + 0.2 * torch.randn(D, generator=g))
            ln.bias.copy_(0.1 * torch.randn(D, generator=g))


def make_input(name):
    """Rows with seeded scales in [0.25, 4) and a seeded per-row offset: LayerNorm matters, max|y| stays near a typical |y|."""
    B, L, D, _, _, seed = BLOCK_CASES[name]
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, L, D, generator=g)
    return (x * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)).contiguous()


def sample_idx(n, count, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (min(count, n),), generator=g).to(torch.int32)


def layer_norm64(x, w, b, eps=EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def attention64(qkv, heads, scale):
    """qkv (B, L, 3*D) packed as (3, heads, head_dim) on the last axis -> (B, L, D)."""
    B, L, D3 = qkv.shape
    hd = D3 // 3 // heads
    t = qkv.double().reshape(B, L, 3, heads, hd)
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]                       # (B, L, heads, hd)
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    s = s - s.max(dim=-1, keepdim=True).values
    w = torch.exp(s)
    w = w / w.sum(dim=-1, keepdim=True)
    return torch.einsum("bhij,bjhd->bihd", w, v).reshape(B, L, heads * hd)


def block64(x, sd, heads=HEADS, scale=None, eps=EPS):
    """fp64 forward of one block from its state_dict (keys of Block); returns (y, {"ln1", "att", "x1"})."""
    p = {k: v.double() for k, v in sd.items()}
    x = x.double()
    D = x.shape[-1]
    scale = scale or (D // heads) ** -0.5
    ln1 = layer_norm64(x, p["norm1.weight"], p["norm1.bias"], eps)
    qkv = ln1 @ p["attn.qkv.weight"].T
    if "attn.qkv.bias" in p:
        qkv = qkv + p["attn.qkv.bias"]
    att = attention64(qkv, heads, scale)
    x1 = x + att @ p["attn.proj.weight"].T + p["attn.proj.bias"]
    h = layer_norm64(x1, p["norm2.weight"], p["norm2.bias"], eps) @ p["mlp.fc1.weight"].T + p["mlp.fc1.bias"]
    h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2.0)))
    y = x1 + h @ p["mlp.fc2.weight"].T + p["mlp.fc2.bias"]
    return y, {"ln1": ln1, "att": att, "x1": x1}


def random_block_state(D, hidden, qkv_bias=True, seed=0, factor=QK_FACTOR):
    """A seeded state_dict for shapes without a fixture (weights ~ U(-1/sqrt(in), 1/sqrt(in)) as nn.Linear draws them)."""
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        return (torch.rand(o, i, generator=g) * 2 - 1) / math.sqrt(i), (torch.rand(o, generator=g) * 2 - 1) / math.sqrt(i)
    sd = {}
    sd["norm1.weight"], sd["norm1.bias"] = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    w, b = lin(3 * D, D)
    w[:2 * D] *= factor
    sd["attn.qkv.weight"] = w
    if qkv_bias:
        sd["attn.qkv.bias"] = b
    sd["attn.proj.weight"], sd["attn.proj.bias"] = lin(D, D)
    sd["norm2.weight"], sd["norm2.bias"] = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    sd["mlp.fc1.weight"], sd["mlp.fc1.bias"] = lin(hidden, D)
    sd["mlp.fc2.weight"], sd["mlp.fc2.bias"] = lin(D, hidden)
    return sd
