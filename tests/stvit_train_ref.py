"""fp64 restatement of one ST-ViT encoder layer IN TRAINING, with its three dropouts as explicit masks and stochastic depth's
per-sequence factors, differentiated by fp64 autograd; plus the seeded recipes that the fixture
(tests/golden/make_golden_stvit_train.py) and the training tests share.

    a     = MHA(LN1(x)) Wproj^T + bproj                 x1 = x  + s1[b] (m_proj * a)
    h_pre = LN2(x1) W1^T + b1                           h  = m_act * GELU(h_pre)
    y     = x1 + s2[b] (m_fc2 * (h W2^T + b2))

``*`` elementwise; m_proj (B, L, D), m_act (B, L, hidden), m_fc2 (B, L, D) hold 0 or 1 / keep, None = 1; s1, s2 (B,) or None.
The qkv linear has no bias (model/ST_Vit/trans.py), the GELU is the exact one, LayerNorm eps 1e-5.
"""
import math

import torch

import altformer_ref as ar
import altformer_train_ref as tr
import stvit_ref as sr

K_SLAB_ROWS = 32768   # vit.h's kSlabRows: long inputs are walked in slabs of whole sequences of about this many tokens
# name: (B, L, D, heads, hidden)
CASES = {
    "vit": (2, 100, 512, 8, 512),                            # the real layer; 200 rows, a full 128-row tile and a tail
    "odd": (3, 37, 256, 8, 1024),                            # hidden != D, head_dim 32, fewer rows than a tile
    "slabs": (K_SLAB_ROWS // 100 + 3, 100, 256, 8, 256),     # two slabs of sequences, the second of 3
}
KEEP = 0.5                                                   # factor 2.0: a mask left out or misplaced moves results by O(1)
PARAMS = tuple(k for k in tr.PARAMS if k != "attn.qkv.bias")
N_SAMPLES = tr.N_SAMPLES
# the fixture: the reference's ViT at the real configuration, two layers, two clips
FIXTURE_DEPTH, FIXTURE_MASK_SEED, FIXTURE_DLOGITS_SEED = 2, 8100, 8200


def make_masks(B, L, D, hidden, seed, keep=KEEP):
    """(m_proj, m_act, m_fc2), seeded, fp32 factors 0 or 1 / keep.  Sequence 0 has all three masks zero (both branches
    dropped whole: y = x, dx = dy).  From three sequences on, sequence 1 has all three masks one (no dropout at all); with
    two sequences the second keeps its drawn masks, or no sequence of the call would see a factor other than 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for width in (D, hidden, D):
        m = torch.empty(B, L, width).bernoulli_(keep, generator=g) / keep
        m[0] = 0.0
        if B >= 3:
            m[1] = 1.0
        out.append(m)
    return tuple(out)


def make_params(D, hidden, seed):
    """A layer's eleven parameters keyed like altformer_train_ref.PARAMS (no qkv bias), seeded: LayerNorms away from the
    identity, linears as nn.Linear draws them."""
    g = torch.Generator().manual_seed(seed)

    def lin(n, k):
        return (torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5, (torch.rand(n, generator=g) * 2 - 1) / k ** 0.5
    sd = {}
    for n in ("norm1", "norm2"):
        sd[n + ".weight"], sd[n + ".bias"] = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    sd["attn.qkv.weight"], _ = lin(3 * D, D)
    sd["attn.proj.weight"], sd["attn.proj.bias"] = lin(D, D)
    sd["mlp.fc1.weight"], sd["mlp.fc1.bias"] = lin(hidden, D)
    sd["mlp.fc2.weight"], sd["mlp.fc2.bias"] = lin(D, hidden)
    return sd


def make_case(name):
    """(x, dy, params, masks) of a case, seeded: rows of x with their own scale and offset, as the blocks' tests draw them."""
    B, L, D, _, hidden = CASES[name]
    seed = 9000 + 7 * L + D + hidden
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    dy = torch.randn(B, L, D, generator=g)
    return x, dy, make_params(D, hidden, seed + 1), make_masks(B, L, D, hidden, seed + 2)


def layer64(x, sd, masks=(None, None, None), s1=None, s2=None, heads=8, scale=None, eps=sr.LN_EPS):
    """fp64 forward of one layer from a dict of (fp64, possibly requires_grad) tensors keyed like PARAMS."""
    D = x.shape[-1]
    scale = scale or (D // heads) ** -0.5
    m_proj, m_act, m_fc2 = (None if m is None else m.double() for m in masks)
    row = lambda s: s.double().reshape(-1, 1, 1)     # noqa: E731
    qkv = ar.layer_norm64(x, sd["norm1.weight"], sd["norm1.bias"], eps) @ sd["attn.qkv.weight"].T
    a = ar.attention64(qkv, heads, scale) @ sd["attn.proj.weight"].T + sd["attn.proj.bias"]
    if m_proj is not None:
        a = a * m_proj
    x1 = x + (a if s1 is None else a * row(s1))
    h = ar.layer_norm64(x1, sd["norm2.weight"], sd["norm2.bias"], eps) @ sd["mlp.fc1.weight"].T + sd["mlp.fc1.bias"]
    h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2.0)))
    if m_act is not None:
        h = h * m_act
    m = h @ sd["mlp.fc2.weight"].T + sd["mlp.fc2.bias"]
    if m_fc2 is not None:
        m = m * m_fc2
    return x1 + (m if s2 is None else m * row(s2))


def grads64(x, sd, dy, masks=(None, None, None), s1=None, s2=None, heads=8, scale=None, eps=sr.LN_EPS):
    """(y, {"x": dx, <param key>: grad, ...}) in fp64 by autograd of layer64."""
    p = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    x = x.detach().double().requires_grad_(True)
    y = layer64(x, p, masks, s1, s2, heads, scale, eps)
    y.backward(dy.double())
    g = {k: v.grad for k, v in p.items()}
    g["x"] = x.grad
    return y.detach(), g


def fixture_masks(layer):
    """The masks of layer ``layer`` of the fixture's model: 2 clips of 100 tokens at dim = mlp_dim = 512."""
    c = sr.CONFIG
    tokens = (c["time_len"] // c["p1"]) * (c["joint"] // c["p2"]) + 1
    return make_masks(sr.CLIPS, tokens, c["dim"], c["mlp_dim"], FIXTURE_MASK_SEED + layer)


def fixture_dlogits():
    return torch.randn(sr.CLIPS, sr.CONFIG["num_classes"], generator=torch.Generator().manual_seed(FIXTURE_DLOGITS_SEED))


def vit_train64(z, sd, depth, masks, heads=8, dim_head=sr.DIM_HEAD):
    """fp64 logits of the ViT in training from a state_dict of fp64 (possibly requires_grad) tensors: stvit_ref's embedding,
    ``depth`` layers through layer64 with ``masks[i]``, the class token, LayerNorm, Linear.  ``z`` fp64."""
    c = sr.CONFIG
    x = sr.embed64(z, sd["to_patch_embedding.1.weight"], sd["to_patch_embedding.1.bias"], sd["cls_token"], sd["pos_embedding"][0],
                   c["p1"], c["p2"])
    for i in range(depth):
        x = layer64(x, sr._block_state(sd, i), masks[i], heads=heads, scale=dim_head ** -0.5)
    ln = ar.layer_norm64(x[:, 0], sd["mlp_head.0.weight"], sd["mlp_head.0.bias"], sr.LN_EPS)
    return ln @ sd["mlp_head.1.weight"].T + sd["mlp_head.1.bias"]
