"""fp64 restatement of the ST-ViT head's forward, written from its formulas, plus the seeded recipes that the fixture
tests/golden/make_golden_stvit.py and the tests share (configuration, parameter preparation, inputs, embedding cases).

    z (N, C, T, V), h = T / p1, w = V / p2, n = h w, K = p1 p2 C
    patch (a, b) of clip i: element k = (f p2 + j) C + c  is  z[i][c][a p1 + f][b p2 + j]   (f slowest, then j, then c)
    x[i][0] = cls + pos[0];   x[i][1 + a w + b] = patch(a, b) W^T + bias + pos[1 + a w + b]
    depth blocks (altformer_ref.block64: pre-norm, qkv without bias, LayerNorm eps 1e-5, scale dim_head ** -0.5)
    pooled = x[:, 0] ('cls') or the mean over all n + 1 tokens ('mean');  logits = LN(pooled) Whead^T + bhead
"""
import torch

import altformer_ref as ar

LN_EPS = 1e-5
# the configuration the reference's ST_GCN_Trans builds (num_classes: the 14 gestures of SHREC)
CONFIG = dict(time_len=180, joint=22, p1=20, p2=2, num_classes=14, dim=512, depth=6, heads=8, mlp_dim=512)
CHANNELS, DIM_HEAD = 128, 64
MODEL_SEED, INPUT_SEED, CLIPS = 4711, 4712, 2

# the embedding on its own: name: (N, C, T, V, p1, p2, E)
EMBED_CASES = {
    "a_K256_rows18": (3, 32, 8, 6, 4, 2, 64),            # K = 256, 18 patch rows, 7 tokens: partial row tile, odd clip count
    "b_K5120_rows4": (1, 128, 40, 4, 20, 2, 512),        # K = 5120 with 4 rows: the K cut and its ordered sum at full depth
    "c_real_rows198": (2, 128, 180, 22, 20, 2, 512),     # the real patching, 198 rows: no tile multiple
    "d_rows396_tile128": (4, 128, 180, 22, 20, 2, 512),  # 396 rows: the plan's 128 x 128 form, its last row tile 12 rows
}


def prepare(model, seed=MODEL_SEED):
    """What a seeded construction leaves trivial is made to matter: the position table (zeros) and every LayerNorm (the
    identity affine map) get seeded values, through the state_dict keys both implementations share."""
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for key, t in model.state_dict().items():
            if key == "pos_embedding":
                t.copy_(0.5 * torch.randn(t.shape, generator=g))
            elif key.endswith("norm.weight") or key == "mlp_head.0.weight":
                t.copy_(1 + 0.2 * torch.randn(t.shape, generator=g))
            elif key.endswith("norm.bias") or key == "mlp_head.0.bias":
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
    return model


def make_input(N=CLIPS, C=CHANNELS, T=CONFIG["time_len"], V=CONFIG["joint"], seed=INPUT_SEED):
    """A stand-in for the stem output: non-negative (it follows a ReLU), with seeded per-channel scales."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, C, T, V, generator=g) * (0.25 + 1.75 * torch.rand(1, C, 1, 1, generator=g))
    return torch.relu(z + 0.3).contiguous()


def embed_case(name):
    """(z, W, bias, cls, pos) of an embedding case, seeded; W as nn.Linear draws it."""
    N, C, T, V, p1, p2, E = EMBED_CASES[name]
    K, n = p1 * p2 * C, (T // p1) * (V // p2)
    g = torch.Generator().manual_seed(5000 + K + n)
    z = make_input(N, C, T, V, seed=5001 + n)
    W = (torch.rand(E, K, generator=g) * 2 - 1) / K ** 0.5
    bias = (torch.rand(E, generator=g) * 2 - 1) / K ** 0.5
    return z, W, bias, torch.randn(E, generator=g), 0.5 * torch.randn(n + 1, E, generator=g)


def patches64(z, p1, p2):
    """(N, n, K) in fp64: token a w + b, element (f p2 + j) C + c."""
    N, C, T, V = z.shape
    h, w = T // p1, V // p2
    return z.double().reshape(N, C, h, p1, w, p2).permute(0, 2, 4, 3, 5, 1).reshape(N, h * w, p1 * p2 * C)


def embed64(z, W, bias, cls, pos, p1, p2):
    """x (N, n + 1, E) in fp64; ``bias`` / ``pos`` may be None."""
    x = patches64(z, p1, p2) @ W.double().T
    if bias is not None:
        x = x + bias.double()
    x = torch.cat((cls.double().reshape(1, 1, -1).expand(x.shape[0], 1, -1), x), dim=1)
    return x if pos is None else x + pos.double().reshape(1, -1, x.shape[2])[:, :x.shape[1]]


def _block_state(sd, i):
    p = f"transformer.layers.{i}."
    return {"norm1.weight": sd[p + "0.norm.weight"], "norm1.bias": sd[p + "0.norm.bias"],
            "attn.qkv.weight": sd[p + "0.fn.to_qkv.weight"], "attn.proj.weight": sd[p + "0.fn.to_out.0.weight"],
            "attn.proj.bias": sd[p + "0.fn.to_out.0.bias"], "norm2.weight": sd[p + "1.norm.weight"],
            "norm2.bias": sd[p + "1.norm.bias"], "mlp.fc1.weight": sd[p + "1.fn.net.0.weight"],
            "mlp.fc1.bias": sd[p + "1.fn.net.0.bias"], "mlp.fc2.weight": sd[p + "1.fn.net.3.weight"],
            "mlp.fc2.bias": sd[p + "1.fn.net.3.bias"]}


def vit64(z, sd, p1, p2, depth, heads, pool="cls", dim_head=DIM_HEAD):
    """(logits, embedding output) in fp64 from a ViT state_dict."""
    x0 = embed64(z, sd["to_patch_embedding.1.weight"], sd["to_patch_embedding.1.bias"], sd["cls_token"], sd["pos_embedding"][0],
                 p1, p2)
    x = x0
    for i in range(depth):
        x, _ = ar.block64(x, _block_state(sd, i), heads=heads, scale=dim_head ** -0.5, eps=LN_EPS)
    pooled = x.mean(dim=1) if pool == "mean" else x[:, 0]
    ln = ar.layer_norm64(pooled, sd["mlp_head.0.weight"].double(), sd["mlp_head.0.bias"].double(), LN_EPS)
    return ln @ sd["mlp_head.1.weight"].double().T + sd["mlp_head.1.bias"].double(), x0
