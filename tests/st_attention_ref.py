"""fp64 restatement of ST-TR's spatial attention unit (gcn_unit_attention in the reference scripts' configuration), written
from the math, plus the seeded parameter / input recipe the fixtures of tests/golden/make_golden_st_attention.py use.

    xn = data_bn(x)  (BatchNorm1d over channel c*V + v of the (N, C*V, T) view)
    qkv = Wqkv xn + b per frame; q *= dkh^-0.5; w = softmax over keys of q_h^T k_h  (drop-connect: w*m / (sum + 1e-8))
    o = heads of w v_h^T;  z = Wout o + bout (+ x when Cin == Cout);  y = relu(BatchNorm2d(z))
"""
import torch
import torch.nn.functional as TF

NH = 8
EPS = 1e-5
MOMENTUM = 0.1


def unit_kwargs(num_point, drop_connect=True, Nh=NH):
    """What model/ST_TR/ST_TR_new.py:344-352 passes in every reference script (attention=True, STR configuration); ``Nh``
    other than the scripts' 8 for the edge tests."""
    return dict(dv_factor=0.25, dk_factor=0.25, Nh=Nh, complete=True, relative=False, only_attention=True, layer=0,
                bn_flag=True, last_graph=False, more_channels=False, drop_connect=drop_connect, adjacency=False, num=4,
                data_normalization=True, skip_conn=True, visualization=False, num_point=num_point)


def layout(cin, cout, V):
    """state_dict keys and shapes in the reference's order."""
    dk = cout // 4
    out = []
    for pre, C in (("data_bn.", cin * V), ("bn.", cout)):
        out += [(pre + "weight", (C,)), (pre + "bias", (C,)), (pre + "running_mean", (C,)), (pre + "running_var", (C,)),
                (pre + "num_batches_tracked", ())]
    out += [("attention_conv.qkv_conv.weight", (2 * dk + cout, cin, 1, 1)), ("attention_conv.qkv_conv.bias", (2 * dk + cout,)),
            ("attention_conv.attn_out.weight", (cout, cout, 1, 1)), ("attention_conv.attn_out.bias", (cout,))]
    return out


def make_state(cin, cout, V, seed, sharp=1.0):
    """Seeded values for every key (CPU generator: the same numbers on every machine).  ``sharp`` multiplies the q and k rows
    of ``qkv_conv.weight`` (the first 2*dk): the logits grow with its square."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in layout(cin, cout, V):
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3, dtype=torch.long)
        elif k.endswith("running_var"):
            sd[k] = torch.rand(shape, generator=g) * 1.5 + 0.25
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(shape, generator=g) * 0.3
        elif "bn." in k and k.endswith("weight"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        elif "bn." in k:
            sd[k] = torch.randn(shape, generator=g) * 0.2
        elif k.endswith("weight"):
            sd[k] = torch.randn(shape, generator=g) / shape[1] ** 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    if sharp != 1.0:
        sd["attention_conv.qkv_conv.weight"][:2 * (cout // 4)] *= sharp
    return sd


def make_input(N, cin, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, cin, T, V, generator=g) * 0.8 + 0.2


def forward64(sd, x, training, mask=None, nh=NH, eps=EPS, momentum=MOMENTUM, aux=None):
    """y and the updated running statistics {key: tensor}; differentiable in x and in the floating entries of ``sd``.
    ``aux`` (a dict) receives the logits (B, nh, V, V) and z, the input of the last BatchNorm."""
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
    qkv = torch.einsum("oc,bcv->bov", Wq, xa) + sd["attention_conv.qkv_conv.bias"].view(1, -1, 1)
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
    ao = (torch.einsum("oc,bcv->bov", Wo, o) + sd["attention_conv.attn_out.bias"].view(1, -1, 1))
    ao = ao.reshape(N, T, cout, V).permute(0, 2, 1, 3)
    z = ao + x if C == cout else ao
    pre = bn(z, "bn.", (0, 2, 3))
    if aux is not None:
        aux["logits"], aux["pre"] = logits.detach(), pre.detach()
    return torch.relu(pre), new


def grads64(sd, x, dy, training=True, mask=None, nh=NH, dtype=torch.float64, aux=None):
    """(y, running statistics, {key: grad} of the floating parameters, dx), all in ``dtype`` (fp64; fp32 runs the same code
    as a statement of what plain fp32 arithmetic gives on these inputs)."""
    sd64 = {k: (v.to(dtype).clone().requires_grad_(not (k.endswith("running_mean") or k.endswith("running_var")))
                if v.is_floating_point() else v) for k, v in sd.items()}
    x64 = x.to(dtype).clone().requires_grad_(True)
    y, new = forward64(sd64, x64, training, None if mask is None else mask.to(dtype), nh=nh, aux=aux)
    y.backward(dy.to(dtype))
    g = {k: v.grad for k, v in sd64.items() if isinstance(v, torch.Tensor) and v.grad is not None}
    return y.detach(), new, g, x64.grad


# ---- the edges of what the kernels cover (tests/test_st_attention_edges_{host,gpu}.py) ----------------------------------------
# mode: "batch" = .train() (batch statistics), "frozen" = .train() with both BatchNorms in .eval() (running statistics, the
# drop-connect mask still drawn), "eval" = .eval() under no_grad.  N*T = 2 with batch statistics is left out on purpose:
# data_bn normalises two values to +-1 there, and plain fp32 alone is 1.4e-4 off on dx.
_EDGE_FIELDS = ("name", "N", "cin", "cout", "T", "V", "nh", "mode", "drop", "sharp", "seed")
EDGE_CASES = [dict(zip(_EDGE_FIELDS, row)) for row in [
    ("v64_skip",    2, 128,  128,  3, 64,  8, "batch",  True,  1.0, 101),   # no idle lane, skip connection
    ("v1",          3,   5,  128,  4,  1,  8, "batch",  True,  1.0, 102),   # one joint, K = 5, all-zero mask blocks
    ("v2_cin3",     4,   3,  256,  5,  2,  8, "batch",  True,  1.0, 103),   # (8,32) widths, K = 3, T*V = 10
    ("v3_cin1",     4,   1,  128,  3,  3,  8, "batch",  True,  1.0, 121),   # K = 1 (seed: 14 of 96 mask blocks all zero)
    ("n16",        16,   4,  128,  2,  5,  8, "batch",  True,  1.0, 105),   # 16 splits of one clip
    ("n17",        17,   8,  128,  2,  7,  8, "batch",  True,  1.0, 106),   # per = 2: 9 splits used, 7 empty
    ("n33",        33,   4,  128,  1,  5,  8, "batch",  True,  1.0, 107),   # per = 3: 11 used, 5 empty; T = 1
    ("chunks",      5,   8,  128, 40, 46,  8, "batch",  True,  1.0, 108),   # 9200 elements per channel: two BatchNorm chunks
    ("h4_c64",      3,  16,   64,  4,  9,  4, "batch",  True,  1.0, 109),   # (4,16) at 4 heads
    ("h16_c256",    3,  16,  256,  4,  9, 16, "batch",  True,  1.0, 110),   # (4,16) at 16 heads
    ("h1_c16",      3,  16,   16,  4,  9,  1, "batch",  True,  1.0, 111),   # (4,16), one head, skip connection
    ("h2_c128",     3,   7,  128,  4,  9,  2, "batch",  True,  1.0, 112),   # (16,64) at 2 heads
    ("h16_c1024",   2,   9, 1024,  2,  5, 16, "batch",  True,  1.0, 113),   # (16,64) at 16 heads
    ("h4_c128",     3,  16,  128,  4,  9,  4, "batch",  True,  1.0, 119),   # (8,32) at 4 heads
    ("sharp",       2,  64,  128,  6, 22,  8, "batch",  False, 6.0, 114),   # logits past fp32 exp's overflow without the max
    ("sharp_mask",  2,  64,  128,  6, 22,  8, "batch",  True,  6.0, 114),
    ("frozen_mask", 2, 131,  128,  6, 22,  8, "frozen", True,  1.0, 115),   # frozen-BatchNorm fine-tuning
    ("eval_v1",     1,   5,  128,  1,  1,  8, "eval",   False, 1.0, 116),   # N*T = 1, one joint
    ("eval_h1_v64", 1,   1,   16,  1, 64,  1, "eval",   False, 1.0, 117),   # one head, full wave, K = 1
    ("eval_v64",    2, 128,  128,  3, 64,  8, "eval",   False, 1.0, 118),
    ("eval_tv3",    1,   3,  128,  1,  3,  8, "eval",   False, 1.0, 120),   # T*V = 3, K = 3
]]
EXP_OVERFLOW_F32 = 88.8          # exp(x) overflows fp32 above 88.72: a soft-max without the row maximum gives inf / inf


def edge_case(name):
    return next(c for c in EDGE_CASES if c["name"] == name)


def edge_inputs(c):
    """(state_dict, x, dy, mask or None) of an EDGE_CASES entry: seeded on the CPU, the mask one Bernoulli(0.5) draw of
    N*T*nh*V elements as the module's."""
    sd = make_state(c["cin"], c["cout"], c["V"], c["seed"], sharp=c["sharp"])
    x = make_input(c["N"], c["cin"], c["T"], c["V"], c["seed"] + 1)
    dy = torch.randn(c["N"], c["cout"], c["T"], c["V"], generator=torch.Generator().manual_seed(c["seed"] + 3))
    mask = None
    if c["drop"]:
        g = torch.Generator().manual_seed(c["seed"] + 2)
        mask = torch.bernoulli(0.5 * torch.ones(c["N"] * c["T"] * c["nh"] * c["V"]), generator=g)
    return sd, x, dy, mask


def edge_grads(c, dtype=torch.float64, aux=None):
    """grads64 of an EDGE_CASES entry ("eval": running statistics, as "frozen")."""
    sd, x, dy, mask = edge_inputs(c)
    return grads64(sd, x, dy, training=c["mode"] == "batch", mask=mask, nh=c["nh"], dtype=dtype, aux=aux)
