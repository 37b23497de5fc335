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


def unit_kwargs(num_point, drop_connect=True):
    """What model/ST_TR/ST_TR_new.py:344-352 passes in every reference script (attention=True, STR configuration)."""
    return dict(dv_factor=0.25, dk_factor=0.25, Nh=NH, complete=True, relative=False, only_attention=True, layer=0,
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


def make_state(cin, cout, V, seed):
    """Seeded values for every key (CPU generator: the same numbers on every machine)."""
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
    return sd


def make_input(N, cin, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, cin, T, V, generator=g) * 0.8 + 0.2


def forward64(sd, x, training, mask=None, nh=NH, eps=EPS, momentum=MOMENTUM):
    """y and the updated running statistics {key: tensor}; differentiable in x and in the floating entries of ``sd``."""
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
    w = TF.softmax(torch.einsum("bhdi,bhdj->bhij", q, k), dim=-1)
    if mask is not None:
        w = w * mask.reshape(B, nh, 1, V).to(w.dtype)
        w = w / (w.sum(3, keepdim=True) + 1e-8)
    o = torch.einsum("bhij,bhej->bhei", w, v).reshape(B, cout, V)
    ao = (torch.einsum("oc,bcv->bov", Wo, o) + sd["attention_conv.attn_out.bias"].view(1, -1, 1))
    ao = ao.reshape(N, T, cout, V).permute(0, 2, 1, 3)
    z = ao + x if C == cout else ao
    y = torch.relu(bn(z, "bn.", (0, 2, 3)))
    return y, new


def grads64(sd, x, dy, training=True, mask=None):
    """(y, running statistics, {key: grad} of the floating parameters, dx), all fp64."""
    sd64 = {k: (v.double().clone().requires_grad_(not (k.endswith("running_mean") or k.endswith("running_var")))
                if v.is_floating_point() else v) for k, v in sd.items()}
    x64 = x.double().clone().requires_grad_(True)
    y, new = forward64(sd64, x64, training, None if mask is None else mask.double())
    y.backward(dy.double())
    g = {k: v.grad for k, v in sd64.items() if isinstance(v, torch.Tensor) and v.grad is not None}
    return y.detach(), new, g, x64.grad
