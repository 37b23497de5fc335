"""fp64 emulation of the heads' bf16 block mode (``VIT_BF16``): ``altformer_ref.block64`` with a round-to-nearest-even bf16
rounding at exactly the points the mode's contract names (include/stgcn_hip.h, DESIGN section 14 "bf16"), everything else
fp64.

    a    = r(LN1(x));   qkv = r(a r(Wqkv)^T + bqkv)                              (qkv is stored as bf16)
    s    = scale * q k^T;   p = exp(s - max s);   out = r((r(p) v) / sum p)      (the row sum adds the UNROUNDED p)
    x1   = x + out r(Wproj)^T + bproj
    h    = r(GELU(r(LN2(x1)) r(W1)^T + b1));   y = x1 + h r(W2)^T + b2

r(t) = ``t.float().bfloat16().double()``.  Products of two bf16 values are exact in fp32 and in fp64, so the emulation differs
from the kernels only by the order of the fp32 sums, the fp32 LayerNorm / GELU / exp, and the rare value that these move across
a bf16 rounding boundary.
"""
import math

import torch

import altformer_ref as ar


def r(t):
    """Round to nearest-even bf16 (through fp32, as the kernels see the value), back in fp64."""
    return t.float().bfloat16().double()


def linear_bf16_64(x, W, bias=None, ln=None, residual=None, gelu=False, y_bf16=False):
    """The bf16 linear on fp64: ``x`` is fp32-valued (rounded here, after the LayerNorm) or already bf16-valued."""
    x = x.double()
    if ln is not None:
        x = ar.layer_norm64(x, ln[0].double(), ln[1].double(), ln[2])
    y = r(x) @ r(W.double()).T
    if bias is not None:
        y = y + bias.double()
    if gelu:
        y = 0.5 * y * (1 + torch.erf(y / math.sqrt(2.0)))
    if residual is not None:
        y = y + residual.double()
    return r(y) if y_bf16 else y


def attention_bf16_64(qkv, heads, scale, round_out=True):
    """qkv (B, L, 3*D) holding bf16 values -> (B, L, D); p rounded as the operand of P V, the row sum over the unrounded p."""
    B, L, D3 = qkv.shape
    hd = D3 // 3 // heads
    t = qkv.double().reshape(B, L, 3, heads, hd)
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    o = torch.einsum("bhij,bjhd->bihd", r(p), v) / p.sum(dim=-1).permute(0, 2, 1).unsqueeze(-1)
    o = o.reshape(B, L, heads * hd)
    return r(o) if round_out else o


def block_bf16_64(x, sd, heads=ar.HEADS, scale=None, eps=ar.EPS):
    """The bf16 mode of one block from its state_dict; returns (y, {"qkv", "att", "x1", "hid"})."""
    p = {k: v.double() for k, v in sd.items()}
    x = x.double()
    D = x.shape[-1]
    scale = scale or (D // heads) ** -0.5
    qkv = linear_bf16_64(x, p["attn.qkv.weight"], p.get("attn.qkv.bias"), ln=(p["norm1.weight"], p["norm1.bias"], eps), y_bf16=True)
    att = attention_bf16_64(qkv, heads, scale)
    x1 = linear_bf16_64(att, p["attn.proj.weight"], p["attn.proj.bias"], residual=x)
    hid = linear_bf16_64(x1, p["mlp.fc1.weight"], p["mlp.fc1.bias"], ln=(p["norm2.weight"], p["norm2.bias"], eps), gelu=True,
                         y_bf16=True)
    y = linear_bf16_64(hid, p["mlp.fc2.weight"], p["mlp.fc2.bias"], residual=x1)
    return y, {"qkv": qkv, "att": att, "x1": x1, "hid": hid}


def head_logits_bf16_64(head, z):
    """Logits of an ``ST`` / ``TS`` head on the stem output ``z`` with every block run through ``block_bf16_64`` and everything
    else (embeddings, pooling, ``mlp_head``) in fp64: what the whole model computes under ``set_head_math(model, 'bf16')`` up
    to fp32 rounding.  The head is left as it was found."""
    import copy
    from stgcn_amd.altformer import Block
    h64 = copy.deepcopy(head).double().eval()
    for m in h64.modules():
        if isinstance(m, Block):
            m.forward = (lambda blk: lambda x: block_bf16_64(x, blk.state_dict(), heads=blk.attn.num_heads, scale=blk.attn.scale,
                                                             eps=blk.norm1.eps)[0])(m)
    with torch.no_grad():
        return h64(z.double())


def whole_model_emulation(style):
    """max|logit error| / max|logit| of the emulated bf16 mode through a whole head of the fixture model (8 clips, oracle stem on
    the CPU) against the fixture's logits, the clips' arg max, and the fixture's top-two margins."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "st-gcn-altformer_amd"), os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import stgcn_amd
    from _util import load_golden, sub_state
    from oracle import stgcn_oracle as so
    g = load_golden("model_altformer_shre")
    torch.manual_seed(int(g["model_seed"]))
    model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style, graph="graph.SHRE",
                                       graph_args={"labeling_mode": "spatial"})
    gp = so.agcn_params_from_state(sub_state(g, "gcn."), torch.from_numpy(g["A_fixed"]))
    tp = so.tcn_params_from_state(sub_state(g, "tcn."))
    z = so.stem_forward(torch.from_numpy(g["skeleton"]).permute(0, 3, 1, 2).contiguous(), gp, tp).float()
    logits = head_logits_bf16_64(model.modelA if style == "ST" else model.modelB, z)
    want = torch.from_numpy(g[f"logits_{style}"]).double()
    return ((logits - want).abs().max() / want.abs().max()).item(), logits.argmax(1).numpy(), g[f"argmax_{style}"], g[f"margin_{style}"]


if __name__ == "__main__":      # the constants of tests/test_altformer_bf16_gpu.py::WHOLE_MODEL_EMULATION
    for _style in ("ST", "TS"):
        _rel, _am, _want_am, _margin = whole_model_emulation(_style)
        print(f"{_style}: max|logit error| / max|logit| = {_rel:.3e}; arg max equal: {bool((_am == _want_am).all())}; "
              f"margins {sorted(float(m) for m in _margin)}")
