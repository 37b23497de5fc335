"""fp64 emulation of the training attention on bf16 matrix operands (``VIT_TRAIN_ATTN_BF16``, include/stgcn_hip.h, DESIGN
section 15 "bf16 attention"): ``altformer_ref.attention64`` as an ``autograd.Function`` that rounds to nearest-even bf16 (r) at
exactly the points the contract names, everything else in the dtype of its input (fp64; ``dtype=torch.float32`` runs the same
emulation in fp32 torch ops on the CPU, the stand-in for the kernels' fp32 noise).

    forward   s = scale * (qh kh^T + qh kl^T + ql kh^T),  qh = r(q), ql = r(q - qh), kh, kl alike         (scores="x3")
              p = exp(s - max s),  l = sum p,  out = (r(p) r(v)) / l                                       p_fwd, v_fwd
    backward  P = p / l recomputed,  dP = r(dO) r(v)^T                                                     do_dp, v_dp
              delta = sum_j P dP  (delta="pdp"; "rowsum": rowsum(dO * out)),  dS = P (dP - delta)
              dV = r(P)^T r(dO)                                                                            p_dv, do_dv
              dQ = scale r(dS) r(k)                                                                        ds_dq, k_dq
              dK = scale r(dS)^T r(q)                                                                      ds_dk, q_dk

``POINTS`` names the ten rounding points, ``skip`` leaves one out; ``scores``: "x3" (the contract), "bf16" (q and k rounded
once: what the inference kernel does) or "exact"; ``fwd_exact``: the forward unrounded, the backward as chosen.
``block_grads`` runs ``altformer_bf16_train_ref.grads_bf16`` (the bf16 linears of ``HEAD_TRAIN_MATH['bf16']``) with this
attention in place of its ``attention``.

    python tests/altformer_bf16_attn_ref.py        reprints the tables of DESIGN section 15 "bf16 attention"
"""
import contextlib

import torch

import altformer_bf16_train_ref as br
import altformer_ref as ar
import altformer_train_ref as tr

POINTS = ("p_fwd", "v_fwd", "do_dp", "v_dp", "p_dv", "do_dv", "ds_dq", "k_dq", "ds_dk", "q_dk")
SCORES = ("exact", "x3", "bf16")
TENSORS = ("out", "dq", "dk", "dv")

# ---- what the GPU tests hold the kernels to (tests/test_altformer_bf16_attn_gpu.py), taken from this emulation alone --------
# Attention alone, ||candidate - emulation|| / ||emulation - fp64|| per tensor of out, dq, dk, dv, on the qkv of the six block
# cases (tests/test_altformer_bf16_attn_host.py measures both ends again and asserts that they bracket the bound):
#   an fp32 torch run of the emulation stays within FP32_RUN_L2 of it (measured 0.001 - 0.039, worst tensor per case; in the
#   max norm it reaches 0.53, which is why the bound is an L2 one);
#   leaving one rounding point out moves the most affected tensor by at least LEAVE_ONE_OUT_L2 (measured 0.225 - 0.289 without
#   p_fwd, on `out`; 0.49 - 0.97 without any of the nine others); plain-bf16 scores move every tensor by 2.3 or more.
# The bound is the geometric mean of the two measured ends, sqrt(0.039 * 0.225) = 0.094, rounded to 0.1.
FP32_RUN_L2 = 0.05
LEAVE_ONE_OUT_L2 = 0.22
ATTN_L2_BOUND = 0.10
# One block (bf16 linears in place, every gradient tensor): the fp32 run of the emulation is 0.26 - 0.39 away, more than a
# missing weak point of the attention moves a tensor there, so the block-level bound is twice the fp32 run's and catches
# gross errors only (plain-bf16 scores, a wrong delta, a missing scale).
BLOCK_FP32_RUN_L2 = 0.40
BLOCK_L2_BOUND = 0.80
# ||emulation - fp64|| / ||fp64|| per tensor: the largest the host test measures over the inputs of the GPU test
# (attention_cases below), rounded up.  The kernels stay within (1 + ATTN_L2_BOUND) times this of the fp64 attention.
EMULATION_DISTANCE = {"out": 2.3e-3, "dq": 3.7e-3, "dk": 3.6e-3, "dv": 2.6e-3}   # measured 2.24e-3, 3.62e-3, 3.50e-3, 2.56e-3


def r(t):
    return br.r(t)


def split(t):
    hi = r(t)
    return hi, r(t - hi)


def _scores(q, k, scale, mode):
    """(B, H, L, L) scores of q, k (B, L, H, hd)."""
    def prod(a, b):
        return torch.einsum("bihd,bjhd->bhij", a, b)
    if mode == "exact":
        return prod(q, k) * scale
    if mode == "bf16":
        return prod(r(q), r(k)) * scale
    if mode == "x3":
        qh, ql = split(q)
        kh, kl = split(k)
        return (prod(qh, kh) + prod(qh, kl) + prod(ql, kh)) * scale
    raise KeyError(mode)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, scale, scores, delta, skip, fwd_exact):
        B, L, D3 = qkv.shape
        hd = D3 // 3 // heads
        t = qkv.reshape(B, L, 3, heads, hd)
        q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]

        def rr(x, point):
            return x if skip in (point, "all") else r(x)
        s = _scores(q, k, scale, "exact" if fwd_exact else scores)
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        l = p.sum(dim=-1, keepdim=True)
        if fwd_exact:
            out = torch.einsum("bhij,bjhd->bihd", p / l, v)
        else:
            out = torch.einsum("bhij,bjhd->bihd", rr(p, "p_fwd"), rr(v, "v_fwd")) / l.permute(0, 2, 1, 3)
        ctx.save_for_backward(qkv, out)
        ctx.cfg = (heads, scale, scores, delta, rr)
        return out.reshape(B, L, heads * hd)

    @staticmethod
    def backward(ctx, dout):
        qkv, out = ctx.saved_tensors
        heads, scale, scores, delta, rr = ctx.cfg
        B, L, D3 = qkv.shape
        hd = D3 // 3 // heads
        t = qkv.reshape(B, L, 3, heads, hd)
        q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
        dO = dout.reshape(B, L, heads, hd)
        s = _scores(q, k, scale, scores)
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        P = p / p.sum(dim=-1, keepdim=True)
        dP = torch.einsum("bihd,bjhd->bhij", rr(dO, "do_dp"), rr(v, "v_dp"))
        if delta == "pdp":
            dl = (P * dP).sum(dim=-1, keepdim=True)
        elif delta == "rowsum":
            dl = (dO * out).sum(dim=-1).permute(0, 2, 1).unsqueeze(-1)
        else:
            raise KeyError(delta)
        dS = P * (dP - dl)
        dV = torch.einsum("bhij,bihd->bjhd", rr(P, "p_dv"), rr(dO, "do_dv"))
        dQ = scale * torch.einsum("bhij,bjhd->bihd", rr(dS, "ds_dq"), rr(k, "k_dq"))
        dK = scale * torch.einsum("bhij,bihd->bjhd", rr(dS, "ds_dk"), rr(q, "q_dk"))
        return torch.stack((dQ, dK, dV), dim=2).reshape(B, L, D3), None, None, None, None, None, None


def attention(qkv, heads, scale, scores="x3", delta="pdp", skip=None, fwd_exact=False):
    """The contract's attention on a packed qkv (B, L, 3 * heads * hd), differentiable; the keywords choose a variant."""
    return _Attention.apply(qkv, heads, scale, scores, delta, skip, fwd_exact)


def attention_grads(qkv, dout, heads, scale, dtype=torch.float64, **variant):
    """{"out", "dq", "dk", "dv"} of the emulation (a variant of it) as fp64 tensors; dq, dk, dv as (B, L, heads * hd)."""
    qkv = qkv.detach().to(dtype).requires_grad_(True)
    out = attention(qkv, heads, scale, **variant)
    out.backward(dout.to(dtype))
    B, L, D3 = qkv.shape
    g = qkv.grad.double().reshape(B, L, 3, D3 // 3)
    return {"out": out.detach().double(), "dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}


def attention_grads64(qkv, dout, heads, scale):
    """The same four tensors of the unrounded fp64 attention (altformer_ref.attention64 under autograd)."""
    qkv = qkv.detach().double().requires_grad_(True)
    out = ar.attention64(qkv, heads, scale)
    out.backward(dout.double())
    B, L, D3 = qkv.shape
    g = qkv.grad.reshape(B, L, 3, D3 // 3)
    return {"out": out.detach(), "dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}


@contextlib.contextmanager
def in_block(**variant):
    """``altformer_bf16_train_ref.block_train_bf16`` with this module's attention in place of its own."""
    old = br.attention
    br.attention = lambda qkv, heads, scale: attention(qkv, heads, scale, **variant)
    try:
        yield
    finally:
        br.attention = old


def block_grads(x, sd, dy, scale=None, s1=None, s2=None, dtype=torch.float64, **variant):
    """(y, gradients) of one block: the bf16 linears of the training mode and this attention (a variant of it)."""
    with in_block(**variant):
        return br.grads_bf16(x, sd, dy, scale=scale, s1=s1, s2=s2, dtype=dtype)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def derived_qkv(name, B=None, L=None, heads=None, seed_offset=0):
    """fp32 qkv (B, L, 3 * heads * hd) as the qkv linear of a block case writes it (LN1, then the linear, in fp64), with a
    seeded dout (B, L, heads * hd) and the block's scale: scores of 25 - 45.  Without B / L / heads: the case's own input;
    with them: an input drawn by altformer_ref.make_input's recipe in that shape, and the first ``heads`` heads."""
    from stgcn_amd.altformer import Block
    B0, L0, D, _, _, seed = ar.BLOCK_CASES[name]
    blk = ar.build_block(Block, name)
    sd = {k: v.double() for k, v in blk.state_dict().items()}
    if B is None and L is None:
        x = ar.make_input(name)
    else:
        g = torch.Generator().manual_seed(seed + 101 + seed_offset)
        B, L = B or B0, L or L0
        x = torch.randn(B, L, D, generator=g)
        x = x * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    qkv = ar.layer_norm64(x.double(), sd["norm1.weight"], sd["norm1.bias"]) @ sd["attn.qkv.weight"].T
    if "attn.qkv.bias" in sd:
        qkv = qkv + sd["attn.qkv.bias"]
    B, L = x.shape[:2]
    hd = D // ar.HEADS
    heads = heads or ar.HEADS
    qkv = qkv.reshape(B, L, 3, ar.HEADS, hd)[:, :, :, :heads].reshape(B, L, 3 * heads * hd).float().contiguous()
    dout = torch.randn(B, L, heads * hd, generator=torch.Generator().manual_seed(seed + 55 + seed_offset))
    return qkv, dout, heads, blk.attn.scale


def random_qkv(B, L, heads, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, 3 * heads * hd, generator=g), torch.randn(B, L, heads * hd, generator=g), heads, hd ** -0.5


# The inputs of the GPU test of the two kernels alone, shared with the host test that measures EMULATION_DISTANCE on them.
# Lengths: one key, the stages' 22 / 46 / 180, both sides of every tile edge (32 | 33, 64 | 65: the workgroup packs 4, 2, 1
# pairs), the longest (255, 256: eight tiles, at hd = 64 the split backward).  "derived": 3 sequences x 3 heads of a block
# case's qkv (9 pairs: no multiple of what a workgroup packs); "random": one sequence, 3 heads, standard normal; "edge": a
# sequence whose keys are all equal, one whose key 5 outweighs the others by e^-250 (their p underflow to 0), one ordinary.
ATTN_LENGTHS = (1, 22, 32, 33, 46, 64, 65, 180, 255, 256)
DERIVED_FROM = {32: "st_spatial_L22_D256", 64: "ts_spatial_L46_D512"}
ATTN_CASES = [(kind, L, hd) for hd in (32, 64) for L in ATTN_LENGTHS for kind in ("derived", "random")] + \
             [("edge", 46, 32), ("edge", 46, 64)]


def attention_case(kind, L, hd):
    """(qkv, dout, heads, scale) of one entry of ATTN_CASES."""
    if kind == "derived":
        return derived_qkv(DERIVED_FROM[hd], B=3, L=L, heads=3, seed_offset=L)
    if kind == "random":
        return random_qkv(1, L, 3, hd, 7000 + L + hd)
    qkv, dout, heads, scale = random_qkv(3, L, 3, hd, 7700 + hd)
    t = qkv.reshape(3, L, 3, heads, hd)
    t[0, :, 1] = t[0, :1, 1]                 # sequence 0: every key is key 0
    t[1, :, 0, :, 0] = 8.0                   # sequence 1: q . k_5 is about 1600 larger than any other q . k
    t[1, :, 1, :, 0] = 0.0
    t[1, 5, 1, :, 0] = 200.0
    return qkv, dout, heads, scale


def l2_rel(got, want):
    got, want = (torch.as_tensor(t).double().cpu() for t in (got, want))
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()


# ---- the tables ---------------------------------------------------------------------------------------------------------------
BLOCK_VARIANTS = (
    ("scores plain bf16, delta = rowsum(dO out)", dict(scores="bf16", delta="rowsum")),
    ("scores x3, delta = rowsum(dO out)", dict(scores="x3", delta="rowsum")),
    ("scores x3, delta = sum P dP (the contract)", dict()),
    ("forward exact, backward as the contract", dict(fwd_exact=True)),
)


def worst(g, g64):
    return max(br.max_rel(g[k], g64[k]) for k in g64)


def block_table(names=None):
    rows = {}
    for name in names or sorted(ar.BLOCK_CASES):
        x, sd, dy, scale, s1, s2 = br.case_inputs(name, True)
        kw = dict(scale=scale, s1=s1, s2=s2)
        y64, g64 = tr.grads64(x, sd, dy, **kw)
        rows.setdefault("fp64 attention (the mode without the switch, emulated)", []).append(worst(br.grads_bf16(x, sd, dy, **kw)[1], g64))
        for tag, variant in BLOCK_VARIANTS:
            y, g = block_grads(x, sd, dy, **kw, **variant)
            rows.setdefault(tag, []).append(worst(g, g64))
            if not variant:
                rows.setdefault("y of the contract", []).append(br.max_rel(y, y64))
                yf, gf = block_grads(x, sd, dy, dtype=torch.float32, **kw)
                keys = [k for k in g if k not in br.EXACT_IN_EMULATION]
                rows.setdefault("fp32 run of the contract, worst L2 ratio", []).append(max(br.l2_ratio(gf[k], g[k], g64[k]) for k in keys))
    return rows


def attention_table(names=None):
    """Per case: the fp32 run's worst L2 and max-norm ratio, the most affected tensor's L2 ratio without each point, and the
    smallest L2 ratio over the tensors with plain-bf16 scores."""
    rows = []
    for name in names or sorted(ar.BLOCK_CASES):
        qkv, dout, heads, scale = derived_qkv(name)
        g64 = attention_grads64(qkv, dout, heads, scale)
        ge = attention_grads(qkv, dout, heads, scale)
        gf = attention_grads(qkv, dout, heads, scale, dtype=torch.float32)
        row = {"case": name,
               "fp32_l2": max(br.l2_ratio(gf[t], ge[t], g64[t]) for t in TENSORS),
               "fp32_max": max(br.max_ratio(gf[t], ge[t], g64[t]) for t in TENSORS),
               "dist": {t: l2_rel(ge[t], g64[t]) for t in TENSORS}}
        for point in POINTS:
            gs = attention_grads(qkv, dout, heads, scale, skip=point)
            row[point] = max(br.l2_ratio(gs[t], ge[t], g64[t]) for t in TENSORS)
        gb = attention_grads(qkv, dout, heads, scale, scores="bf16")
        row["scores_bf16"] = min(br.l2_ratio(gb[t], ge[t], g64[t]) for t in TENSORS)
        rows.append(row)
    return rows


if __name__ == "__main__":
    import os
    import sys
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(_here), "st-gcn-altformer_amd"))
    print("block level, six cases with factors, worst gradient tensor relative to max|fp64|:")
    for _tag, _vals in block_table().items():
        print(f"  {_tag}: {min(_vals):.2e} - {max(_vals):.2e}   [{' '.join(f'{v:.2e}' for v in _vals)}]")
    print("attention level, L2 ratio ||candidate - emulation|| / ||emulation - fp64||, worst of out, dq, dk, dv:")
    _rows = attention_table()
    for _r in _rows:
        print(f"  {_r['case']}: fp32 run L2 {_r['fp32_l2']:.3f} (max norm {_r['fp32_max']:.3f}); plain-bf16 scores, least moved "
              f"tensor {_r['scores_bf16']:.2f}; emulation vs fp64 (rel. L2) " + " ".join(f"{t} {_r['dist'][t]:.2e}" for t in TENSORS))
        print("      without " + "  ".join(f"{p} {_r[p]:.3f}" for p in POINTS))
    print(f"largest fp32-run ratio {max(r_['fp32_l2'] for r_ in _rows):.3f}, smallest leave-one-out ratio "
          f"{min(r_[p] for r_ in _rows for p in POINTS):.3f}, bound {ATTN_L2_BOUND}")
