"""GPU tests of the AltFormer heads' HIP path: the linear and attention entry points against fp64, one block against the
reference's fixture cases (tests/golden/make_golden_altformer.py) and the fp64 restatement (tests/altformer_ref.py), and the
whole model from skeleton clips to class indices against the reference's logits (tests/golden/model_altformer_shre.npz)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF
from torch.nn.parallel import parallel_apply

import altformer_ref as ar
from _util import MATH_GATES, gather_flat, load_golden, parity_gate, sub_state
from entry_points import peaked_qkv, small_head

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]            # the project's 1e-4, both criteria, for f32 and for bf16x3
assert MATH_GATES["bf16x3"] == (REL, True) and MATH_GATES["f32"][1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref():
    return load_golden("altformer_reference")


def gate_on_device(out, want, rel, what):
    """parity_gate's two criteria, evaluated where the tensors are (the large linears: 200 M elements per case)."""
    out = out.double()
    assert out.shape == want.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(want.shape)}"
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    scale = want.abs().max().item()
    err = (out - want).abs().max().item()
    print(f"{what}: max|err|/max|ref| = {err / scale:.3e}")
    assert err <= rel * scale, f"{what}: max abs err {err:.3e} > {rel:g} * max|ref| ({scale:.3e})"
    assert torch.allclose(out, want, rtol=rel, atol=rel * 0.1 * scale), f"{what}: allclose(rtol={rel}) failed"


# ---- 5. the linear ------------------------------------------------------------------------------------------------------
# (M, K, Nout) of the four linears at every stage of the heads, batch 32: ST spatial (SHREC 32 x 180 x 22 tokens, DHG
# 32 x 150 x 22), ST temporal (32 x 180, 32 x 150), TS temporal (32 x 46 x 180), TS spatial (32 x 46, 32 x 22); then M off the
# 128-row tile, M = 1, and an Nout off the tile.
LINEAR_SHAPES = [(126720, 256, 768), (126720, 256, 256), (126720, 256, 512), (126720, 512, 256), (105600, 256, 768),
                 (5760, 512, 1536), (5760, 512, 512), (5760, 512, 1024), (5760, 1024, 512), (4800, 512, 1536),
                 (264960, 256, 768), (264960, 512, 256), (1472, 512, 1536), (1472, 1024, 512), (704, 512, 1024),
                 (1000, 256, 768), (129, 512, 512), (1, 512, 1536), (1, 256, 256), (300, 256, 200)]


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_entry_point_vs_fp64(shape, math, dev):
    """Every (LayerNorm, GELU, residual, bias) combination against fp64 torch on the CPU (the two matrix products; the
    elementwise epilogue of the reference value is applied to them in fp64 on the device)."""
    from stgcn_amd import functional as F
    M, K, Nout = shape
    g = torch.Generator().manual_seed(M + K + Nout)
    x = torch.randn(M, K, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    W = (torch.rand(Nout, K, generator=g) * 2 - 1) / K ** 0.5
    b = torch.randn(Nout, generator=g) * 0.5
    R = torch.randn(M, Nout, generator=g)
    lw, lb = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    xn = TF.layer_norm(x.double(), (K,), lw.double(), lb.double(), ar.EPS)
    base = {False: (x.double() @ W.double().T).to(dev), True: (xn @ W.double().T).to(dev)}
    del xn
    xd, Wd, bd, Rd, lwd, lbd = (t.to(dev) for t in (x, W, b, R, lw, lb))
    mode = getattr(F, "MATH_" + math.upper())
    for ln, gelu, res, bias in itertools.product((False, True), repeat=4):
        want = base[ln] + (bd.double() if bias else 0)
        if gelu:
            want = TF.gelu(want)
        if res:
            want = want + Rd.double()
        y = F.vit_linear(xd, Wd, bd if bias else None, ln=(lwd, lbd, ar.EPS) if ln else None, residual=Rd if res else None,
                         gelu=gelu, math=mode)
        gate_on_device(y, want, REL, f"linear {shape} {math} ln={ln} gelu={gelu} residual={res} bias={bias}")


# ---- 6. the attention ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [1, 22, 46, 64, 65, 150, 180, 256])
def test_attention_entry_point_vs_fp64(L, hd, dev):
    from stgcn_amd import functional as F
    B, heads = 9, 8
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd)
    want = ar.attention64(qkv, heads, hd ** -0.5)
    out = F.vit_attention(qkv.to(dev), heads)
    print(f"attention L={L} hd={hd}: {parity_gate(out, want, REL, f'attention L={L} hd={hd}'):.3e}")
    out2 = F.vit_attention(qkv.to(dev), heads, scale=0.37)
    parity_gate(out2, ar.attention64(qkv, heads, 0.37), REL, f"attention L={L} hd={hd} scale=0.37")


@pytest.mark.parametrize("L,hd", [(22, 32), (180, 64)])
def test_attention_subtracts_the_row_maximum(L, hd, dev):
    """Scores that reach +-80 and beyond: exp() of them overflows fp32, the result is finite only with the max subtraction."""
    from stgcn_amd import functional as F
    heads = 8
    qkv = peaked_qkv(5, L, heads, hd, 7, amp=5.0)
    t = qkv.reshape(5, L, 3, heads, hd)
    s = torch.einsum("bihd,bjhd->bhij", t[:, :, 0], t[:, :, 1]) * hd ** -0.5
    assert s.max().item() > 89 and s.min().item() < -89, (s.min().item(), s.max().item())   # exp(89) > fp32 max
    out = F.vit_attention(qkv.to(dev), heads)
    parity_gate(out, ar.attention64(qkv, heads, hd ** -0.5), REL, f"attention with +-{s.abs().max().item():.0f} scores")


# ---- 7. one block -------------------------------------------------------------------------------------------------------
def gate_case(out, ref, key, what):
    got = gather_flat(out.detach().cpu(), ref[key + "_idx"].astype(np.int64))
    rel = parity_gate(got, ref[key + "_val"], REL, what)
    print(f"{what}: {rel:.3e}")


@pytest.mark.parametrize("mode", ["f32", "default"])
@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_vs_reference_case(name, mode, ref, dev):
    """The reference's output and its three intermediates.  The block entry point keeps its intermediates in its workspace, so
    they are taken from the same kernels through the entry points it is made of: LN1(x) as the fused LayerNorm + linear with
    an identity weight, the attention output from the qkv linear + attention, the first residual from the proj linear."""
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH, Block, _default_head_math, set_head_math
    B, L, D, qkv_bias, qk_scale, seed = ar.BLOCK_CASES[name]
    pre = f"case.{name}."
    x = ar.make_input(name)
    assert torch.equal(gather_flat(x, ref[pre + "x_idx"].astype(np.int64)), torch.from_numpy(ref[pre + "x_val"]))
    blk = ar.build_block(Block, name).to(dev)
    flags = _default_head_math() if mode == "default" else HEAD_MATH[mode]
    set_head_math(blk, None if mode == "default" else mode)
    xd = x.to(dev)
    with torch.no_grad():
        blk.hip_min_tokens = 0
        assert blk.uses_hip(xd)
        y = blk(xd)
        gate_case(y, ref, pre + "y", f"{name} {mode} y")
        math, math_qkv = flags & F._capi.MATH_MASK, (F.MATH_F32 if flags & F._capi.VIT_QKV_F32 else flags & F._capi.MATH_MASK)
        norm1 = (blk.norm1.weight, blk.norm1.bias, ar.EPS)
        ln1 = F.vit_linear(xd, torch.eye(D, device=dev), None, ln=norm1, math=math_qkv)
        gate_case(ln1, ref, pre + "ln1", f"{name} {mode} LN1(x)")
        att = F.vit_attention(F.vit_linear(xd, blk.attn.qkv.weight, blk.attn.qkv.bias, ln=norm1, math=math_qkv),
                              blk.attn.num_heads, blk.attn.scale)
        gate_case(att, ref, pre + "att", f"{name} {mode} attention output")
        x1 = F.vit_linear(att, blk.attn.proj.weight, blk.attn.proj.bias, residual=xd, math=math)
        gate_case(x1, ref, pre + "x1", f"{name} {mode} first residual")


# (B, L, D, heads, hidden, qkv_bias): sequence lengths at the edges of the tiles, head_dim 64 at D = 256, mlp_ratio 4 and 1
FREE_SHAPES = [(5, 256, 256, 8, 512, True), (3, 65, 512, 8, 1024, True), (7, 1, 256, 8, 512, True), (40, 64, 512, 8, 1024, False),
               (6, 33, 256, 4, 1024, True), (4, 129, 512, 16, 512, True), (1600, 22, 256, 8, 512, True)]


@pytest.mark.parametrize("mode", ["f32", "default"])
@pytest.mark.parametrize("shape", FREE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_vs_fp64_restatement(shape, mode, dev):
    from stgcn_amd.altformer import Block, set_head_math
    B, L, D, heads, hidden, qkv_bias = shape
    sd = ar.random_block_state(D, hidden, qkv_bias, seed=B + L + D)
    blk = Block(D, heads, mlp_ratio=hidden / D, qkv_bias=qkv_bias, norm_layer=ar.norm_layer())
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).eval()
    set_head_math(blk, None if mode == "default" else mode)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    want, _ = ar.block64(x, sd, heads=heads)
    blk.hip_min_tokens = 0
    with torch.no_grad():
        assert blk.uses_hip(x.to(dev))
        y = blk(x.to(dev))
    print(f"block {shape} {mode}: {parity_gate(y, want, REL, f'block {shape} {mode}'):.3e}")


# ---- 8. the whole model -------------------------------------------------------------------------------------------------
def whole_model(style, dev, mode="default", layout="contiguous", policy="hip"):
    import stgcn_amd
    g = load_golden("model_altformer_shre")
    torch.manual_seed(int(g["model_seed"]))
    model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style, graph="graph.SHRE",
                                       graph_args={"labeling_mode": "spatial"})
    model.gcn0.load_state_dict(sub_state(g, "gcn."), strict=True)
    model.tcn0.load_state_dict(sub_state(g, "tcn."), strict=True)
    model = model.to(dev).eval()
    model.gcn0.A = torch.from_numpy(g["A_fixed"]).clone()       # plain CPU attribute, like the reference's self.A
    if mode != "default":
        stgcn_amd.set_math_mode(model, mode)
    stgcn_amd.set_output_layout(model, layout)
    if policy == "hip":                                         # every block on the kernels, however few tokens the call has
        stgcn_amd.set_hip_min_tokens(model, 0)
    return model, g


@pytest.mark.parametrize("policy", ["hip", "default"])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("mode", ["default", "f32"])
@pytest.mark.parametrize("style", ["ST", "TS", None])
def test_whole_model_logits_and_argmax(style, mode, layout, policy, dev):
    """Skeleton clips -> class indices on the GPU, against the reference model's logits.  1e-4 of max|logit| (1.03 for ST) moves
    a difference of two logits by at most 2.1e-4, under the smallest top-1 / top-2 margin of the fixture (9.0e-4, ST clip 7),
    so the first assertion implies the second; both are made.  policy 'hip': every block on the kernels; 'default': as a user
    gets it (with 8 clips the second stage of each head is under HIP_MIN_TOKENS and takes its torch path)."""
    from stgcn_amd.altformer import Block
    model, g = whole_model(style, dev, mode, layout, policy)
    calls = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: calls.append(mod.uses_hip(args[0])))
             for m in model.modules() if isinstance(m, Block)]
    x = torch.from_numpy(g["skeleton"]).to(dev)
    with torch.no_grad():
        logits = model(x).cpu()
    for h in hooks:
        h.remove()
    assert len(calls) == (24 if style is None else 12)
    assert all(calls) if policy == "hip" else sum(calls) == len(calls) // 2, "blocks on the HIP path"
    if style is None:
        want = g["logits_ST"].astype(np.float64) + g["logits_TS"].astype(np.float64)
    else:
        want = g[f"logits_{style}"]
    rel = parity_gate(logits, want, REL, f"whole model {style} {mode} {layout}")
    print(f"whole model style={style} {mode} {layout}: max|err|/max|logit| = {rel:.3e}")
    if style is not None:
        assert float(g[f"margin_{style}"].min()) > 2.1 * REL * float(np.abs(want).max())
        assert np.array_equal(logits.argmax(1).numpy(), g[f"argmax_{style}"])
    else:
        assert np.array_equal(logits.argmax(1).numpy(), want.argmax(1))


# ---- 9. paths, determinism, replicas ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_two_runs_are_bit_identical_and_match_the_torch_path(cls_name, dev):
    from stgcn_amd.altformer import Block
    head = small_head(dev, cls_name)
    z = torch.randn(6, 128, 40, 22, device=dev)
    with torch.no_grad():
        a, b = head(z), head(z)
        assert torch.equal(a, b), "two runs of the HIP path differ"
        for m in head.modules():
            if isinstance(m, Block):
                m.force_torch = True
        t = head(z)
    print(f"{cls_name}: HIP vs torch path {parity_gate(a, t, REL, f'{cls_name} HIP path vs the module torch path'):.3e}")


def test_block_bit_identical_at_batch_size(dev):
    from stgcn_amd.altformer import Block
    blk = ar.build_block(Block, "st_spatial_L22_D256").to(dev)
    x = torch.randn(3000, 22, 256, device=dev)            # more than one slab of the block entry point
    with torch.no_grad():
        assert blk.uses_hip(x) and not blk.uses_hip(x[:100]) and blk.hip_applies(x[:100])   # the default policy
        assert torch.equal(blk(x), blk(x))


def test_autograd_takes_the_torch_path_and_fills_every_grad(dev):
    head = small_head(dev, "ST")
    z = torch.randn(2, 128, 40, 22, device=dev, requires_grad=True)
    blocks = list(head.Spatial_blocks) + list(head.blocks)
    assert not any(b.hip_applies(torch.zeros(2, 22, b.norm1.normalized_shape[0], device=dev)) for b in blocks), \
        "parameters require gradients and autograd is recording: the torch path"
    with torch.no_grad():
        assert all(b.hip_applies(torch.zeros(2, 22, b.norm1.normalized_shape[0], device=dev)) for b in blocks)
        want = head(z)
    out = head(z)                                         # .eval() with gradients
    parity_gate(out, want, REL, "torch path under autograd vs HIP path")
    out.sum().backward()
    unused = ("Spatial_cls_token", "cls_token", "Spatial_norm.", "Temporal_norm.", "weighted_mean.", "fcn.")
    for k, p in head.named_parameters():
        assert (p.grad is not None) != k.startswith(unused), k
    assert z.grad is not None and z.grad.abs().sum().item() > 0
    head.train()
    assert head(z.detach()).shape == (2, 14)              # training mode (stochastic depth draws): torch path, no error


def test_uncovered_shape_takes_the_torch_path(dev):
    from stgcn_amd.altformer import Block
    torch.manual_seed(2)
    blk = Block(384, 8, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer()).to(dev).eval()     # head_dim 48
    x = torch.randn(4, 22, 384, device=dev)
    with torch.no_grad():
        assert not blk.hip_applies(x)
        y = blk(x)
    want, _ = ar.block64(x.cpu(), {k: v.cpu() for k, v in blk.state_dict().items()}, heads=8)
    parity_gate(y, want, REL, "head_dim 48 on the torch path")
    cpu = Block(256, 8, mlp_ratio=2., qkv_bias=True).eval()
    with torch.no_grad():
        assert not cpu.hip_applies(torch.randn(2, 22, 256)) and cpu(torch.randn(2, 22, 256)).shape == (2, 22, 256)


def test_replicas_give_the_masters_result(dev):
    from test_data_parallel import _replicas
    head = small_head(dev, "ST")
    z = torch.randn(8, 128, 40, 22, device=dev)
    halves = [(z[:4],), (z[4:],)]
    with torch.no_grad():
        want = [head(h) for (h,) in halves]
        for _ in range(2):                                # replicas are new objects with fresh parameter clones on every call
            got = parallel_apply(_replicas(head, 2), halves, devices=[dev, dev])   # one thread per replica
            for o, w in zip(got, want):
                assert torch.equal(o, w)
        dp = nn.DataParallel(head, device_ids=[dev.index or 0])
        assert torch.equal(dp(z), head(z))
