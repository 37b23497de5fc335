"""GPU parity tests (run with ``-m gpu`` on an MI355X): HIP path vs golden fixtures and the CPU oracle.

Gate (north_star): fp32 within 1e-4 relative — ``max|out-ref| <= 1e-4*max|ref|`` and
``allclose(rtol=1e-4, atol=1e-5*max|ref|)``.  Every call goes through the C ABI
(stgcn_amd.functional -> ctypes -> libstgcn_hip.so); the oracle is only the checker.
"""
import numpy as np
import pytest
import torch

from _util import MATH_GATES, gather_flat, load_golden, parity_gate, sub_state
from _util import grad_gate as _grad_gate, kink_free_cotangent as _kink_free_cotangent
from entry_points import (agcn_compare_grads as _compare_grads, agcn_module_grads as _agcn_module_grads,
                          agcn_oracle_leaves as _agcn_oracle_leaves, random_stem as _random_stem)

pytestmark = pytest.mark.gpu

GCN_CASES = {  # name -> (cin, cout)
    "gcn_shre_3_128_quirk": (3, 128), "gcn_shre_3_128_trueA": (3, 128),
    "gcn_shre_3_128_default_init": (3, 128), "gcn_lmdhg_3_128": (3, 128),
    "gcn_shre_64_64_identity": (64, 64), "gcn_shre_64_128": (64, 128),
}
TCN_CASES = {  # name -> (cin, cout, K, stride, bias)
    "tcn_128_128_k9": (128, 128, 9, 1, True), "tcn_64_128_k9_s2": (64, 128, 9, 2, True),
    "tcn_64_128_k1_s2": (64, 128, 1, 2, True), "tcn_128_128_k9_v46": (128, 128, 9, 1, True),
    "tcn_32_64_k5_nobias": (32, 64, 5, 1, False),
}
STEM_CASES = ["stem_shre_T180", "stem_lmdhg_T200", "stem_shre_T500"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def build_gcn(g, cin, cout, dev):
    from stgcn_amd import unit_agcn
    m = unit_agcn(cin, cout, torch.from_numpy(g["A_true"]).clone() if "A_true" in g
                  else torch.zeros_like(torch.from_numpy(g["A_fixed"])))
    m.load_state_dict(sub_state(g, "gcn."), strict=True)
    m = m.to(dev).eval()
    m.A = torch.from_numpy(g["A_fixed"]).clone()       # plain CPU attribute, like the reference's self.A
    return m


def build_tcn(g, cin, cout, K, stride, bias, dev, math="f32"):
    from stgcn_amd import Unit2D, set_math_mode
    m = Unit2D(cin, cout, kernel_size=K, stride=stride, bias=bias)
    m.load_state_dict(sub_state(g, "tcn."), strict=True)
    m = m.to(dev).eval()
    set_math_mode(m, math)
    return m


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(GCN_CASES))
def test_agcn_vs_golden(case, dev):
    g = load_golden(case)
    cin, cout = GCN_CASES[case]
    m = build_gcn(g, cin, cout, dev)
    with torch.no_grad():
        y = m(torch.from_numpy(g["x"]).to(dev))
    parity_gate(m.last_attention, g["P_eval"], 1e-4, f"{case} P")
    parity_gate(y, g["y_eval"], 1e-4, f"{case} y")


def test_agcn_T180_samples(dev):
    g = load_golden("gcn_shre_3_128_T180")
    m = build_gcn(g, 3, 128, dev)
    with torch.no_grad():
        y = m(torch.from_numpy(g["x"]).to(dev)).cpu()
    parity_gate(m.last_attention, g["P_eval"], 1e-4, "P")
    scale = float(g["y_eval_absmax"])
    err = (gather_flat(y, g["y_eval_idx"]).double() - torch.from_numpy(g["y_eval_val"]).double()).abs().max().item()
    assert err <= 1e-4 * scale
    assert float(y.double().sum()) == pytest.approx(float(g["y_eval_sum"]), rel=1e-4)


@pytest.mark.parametrize("math", ["f32", "f32_valu", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", sorted(TCN_CASES))
def test_tcn_vs_golden(case, math, dev):
    g = load_golden(case)
    cin, cout, K, stride, bias = TCN_CASES[case]
    m = build_tcn(g, cin, cout, K, stride, bias, dev, math)
    with torch.no_grad():
        y = m(torch.from_numpy(g["x"]).to(dev))
    rel, strict = MATH_GATES[math]
    parity_gate(y, g["y_eval"], rel, f"{case} {math}", strict)


def test_tcn_one_shot_entry_point(dev):
    """stgcn_tcn_forward (pack + run in one call) agrees with the packed path."""
    from stgcn_amd import functional as F
    g = load_golden("tcn_128_128_k9")
    m = build_tcn(g, 128, 128, 9, 1, True, dev)
    st = m._staged(dev)
    x = torch.from_numpy(g["x"]).to(dev)
    y = F.tcn_forward(x, st["W"], st["scale"], st["shift"], 1, F.MATH_F32)
    parity_gate(y, g["y_eval"], 1e-4, "one-shot")


@pytest.mark.parametrize("math", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_vs_golden(case, fused, math, dev):
    from stgcn_amd import enable_stem_fusion
    g = load_golden(case)
    rel, strict = MATH_GATES[math]
    gcn = build_gcn(g, 3, 128, dev)
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev, math)
    if fused:
        enable_stem_fusion(gcn, tcn)
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2).contiguous()   # ST_GCN_AltFormer.py:64-68
    with torch.no_grad():
        y = gcn(x)
        z = tcn(y)
    if fused:
        assert z.data_ptr() == y.data_ptr() and type(z) is torch.Tensor, "fused stem must hand tcn0 its own output"
    parity_gate(gcn.last_attention, g["P_eval"], 1e-4, "P")
    checks = [("z", z)] if fused else [("y", y), ("z", z)]
    for nm, arr in checks:
        arr = arr.cpu()
        scale = float(g[f"{nm}_eval_absmax"])
        err = (gather_flat(arr, g[f"{nm}_eval_idx"]).double()
               - torch.from_numpy(g[f"{nm}_eval_val"]).double()).abs().max().item()
        assert err <= rel * scale, f"{case} {nm} {math}: {err:.3e} vs {scale:.3e}"
        assert float(arr.double().sum()) == pytest.approx(float(g[f"{nm}_eval_sum"]), rel=rel, abs=10 * rel * scale)
        assert float((arr.double() ** 2).sum()) == pytest.approx(float(g[f"{nm}_eval_sumsq"]), rel=2 * rel)


# ---------------------------------------------------------------------------------------
# seeded comparisons against the oracle at shapes the fixtures do not hold (ragged tiles, odd V)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("N,T,V", [(3, 37, 22), (2, 9, 46), (1, 5, 22), (2, 64, 25), (1, 1, 22), (2, 23, 7), (1, 30, 64)])
@pytest.mark.parametrize("fused", [False, True])
def test_stem_vs_oracle_ragged(N, T, V, fused, math, dev):
    from stgcn_amd import enable_stem_fusion, set_math_mode
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 100 + T + V, dev)
    set_math_mode(tcn, math)
    if fused:
        enable_stem_fusion(gcn, tcn)
    x = torch.randn(N, 3, T, V, generator=gen)
    aux = {}
    ref = so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64), aux=aux)
    with torch.no_grad():
        y = gcn(x.to(dev))
        z = tcn(y)
    parity_gate(gcn.last_attention, aux["gcn"]["P"], 1e-4, "P")
    if not fused:
        parity_gate(y, aux["gcn_out"], 1e-4, "gcn out")
    parity_gate(z, ref, 1e-4, "stem out")


@pytest.mark.parametrize("cin,cout,K,stride,T,V", [
    (128, 128, 9, 1, 41, 22), (64, 128, 9, 2, 40, 22), (128, 256, 9, 2, 33, 22), (256, 256, 9, 1, 12, 46),
    (16, 128, 3, 1, 7, 22), (48, 96, 9, 1, 20, 22), (128, 128, 1, 1, 30, 22), (64, 64, 9, 1, 25, 22),
    (128, 128, 4, 1, 19, 22), (64, 128, 6, 2, 20, 22),       # even K: Tout = (T + 2*((K-1)//2) - K)//stride + 1
    (64, 64, 9, 1, 180, 22), (32, 64, 9, 2, 31, 25), (64, 64, 1, 1, 9, 46), (128, 64, 3, 1, 14, 22),    # 64 output channels:
    (32, 128, 9, 1, 23, 22), (32, 64, 9, 1, 40, 25), (256, 128, 9, 1, 17, 22)])   # K3v6 with one period per tile / eight
    # packed as 128 rows for the bf16 matrix-core kernels (tcn_bf16.hip), rows >= 64 never stored
@pytest.mark.parametrize("math", ["f32", "bf16x3"])
def test_tcn_vs_oracle_shapes(cin, cout, K, stride, T, V, math, dev):
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    gen = torch.Generator().manual_seed(cin + cout + K + T)
    torch.manual_seed(5)
    m = Unit2D(cin, cout, kernel_size=K, stride=stride)
    with torch.no_grad():
        m.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
        m.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        m.bn.running_mean.copy_(torch.randn(cout, generator=gen) * 0.3)
        m.bn.running_var.copy_(torch.rand(cout, generator=gen) + 0.25)
    tp = so.tcn_params_from_state(m.state_dict(), stride=stride).to(torch.float64)
    x = torch.randn(2, cin, T, V, generator=gen)
    ref = so.tcn_forward(x.double(), tp)
    m = m.to(dev).eval()
    set_math_mode(m, math)
    with torch.no_grad():
        y = m(x.to(dev))
    parity_gate(y, ref, 1e-4, f"tcn {cin}->{cout} K{K} s{stride} {math}")


@pytest.mark.parametrize("cin,cout,K,stride,N,T,V", [(32, 128, 3, 1, 2, 10, 22), (3, 70, 9, 1, 3, 7, 46), (16, 16, 5, 2, 2, 5, 25),
                                                     (8, 40, 1, 1, 1, 300, 3)])
def test_unit2d_dim3(cin, cout, K, stride, N, T, V, dev):
    """dim=3 (model/net.py:28-36: conv along the joints) = the same op on the (T,V)-transposed tensor.  Inference reads x in
    place (STGCN_CONV_ALONG_V, plain-FMA kernel — round 2 transposed into a copy and back); with batch statistics the module
    still runs the frame-axis kernels on a transposed copy (no model builds either)."""
    from stgcn_amd import Unit2D
    from oracle import stgcn_oracle as so
    torch.manual_seed(9 + K)
    m = Unit2D(cin, cout, kernel_size=K, stride=stride, dim=3)
    with torch.no_grad():
        m.bn.running_mean.normal_(0, 0.3); m.bn.running_var.uniform_(0.5, 2.0); m.bn.weight.uniform_(0.5, 1.5); m.bn.bias.normal_(0, 0.2)
    x = torch.randn(N, cin, T, V)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["conv.weight"] = sd["conv.weight"].permute(0, 1, 3, 2)        # (Cout,Cin,1,K) -> (Cout,Cin,K,1)
    tp = so.tcn_params_from_state(sd, stride=stride).to(torch.float64)
    ref = so.tcn_forward(x.double().transpose(2, 3), tp).transpose(2, 3)
    m = m.to(dev)
    with torch.no_grad():
        y = m.eval()(x.to(dev))
    assert y.shape == ref.shape and y.is_contiguous()
    parity_gate(y, ref, 1e-4, "dim=3, inference")
    with torch.no_grad():
        yt = m.train()(x.to(dev))
    ref_t = so.tcn_forward(x.double().transpose(2, 3), tp, training=True).transpose(2, 3)
    parity_gate(yt, ref_t, 1e-4, "dim=3, batch statistics")


# ---------------------------------------------------------------------------------------
# full-size properties: every BASELINE.json config at its full size
#   configs[1] N=256,T=180,V=22 · configs[2] N=512,T=500,V=22 · configs[3] N=256,T=200,V=46 (LMDHG)
#   configs[4] the per-rank shard at 8 GPUs: N=1024,T=180,V=22 (8192 clips / 8)
# ---------------------------------------------------------------------------------------
FULL_SIZE = {"configs1": (256, 180, 22, "SHRE"), "configs2": (512, 500, 22, "SHRE"),
             "configs3": (256, 200, 46, "LMDHG"), "configs4_shard": (1024, 180, 22, "SHRE")}


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("cfg", sorted(FULL_SIZE))
def test_full_size_properties(cfg, math, dev):
    """Size-independent properties at the full BASELINE sizes (the oracle cannot run these in seconds):
    clip independence and batch-permutation equivariance bit for bit, fused == two-stage on a 32-clip slice,
    five sampled clips (first / last / middle / two more) against the fp64 oracle at 1e-4."""
    from stgcn_amd import enable_stem_fusion, disable_stem_fusion, set_math_mode
    from stgcn_amd.graphs import LMDHGGraph, SHREGraph
    from oracle import stgcn_oracle as so
    N, T, V, graph = FULL_SIZE[cfg]
    A = torch.from_numpy((SHREGraph if graph == "SHRE" else LMDHGGraph)("spatial").A.astype(np.float32))
    gcn, tcn, gp, tp, gen = _random_stem(V, A, 77, dev)
    set_math_mode(tcn, math)
    x = torch.randn(N, T, V, 3, generator=gen).permute(0, 3, 1, 2).contiguous()
    xd = x.to(dev)
    sel = sorted({0, N // 3, N // 2, N - 2, N - 1})
    lo = N // 2 - 16
    with torch.no_grad():
        z_two = tcn(gcn(xd[lo:lo + 32].contiguous()))
        enable_stem_fusion(gcn, tcn)
        z_fused = tcn(gcn(xd))
        # clip independence: clips computed alone equal the same clips inside the batch, bit for bit
        z_sel = tcn(gcn(xd[sel].contiguous()))
        assert torch.equal(z_sel, z_fused[sel])
        # batch permutation equivariance
        perm = torch.randperm(N, generator=gen).to(dev)
        z_perm = tcn(gcn(xd[perm].contiguous()))
        assert torch.equal(z_perm, z_fused[perm])
        del z_perm
        disable_stem_fusion(gcn)
    assert z_fused.shape == (N, 128, T, V)
    assert torch.isfinite(z_fused).all()
    assert (z_fused >= 0).all()
    parity_gate(z_fused[lo:lo + 32], z_two, 1e-5 if math == "f32" else 1e-4, f"{cfg} fused vs two-stage")
    ref = so.stem_forward(x[sel].double(), gp.to(torch.float64), tp.to(torch.float64))
    parity_gate(z_fused[sel], ref, 1e-4, f"{cfg} full-size clips vs oracle")


@pytest.mark.parametrize("math", ["f32", "bf16x3", "f16mx"])
def test_whole_model_stem_output_and_argmax_handoff(math, dev):
    """north_star's argmax clause, GPU half.  The fixture (tests/golden/make_golden_model.py) holds the reference
    ST_GCN_AltFormer's stem parameters, 8 skeleton clips, samples of the reference stem output z and the logits / argmax
    of both transformer heads.  Here: z from the fused HIP stem is gated at 1e-4 against the reference's z and written
    to gpurun_out/argmax/ — tools/argmax_check.py (build container, where the reference's heads can be imported) feeds
    that file through the heads and asserts the class indices are identical (recorded in profiles/)."""
    import os
    from stgcn_amd import enable_stem_fusion
    g = load_golden("model_altformer_shre")
    gcn = build_gcn(g, 3, 128, dev)
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev, math)
    enable_stem_fusion(gcn, tcn)
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2)       # the caller's permuted view, read in place
    with torch.no_grad():
        z = tcn(gcn(x)).cpu()
    scale = float(g["z_absmax"])
    err = (gather_flat(z, g["z_idx"]).double() - torch.from_numpy(g["z_val"]).double()).abs().max().item()
    assert err <= 1e-4 * scale, f"whole-model stem output {math}: {err:.3e} vs {scale:.3e}"
    parity_gate(z[0, :, :12], g["z_clip0"], 1e-4, "dense corner of clip 0", strict=False)
    assert float(z.double().sum()) == pytest.approx(float(g["z_sum"]), rel=1e-4)
    assert float((z.double() ** 2).sum()) == pytest.approx(float(g["z_sumsq"]), rel=2e-4)
    root = os.environ.get("GRAFT_REPO_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        d = os.path.join(root, "gpurun_out", "argmax")
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, f"z_gpu_{math}.npy"), z.numpy())
    except OSError:
        pass                                                              # read-only checkout: the gate above still ran


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("order", ["ST", "TS"])
def test_patch_embedding_vs_reference(order, layout, dev):
    """SURVEY §8(f)-1, third clause: rearrange + first nn.Linear(128->256) + position embedding of the transformer heads
    (model_ST.py:152-155 / model_TS.py:161-163) as ONE entry point on the stem output, against the reference's own
    rearrange / nn.Linear applied to the reference's stem output (fixture model_altformer_shre)."""
    from stgcn_amd import enable_stem_fusion, functional as F, set_output_layout
    g = load_golden("model_altformer_shre")
    gcn = build_gcn(g, 3, 128, dev)
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev, "bf16x3")
    enable_stem_fusion(gcn, tcn)
    set_output_layout(tcn, layout)
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2)
    W, b, pos = (torch.from_numpy(g[f"emb_{order}.{k}"]).to(dev) for k in ("weight", "bias", "pos"))
    with torch.no_grad():
        z = tcn(gcn(x))
        assert z.is_contiguous() == (layout == "contiguous")
        e = F.patch_embed(z, W, b, pos, order=order)
        ref_torch = torch.nn.functional.linear(z.permute(0, 2, 3, 1).reshape(-1, 22, 128) if order == "ST"
                                               else z.permute(0, 3, 2, 1).reshape(-1, 180, 128), W, b) + pos
    assert tuple(e.shape) == tuple(g[f"emb_{order}_shape"])
    scale = float(g[f"emb_{order}_absmax"])
    err = (gather_flat(e.cpu(), g[f"emb_{order}_idx"]).double() - torch.from_numpy(g[f"emb_{order}_val"]).double()).abs().max().item()
    assert err <= 1e-4 * scale, f"patch embedding {order}: {err:.3e} vs {scale:.3e}"
    assert float(e.double().sum()) == pytest.approx(float(g[f"emb_{order}_sum"]), rel=1e-4, abs=1e-3 * scale)
    parity_gate(e, ref_torch, 1e-5, "entry point vs torch ops on the same z", strict=False)   # same z: only fp32 reassociation
    e0 = F.patch_embed(z, W, b, None, order=order)                      # without the position embedding
    parity_gate(e0, ref_torch - pos, 1e-5, "no pos", strict=False)


def test_fused_stem_result_cannot_be_misused(dev):
    """With stem fusion gcn0 returns tcn0's result typed FusedStemOutput: only the paired Unit2D can take it; a forward
    hook / residual / cast on gcn0's return value fails loudly instead of reading the wrong activation."""
    from stgcn_amd import FusedStemOutput, Unit2D, disable_stem_fusion, enable_stem_fusion
    g = load_golden("stem_shre_T180")
    gcn = build_gcn(g, 3, 128, dev)
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev, "bf16x3")
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        y_plain = gcn(x)
        z_plain = tcn(y_plain)
        enable_stem_fusion(gcn, tcn)
        y = gcn(x)
        assert isinstance(y, FusedStemOutput) and y.shape == z_plain.shape and y.device == x.device
        for misuse in (lambda: y + 1, lambda: y.clone(), lambda: y.half(), lambda: torch.relu(y), lambda: y.cpu(),
                       lambda: y[:, :8], lambda: gcn(y), lambda: Unit2D(128, 128, 9).to(dev).eval()(y)):
            with pytest.raises(RuntimeError):
                misuse()
        z = tcn(y)
        assert type(z) is torch.Tensor
        parity_gate(z, z_plain, 1e-4, "fused vs two-stage")
        seen = []
        h = gcn.register_forward_hook(lambda m, i, o: seen.append(o.float().mean().item()))   # a feature-extraction hook
        with pytest.raises(RuntimeError):
            gcn(x)
        disable_stem_fusion(gcn)                    # the documented way to get gcn0's own activation
        assert torch.equal(gcn(x), y_plain) and len(seen) == 1
        h.remove()


def test_batchnorm_mode_follows_the_bn_submodules(dev):
    """model.train() followed by bn.eval() (frozen-BN fine-tuning) freezes the statistics in the reference
    (nn.BatchNorm2d looks at its own flag); same here; mixed modes are refused, eval-mode autograd is served."""
    g = load_golden("stem_shre_T180")
    gcn = build_gcn(g, 3, 128, dev)
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev, "f32")
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2).contiguous()[:, :, :24].contiguous()
    with torch.no_grad():
        ref = tcn(gcn(x))
        gcn.train(); tcn.train()
        for m in (gcn.bn, gcn.down[1], tcn.bn):
            m.eval()
        rm = tcn.bn.running_mean.clone()
        out = tcn(gcn(x))
        assert torch.equal(out, ref) and torch.equal(tcn.bn.running_mean, rm)
        gcn.bn.train()
        with pytest.raises(NotImplementedError):
            gcn(x)                                   # bn on batch statistics, down[1] frozen
        gcn.eval(); tcn.eval()
    out = tcn(gcn(x))                                # grad-enabled call through running-statistics BatchNorm: differentiable
    assert out.grad_fn is not None and torch.equal(tcn.bn.running_mean, rm)     # (test_eval_mode_backward_* check the values)
    parity_gate(out.detach(), ref, 1e-5, "eval mode under autograd vs inference kernels")
    for p in list(gcn.parameters()) + list(tcn.parameters()):
        p.requires_grad_(False)
    assert torch.equal(tcn(gcn(x)), ref)             # nothing wants a gradient: plain inference, no no_grad needed


def test_errors_are_loud(dev):
    from stgcn_amd import Unit2D, functional as F, StgcnError
    from stgcn_amd import unit_agcn
    m = Unit2D(8, 8, kernel_size=3).to(dev)
    g = unit_agcn(8, 8, torch.rand(3, 4, 4), coff_embedding=2).to(dev)
    with pytest.raises(NotImplementedError):
        g.train()(torch.zeros(1, 8, 4, 4, device=dev))   # autograd outside what the HIP backward covers (embedding wider
                                                         # than C_out/4): refused, not silently cut out of the graph
    with pytest.raises(RuntimeError):
        m.eval()(torch.zeros(1, 8, 4, 4))            # CPU tensor: no fallback
    with pytest.raises(ValueError):
        Unit2D(8, 8, kernel_size=3, dim=4)
    x = torch.zeros(1, 8, 4, 4, device=dev)
    with pytest.raises(StgcnError):                  # unknown arithmetic mode -> error, not a silent fallback
        F.tcn_forward_packed(x, torch.zeros(4096, device=dev, dtype=torch.uint8), torch.zeros(8, device=dev), 8, 3,
                             math=9)
    with pytest.raises(StgcnError):                  # fused stem asked for a shape it does not cover
        F.stem_forward(torch.zeros(1, 5, 4, 4, device=dev), torch.zeros(3, 4, 4, device=dev),
                       torch.zeros(3, 32, 5, device=dev), torch.zeros(3, 32, device=dev),
                       torch.zeros(3, 32, 5, device=dev), torch.zeros(3, 32, device=dev),
                       torch.zeros(1 << 20, device=dev, dtype=torch.uint8), torch.zeros(128, device=dev), 128, 9)
    with pytest.raises(StgcnError) as e:             # workspace too small is reported, not overrun
        from ctypes import c_int, c_size_t, c_uint, c_void_p
        from stgcn_amd import _capi
        z = torch.zeros(64, device=dev)
        _capi.call("stgcn_stem_attention", *[c_void_p(z.data_ptr())] * 7, c_size_t(16), c_int(4), c_int(3), c_int(128),
                   c_int(20), c_int(22), c_int(32), c_int(3), c_int(9), c_uint(0), c_void_p(0))
    assert e.value.code == -3


def test_stem_forward_prepared_entry_point(dev):
    """The one-call C entry (attention + fused kernel) agrees with the two-call path the wrapper uses."""
    from ctypes import c_int, c_uint, c_void_p
    from stgcn_amd import _capi, enable_stem_fusion
    g = load_golden("stem_shre_T180")
    gcn = build_gcn(g, 3, 128, dev)
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev)
    enable_stem_fusion(gcn, tcn)
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        ref = tcn(gcn(x))
    st, ts = gcn._staged(dev), tcn._staged(dev)
    out = torch.empty_like(ref)
    from ctypes import c_size_t
    lib = _capi.lib()
    nbytes = lib.stgcn_stem_ws_bytes(x.shape[0], 3, 128, 180, 22, 9, 3, 0)
    ws = torch.empty(nbytes // 4 + 1, device=dev)
    p = lambda t: c_void_p(t.data_ptr())
    _capi.call("stgcn_stem_forward_prepared", p(x), p(st["A_eff"]), p(st["Wa"]), p(st["ba"]), p(st["Wb"]), p(st["bb"]),
               p(st["stem_prep"]), p(ts["shift"]), p(ws), c_size_t(ws.numel() * 4), p(out), c_int(x.shape[0]), c_int(3),
               c_int(128), c_int(180), c_int(22), c_int(32), c_int(3), c_int(9), c_uint(0),
               c_void_p(torch.cuda.current_stream().cuda_stream))
    parity_gate(ws[:x.shape[0] * 3 * 22 * 22].view(-1, 3, 22, 22), gcn.last_attention, 1e-6, "P in workspace")
    assert torch.equal(out, ref)


def test_step_stats_kernel_matches_torch(dev):
    """stgcn_step_stats (the per-rank reduction that is all-reduced each step) equals the torch formulation."""
    from stgcn_amd import dist as sd
    gen = torch.Generator().manual_seed(5)
    out = torch.randn(37, 128, 6, 22, generator=gen).to(dev)
    got = sd.step_stats(out, 37).cpu()
    probe = out[:, :, 0, 0].double().cpu()
    ref = torch.tensor([37.0, probe.sum().item(), probe.square().sum().item(), 0.0], dtype=torch.float64)
    assert torch.allclose(got.double(), ref, rtol=1e-5, atol=1e-3)
    got16 = sd.step_stats(out.to(torch.bfloat16), 37).cpu()
    p16 = out.to(torch.bfloat16)[:, :, 0, 0].double().cpu()
    assert torch.allclose(got16[1:3].double(), torch.tensor([p16.sum().item(), p16.square().sum().item()], dtype=torch.float64),
                          rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("n,classes", [(8, 14), (300, 28), (1024, 14), (1, 2)])
def test_step_stats_argmax_is_numpy_argmax(n, classes, dev):
    """The correct-count of the HIP step_stats kernel == get_acc of train_sttran.py:105-109 (np.argmax on the host),
    bit-exact class indices including ties (lowest index), NaN rows and +-inf."""
    from stgcn_amd import dist as sd
    gen = torch.Generator().manual_seed(n + classes)
    logits = torch.randn(n, classes, generator=gen)
    logits = (logits * 4).round() / 4                       # quarter steps: plenty of exact ties
    if n >= 8:
        logits[1] = 0.0                                     # all equal -> class 0
        logits[2, classes - 1] = float("inf")
        logits[3, :] = float("-inf")                        # all -inf -> class 0
        logits[4, 1] = float("nan")                         # numpy: NaN is the maximum
        logits[5, 0] = logits[5].max()                      # tie with a later class -> the lower index
    want = np.argmax(logits.numpy(), axis=1)
    labels = torch.from_numpy(want.copy())
    flip = torch.rand(n, generator=gen) < 0.3
    labels[flip] = (labels[flip] + 1) % classes
    out = torch.randn(n, 4, 2, 3, generator=gen).to(dev)
    pred = torch.full((n,), -1, dtype=torch.int64, device=dev)
    stats = sd.step_stats(out, n, logits.to(dev), labels.to(dev), pred).cpu()
    assert np.array_equal(pred.cpu().numpy(), want)
    assert float(stats[3]) == float((torch.from_numpy(want) == labels).sum())
    assert float(stats[0]) == n
    cpu = sd.step_stats(out.cpu(), n, logits, labels)       # the torch formulation used by the gloo tests
    assert float(cpu[3]) == float(stats[3])


# ---------------------------------------------------------------------------------------
# training-mode forward (batch-statistics BatchNorm), against the reference's own train-mode outputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(GCN_CASES))
def test_agcn_train_forward_vs_golden(case, dev):
    g = load_golden(case)
    cin, cout = GCN_CASES[case]
    m = build_gcn(g, cin, cout, dev).train()
    with torch.no_grad():
        y = m(torch.from_numpy(g["x"]).to(dev))
    parity_gate(m.last_attention, g["P_train"], 1e-4, f"{case} P")
    parity_gate(y, g["y_train"], 1e-4, f"{case} y (train)")
    sd = m.state_dict()
    for k, v in g.items():
        if k.startswith("after_train.gcn."):
            name = k[len("after_train.gcn."):]
            if "num_batches" in name:
                assert int(sd[name]) == int(v)
            else:
                parity_gate(sd[name], v, 1e-4, f"{case} {name}")


@pytest.mark.parametrize("math", ["f32", "bf16x3", "f32_valu"])
@pytest.mark.parametrize("case", sorted(TCN_CASES))
def test_tcn_train_forward_vs_golden(case, math, dev):
    g = load_golden(case)
    cin, cout, K, stride, bias = TCN_CASES[case]
    m = build_tcn(g, cin, cout, K, stride, bias, dev, math).train()
    with torch.no_grad():
        y = m(torch.from_numpy(g["x"]).to(dev))
    parity_gate(y, g["y_train"], 1e-4, f"{case} {math} (train)")
    sd = m.state_dict()
    parity_gate(sd["bn.running_mean"], g["after_train.tcn.bn.running_mean"], 1e-4, "running_mean")
    parity_gate(sd["bn.running_var"], g["after_train.tcn.bn.running_var"], 1e-4, "running_var")
    assert int(sd["bn.num_batches_tracked"]) == int(g["after_train.tcn.bn.num_batches_tracked"])


def test_stem_train_forward_vs_golden(dev):
    g = load_golden("stem_shre_T180")
    gcn = build_gcn(g, 3, 128, dev).train()
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev).train()
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        z = tcn(gcn(x)).cpu()
    scale = float(g["z_train_absmax"])
    err = (gather_flat(z, g["z_train_idx"]).double() - torch.from_numpy(g["z_train_val"]).double()).abs().max().item()
    assert err <= 1e-4 * scale
    parity_gate(tcn.bn.running_var, g["after_train.tcn.bn.running_var"], 1e-4, "tcn running_var after one step")


def test_unsupported_backward_is_refused_loudly(dev):
    from stgcn_amd import Unit2D
    m = Unit2D(16, 128, kernel_size=9, dim=3).to(dev).train()   # dim=3 (transposed) has no HIP backward
    with pytest.raises(NotImplementedError, match="backward"):
        m(torch.zeros(1, 16, 22, 8, device=dev))          # grad enabled + trainable parameters


@pytest.mark.parametrize("N", [17, 33])
def test_persistent_kernel_uneven_tiles(N, dev):
    """More tiles than CUs but not a multiple (some workgroups of the persistent kernel loop twice, most once):
    the fused bf16x3 stem must equal the two-stage path and three of its clips the fp64 oracle."""
    from stgcn_amd import enable_stem_fusion
    from stgcn_amd.graphs import SHREGraph
    from oracle import stgcn_oracle as so
    A = torch.from_numpy(SHREGraph("spatial").A.astype(np.float32))
    gcn, tcn, gp, tp, gen = _random_stem(22, A, 300 + N, dev)
    x = torch.randn(N, 3, 180, 22, generator=gen)
    with torch.no_grad():
        two = tcn(gcn(x.to(dev)))
        enable_stem_fusion(gcn, tcn)
        fused = tcn(gcn(x.to(dev)))
    parity_gate(fused, two, 1e-4, "fused vs two-stage")
    sel = [0, N // 2, N - 1]
    ref = so.stem_forward(x[sel].double(), gp.to(torch.float64), tp.to(torch.float64))
    parity_gate(fused[sel], ref, 1e-4, "clips vs oracle")


@pytest.mark.parametrize("math,N,T,V", [("bf16", 40, 180, 22), ("bf16x3", 80, 300, 7), ("bf16x3", 48, 90, 25),
                                        ("bf16", 80, 300, 7),
                                        ("bf16x3", 24, 60, 46), ("bf16", 24, 60, 46), ("bf16x3", 30, 50, 30)])   # 128-pixel tile form
def test_persistent_kernel_many_tiles_small_images(math, N, T, V, dev):
    """Every workgroup of the persistent kernel runs several tiles at shapes whose LDS image buffers are smaller
    than at the BASELINE shape (narrow V, or one image per buffer in bf16 mode): the epilogue staging and the
    prefetched feature tile of the next tile must not overlap."""
    from stgcn_amd import enable_stem_fusion, set_math_mode
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 500 + N + V, dev)
    set_math_mode(tcn, math)
    x = torch.randn(N, 3, T, V, generator=gen)
    with torch.no_grad():
        two = tcn(gcn(x.to(dev)))
        enable_stem_fusion(gcn, tcn)
        fused = tcn(gcn(x.to(dev)))
    gate, strict = MATH_GATES[math]
    parity_gate(fused, two, 2 * gate, "fused vs two-stage", strict=False)
    sel = [0, 1, N // 2, N - 2, N - 1]
    ref = so.stem_forward(x[sel].double(), gp.to(torch.float64), tp.to(torch.float64))
    parity_gate(fused[sel], ref, gate, "clips vs oracle", strict=strict)


# ---------------------------------------------------------------------------------------
# SURVEY §8(f) rank 1 — layout fusion with the callers either side of the stem
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("math,N,T,V", [("bf16x3", 5, 60, 22),     # large-tile persistent kernel (features path)
                                        ("bf16x3", 40, 180, 22),   # ... several tiles per workgroup
                                        ("bf16", 3, 33, 25),
                                        ("bf16x3", 2, 40, 46),     # 128-pixel tile of the large-tile kernel (LMDHG graph)
                                        ("bf16x3", 24, 60, 46),    # ... several of them per workgroup
                                        ("bf16x3", 2, 2, 52),      # 128-pixel kernel KFb (only very wide, very short clips are left to it): reads the channel-major x copy
                                        ("f32", 3, 37, 22),        # fp32 matrix-core kernel
                                        ("f32", 2, 20, 46)])
@pytest.mark.parametrize("out_bf16", [False, True])
def test_stem_layout_fusion_is_bit_exact(math, N, T, V, out_bf16, dev):
    """STGCN_IN_NTVC / STGCN_OUT_NTVC change addressing only: reading the loader's (N,T,V,3) batch in place and
    writing (N,T,V,C) must give the same bits as the (N,C,T,V) call (ST_GCN_AltFormer.py:62-68, model_ST.py:152)."""
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 700 + T + V, dev)
    set_math_mode(tcn, math)
    tcn.out_bf16 = out_bf16
    enable_stem_fusion(gcn, tcn)
    batch = torch.randn(N, T, V, 3, generator=gen).to(dev)             # as the data loader delivers it
    x_view = batch.permute(0, 3, 1, 2)                                  # ST_GCN_AltFormer.py:64 (no copy)
    assert not x_view.is_contiguous()
    with torch.no_grad():
        base = tcn(gcn(x_view.contiguous()))                            # the reference's own call sequence (:68)
        P_base = gcn.last_attention.clone()
        z_in = tcn(gcn(x_view))                                         # permuted view read in place
        assert torch.equal(gcn.last_attention, P_base)
        assert torch.equal(z_in, base)
        set_output_layout(tcn, "channels_last")
        z_cl = tcn(gcn(x_view))
    assert z_cl.shape == base.shape and z_cl.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(z_cl, base)
    from einops import rearrange
    st_tokens = rearrange(z_cl, "b c f p -> (b f) p c")                 # model_ST.py:152
    assert st_tokens.data_ptr() == z_cl.data_ptr(), "rearrange copied: the channels-last result is not a view"
    assert torch.equal(st_tokens, rearrange(base, "b c f p -> (b f) p c"))
    if not out_bf16:
        ref = so.stem_forward(x_view[:2].double().cpu(), gp.to(torch.float64), tp.to(torch.float64))
        gate, strict = MATH_GATES[math]
        parity_gate(z_cl[:2], ref, gate, "channels-last stem vs oracle", strict=strict)


def test_two_stage_path_accepts_channels_last_input(dev):
    """Outside the fused kernels the modules still take the permuted view (they copy, like the reference's .contiguous())."""
    gcn, tcn, gp, tp, gen = _random_stem(22, None, 811, dev)
    batch = torch.randn(2, 30, 22, 3, generator=gen).to(dev)
    with torch.no_grad():
        a = tcn(gcn(batch.permute(0, 3, 1, 2)))
        b = tcn(gcn(batch.permute(0, 3, 1, 2).contiguous()))
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------
# SURVEY §8(f) rank 2 — backward of the training-mode blocks, against autograd through the fp64 oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["bf16x3", "f32", "f32_valu"])
@pytest.mark.parametrize("cin,cout,K,stride,N,T,V,bias", [
    (128, 128, 9, 1, 3, 21, 22, True),     # the stem's block: matrix-core wgrad + forward kernel as dgrad
    (128, 128, 9, 1, 2, 10, 46, True),     # 46 joints: other frame padding / frames per unit in the wgrad
    (64, 128, 9, 2, 2, 21, 22, True),      # strided: plain fp32 kernels
    (32, 64, 5, 1, 2, 9, 22, False),       # no conv bias, K = 5, 64 output channels
    (64, 64, 9, 1, 3, 40, 22, True),       # TCN_GCN_unit(64, 64): 64 output channels on the 128-channel matrix-core tiles
    (64, 128, 1, 1, 2, 12, 25, True),      # 1x1 (the residual "down" convs of the deeper layers)
    (128, 128, 4, 1, 2, 11, 22, True),     # EVEN K: the forward drops a frame (Tout = T-1); dgrad must not be the
    (32, 64, 2, 1, 2, 7, 22, True),        #   flipped-weight forward there, wgrad not the Tout==T kernel
    # corners of the one-wave-per-SIMD wgrad (tcn_wgrad_v6.hip: 17 <= V <= 24, odd K, ring of frames, two-frame units):
    (128, 256, 9, 1, 3, 13, 17, True),     # V = 17 (7 padded columns a frame: dz is not masked there, the input is), odd T, 2 row groups
    (96, 128, 7, 1, 5, 8, 24, False),      # V = 24 (no padding), three 32-channel groups (one block per wave), K = 7, clips % splits != 0
    (64, 128, 3, 1, 2, 5, 20, True),       # K = 3, clip shorter than the ring's window
    (128, 64, 1, 1, 2, 6, 19, True),       # K = 1, 64 output channels (half the dz tile reads as zeros)
    (64, 128, 9, 1, 1, 1, 22, True),       # one clip of ONE frame: lead-in units only + a half-empty unit
    # stride 2 with an odd K runs as the stride-1 backward on dz upsampled with zero frames (capi.hip: tcn_bwd_upsampled):
    (64, 128, 3, 2, 2, 20, 22, True),      # even T (the last input frame gets no gradient term from a dz frame), K = 3
    (128, 256, 9, 2, 2, 31, 25, False),    # odd T, 25 joints (the eight-wave wgrad kernel), no conv bias
    (32, 64, 9, 2, 1, 2, 22, True)])       # two input frames -> one output frame
def test_unit2d_backward_vs_oracle(cin, cout, K, stride, N, T, V, bias, math, dev):
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    torch.manual_seed(900 + cin + K + V)
    gen = torch.Generator().manual_seed(901 + cin + K + V)
    m = Unit2D(cin, cout, kernel_size=K, stride=stride, bias=bias)
    with torch.no_grad():
        m.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        if bias:
            m.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
    set_math_mode(m, math)
    tp = so.tcn_params_from_state(m.state_dict(), stride=stride).to(torch.float64)
    x = torch.randn(N, cin, T, V, generator=gen)
    # oracle: autograd through the fp64 restatement
    leaves = [tp.conv_w, tp.bn.weight, tp.bn.bias] + ([tp.conv_b] if bias else [])
    for t in leaves:
        t.requires_grad_(True)
    xr = x.double().requires_grad_(True)
    yr = so.tcn_forward(xr, tp, training=True)
    G = _kink_free_cotangent(yr, gen)
    grads = torch.autograd.grad((yr * G.double()).sum(), leaves + [xr])
    # HIP path
    m = m.to(dev).train()
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    parity_gate(y.detach(), yr.detach(), 1e-4, "training-mode forward")
    (y * G.to(dev)).sum().backward()
    gate = 1e-4
    _grad_gate(m.conv.weight.grad.reshape(cout, cin, K), grads[0], gate, "dW")
    _grad_gate(m.bn.weight.grad, grads[1], gate, "dgamma")
    _grad_gate(m.bn.bias.grad, grads[2], gate, "dbeta")
    _grad_gate(xd.grad, grads[-1], gate, "dx")
    if bias:   # analytically zero behind a batch-statistics BatchNorm: both sides are rounding noise
        assert m.conv.bias.grad.abs().max().item() <= 1e-3 * grads[2].abs().max().item()
        assert grads[3].abs().max().item() <= 1e-6 * grads[2].abs().max().item()


@pytest.mark.parametrize("N,T,V,cout", [(3, 20, 22, 128), (2, 50, 22, 128), (2, 12, 46, 128), (2, 9, 25, 64), (1, 7, 22, 256)])
def test_unit_agcn_backward_vs_oracle(N, T, V, cout, dev):
    """Every parameter gradient of the training-mode graph conv against autograd through the fp64 oracle."""
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = _random_stem(V, None, 1000 + T + V + cout, dev, c=cout)
    gp = gp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    x = torch.randn(N, 3, T, V, generator=gen)
    yr = so.agcn_forward(x.double(), gp, training=True)
    G = _kink_free_cotangent(yr, gen)
    names = sorted(leaves)
    ref = dict(zip(names, torch.autograd.grad((yr * G.double()).sum(), [leaves[k] for k in names])))
    gcn.train()
    y = gcn(x.to(dev))
    parity_gate(y.detach(), yr.detach(), 1e-4, "training-mode forward")
    (y * G.to(dev)).sum().backward()
    _compare_grads(_agcn_module_grads(gcn), ref, 1e-4)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("cin,cout,K,stride,N,T,V", [(128, 128, 9, 1, 3, 21, 22), (64, 128, 9, 2, 2, 21, 22), (32, 64, 3, 1, 2, 9, 25)])
def test_eval_mode_backward_unit2d_vs_oracle(cin, cout, K, stride, N, T, V, math, dev):
    """the reference's nn.BatchNorm2d stays differentiable in .eval() (model/net.py:52) — frozen-BatchNorm
    fine-tuning, saliency.  Running statistics are constants of the backward (STGCN_BN_FROZEN): every gradient against
    autograd through the fp64 oracle in eval mode; the buffers must not move."""
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    torch.manual_seed(1900 + cin + K + V)
    gen = torch.Generator().manual_seed(1901 + cin + K + V)
    m = Unit2D(cin, cout, kernel_size=K, stride=stride)
    with torch.no_grad():
        m.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        m.bn.running_mean.copy_(torch.randn(cout, generator=gen) * 0.3)
        m.bn.running_var.copy_(torch.rand(cout, generator=gen) * 1.5 + 0.25)
        m.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
    set_math_mode(m, math)
    tp = so.tcn_params_from_state(m.state_dict(), stride=stride).to(torch.float64)
    x = torch.randn(N, cin, T, V, generator=gen)
    leaves = [tp.conv_w, tp.bn.weight, tp.bn.bias, tp.conv_b]
    for t in leaves:
        t.requires_grad_(True)
    xr = x.double().requires_grad_(True)
    yr = so.tcn_forward(xr, tp, training=False)
    G = _kink_free_cotangent(yr, gen)
    grads = torch.autograd.grad((yr * G.double()).sum(), leaves + [xr])
    m = m.to(dev).eval()
    rm, rv, nb = m.bn.running_mean.clone(), m.bn.running_var.clone(), m.bn.num_batches_tracked.clone()
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    parity_gate(y.detach(), yr.detach(), 1e-4, "eval-mode forward under autograd")
    (y * G.to(dev)).sum().backward()
    assert torch.equal(m.bn.running_mean, rm) and torch.equal(m.bn.running_var, rv) and torch.equal(m.bn.num_batches_tracked, nb)
    _grad_gate(m.conv.weight.grad.reshape(cout, cin, K), grads[0], 1e-4, "dW")
    _grad_gate(m.bn.weight.grad, grads[1], 1e-4, "dgamma")
    _grad_gate(m.bn.bias.grad, grads[2], 1e-4, "dbeta")
    _grad_gate(m.conv.bias.grad, grads[3], 1e-4, "dbias")       # NOT zero behind a frozen BatchNorm
    _grad_gate(xd.grad, grads[-1], 1e-4, "dx")


@pytest.mark.parametrize("cin,cout,N,T,V,want_dx", [(3, 128, 3, 20, 22, False), (64, 64, 2, 12, 22, True), (64, 128, 2, 9, 25, True)])
def test_eval_mode_backward_unit_agcn_vs_oracle(cin, cout, N, T, V, want_dx, dev):
    """Same for unit_agcn (model/unit_agcn.py:54,91 in .eval()): stem class (the moment form is the batch-statistics closed
    form, so frozen statistics take the GEMM chain), identity residual and down branch, with dx."""
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = _random_stem(V, None, 2100 + cin + cout + T + V, dev, cin=cin, c=cout)
    gp = gp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    x = torch.randn(N, cin, T, V, generator=gen)
    xr = x.double().requires_grad_(want_dx)
    yr = so.agcn_forward(xr, gp, training=False)
    G = _kink_free_cotangent(yr, gen)
    names = sorted(leaves)
    got = torch.autograd.grad((yr * G.double()).sum(), [leaves[k] for k in names] + ([xr] if want_dx else []))
    ref = dict(zip(names, got))
    gcn.eval()
    bufs = [b.clone() for b in gcn.buffers()]
    xd = x.to(dev).requires_grad_(want_dx)
    y = gcn(xd)
    parity_gate(y.detach(), yr.detach(), 1e-4, "eval-mode forward under autograd")
    (y * G.to(dev)).sum().backward()
    assert all(torch.equal(a, b) for a, b in zip(bufs, gcn.buffers())), "eval-mode backward moved a buffer"
    grads = _agcn_module_grads(gcn)
    bad = []
    for k in names:       # (behind frozen statistics the conv_d / down biases have real gradients: plain per-tensor gate)
        g, r = grads[k].reshape(ref[k].shape).double().cpu(), ref[k].double().cpu()
        scale = r.abs().max().item()
        if k.startswith("a_b"):                    # conv_a's bias: constant shift under the column soft-max, zero gradient
            scale = max(scale, ref["a_w" + k[3:]].abs().max().item())
        err = (g - r).abs().max().item()
        if err > 1e-4 * max(scale, 1e-30):
            bad.append(f"d{k}: err {err:.3e} vs 1e-4*{scale:.3e}")
    assert not bad, "; ".join(bad)
    if want_dx:
        _grad_gate(xd.grad, got[-1], 1e-4, "dx")


def test_training_step_is_hip_graph_capturable(dev):
    """north_star / MI355X design: launch-bound loops belong in HIP graphs.  One training step of the stem — forward and
    backward, every kernel through the C ABI on the capturing stream, workspaces from torch's graph-private pool, no host
    synchronisation (the constant adjacency is uploaded once, not per step) — is captured once and replayed; the
    replayed gradients are bit-identical to the eager ones."""
    gcn, tcn, _, _, gen = _random_stem(22, None, 4242, dev)
    gcn.train(); tcn.train()
    params = list(gcn.parameters()) + list(tcn.parameters())
    bufs = [b for m in (gcn, tcn) for b in m.buffers()]
    x = torch.randn(6, 3, 24, 22, generator=gen).to(dev)
    G = torch.randn(6, 128, 24, 22, generator=gen).to(dev)

    def step():
        tcn(gcn(x)).backward(G)

    def restore(state):
        for b, s0 in zip(bufs, state):
            b.copy_(s0)

    step()                                            # first call: staging caches, adjacency upload
    state = [b.clone() for b in bufs]
    for p in params:
        p.grad = None
    step()
    ref = [p.grad.clone() for p in params]
    restore(state)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # torch's capture protocol: warm up on a side stream
        for p in params:
            p.grad = None
        step()
    torch.cuda.current_stream().wait_stream(side)
    restore(state)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    static = [p.grad for p in params]
    for _ in range(2):                                # replays are independent of each other
        restore(state)
        for g in static:
            g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, r in zip(static, ref):
            assert torch.equal(g, r)


def test_eval_mode_backward_through_the_stem(dev):
    """tcn0(gcn0(x)) in .eval() with gradients enabled and stem fusion on: the fused inference kernel has no backward, so
    the call takes the differentiable path; the result equals the fused kernel's within the fp32 contract."""
    from stgcn_amd import enable_stem_fusion
    gcn, tcn, gp, tp, gen = _random_stem(22, None, 77, dev)
    enable_stem_fusion(gcn, tcn)
    x = torch.randn(4, 3, 30, 22, generator=gen).to(dev)
    with torch.no_grad():
        ref = tcn(gcn(x))
    out = tcn(gcn(x))
    assert out.grad_fn is not None
    parity_gate(out.detach(), ref, 1e-4, "eval-mode stem under autograd vs fused inference kernel")
    out.square().mean().backward()
    for name, p in list(gcn.named_parameters()) + list(tcn.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


@pytest.mark.parametrize("cin,cout,N,T,V,layout", [
    (64, 64, 2, 180, 22, "nctv"),     # TCN_GCN_unit(64, 64) at the reference's frame count: 17 frame chunks
    (64, 128, 3, 37, 22, "nctv"),     # ragged last chunk
    (128, 128, 2, 90, 25, "nctv"),    # after the first stride-2 unit, odd joint count
    (256, 256, 1, 45, 22, "nctv"),    # last stage: inter_c = 64, two-frame chunks
    (64, 64, 2, 9, 46, "nctv"),       # two-hand graph: 3 x 3 blocks of the Gram
    (32, 64, 2, 5, 7, "nctv"),        # one block, mostly padding
    (64, 64, 1, 1, 22, "nctv"),       # a single frame
    (64, 64, 2, 30, 64, "nctv"),      # widest graph the attention kernels take
    (64, 64, 2, 23, 22, "ntvc"),      # channels-last input view
    (32, 64, 130, 6, 22, "nctv"),     # more than 128 clips: one workgroup per clip (up to 128: one per clip and subset)
    (64, 64, 130, 31, 22, "ntvc"),    # the same from the channels-last view: the contiguous copy is written by the staging path
    (256, 256, 2, 23, 22, "nctv"),    # 256 channels, two-frame chunks: in-place staging, eight rows per trip
    (48, 64, 2, 11, 22, "nctv"),      # C_in % 16 == 0 but not a power of two
    (24, 32, 2, 11, 22, "nctv")])     # C_in % 16 != 0: dword weight fragments, unpermuted rows
def test_generic_attention_on_matrix_cores_vs_oracle(cin, cout, N, T, V, layout, dev):
    """the adaptive adjacency of the deeper unit_agcn layers (model/unit_agcn.py:73-85 with C_in = 64..256:
    embeddings, Gram over (inter_c, T), column soft-max) runs on the fp32 matrix cores; P and the module output against the
    fp64 oracle at 1e-4."""
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = _random_stem(V, None, 3000 + cin + cout + T + V, dev, cin=cin, c=cout)
    x = torch.randn(N, cin, T, V, generator=gen)
    aux = {}
    yr = so.agcn_forward(x.double(), gp.to(torch.float64), aux=aux)
    P_ref = aux["P"]
    xg = x.to(dev)
    if layout == "ntvc":
        xg = xg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    with torch.no_grad():
        y = gcn(xg)
    parity_gate(gcn.last_attention, P_ref, 1e-4, "P")
    parity_gate(y, yr, 1e-4, "y")


@pytest.mark.parametrize("cin,cout,N,T,V,want_dx", [
    (64, 64, 2, 12, 22, True),      # TCN_GCN_unit(64, 64): identity residual (unit_agcn.py:57-58), input gradient
    (64, 128, 2, 10, 22, True),     # TCN_GCN_unit(64, 128): conv + BatchNorm residual, input gradient
    (128, 256, 1, 9, 25, True),     # wider, odd joint count
    (16, 32, 3, 7, 46, True),       # two-hand graph width, small channels (tiles mostly padding)
    (3, 128, 2, 20, 22, True),      # the stem's own shape WITH an input gradient: the generic chain, not the fused kernel
    (64, 128, 2, 10, 22, False),    # generic shape, x is data
    (64, 64, 4, 90, 22, True)])     # long clips: the weight-gradient slices and joint Grams split along K (15 parts, the last EMPTY)
def test_unit_agcn_generic_backward_vs_oracle(cin, cout, N, T, V, want_dx, dev):
    """unit_agcn backward for generic C_in / C_out, identity or conv residual, INCLUDING dx — what makes
    a TCN_GCN_unit (model/ST_TR/ST_TR_new.py:355-372) trainable.  Every gradient against autograd through the fp64
    oracle at 1e-4 of its tensor's max."""
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = _random_stem(V, None, 2000 + cin + cout + T + V, dev, cin=cin, c=cout)
    gp = gp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    x = torch.randn(N, cin, T, V, generator=gen)
    xr = x.double().requires_grad_(True)
    yr = so.agcn_forward(xr, gp, training=True)
    G = _kink_free_cotangent(yr, gen)
    names = sorted(leaves)
    grads = torch.autograd.grad((yr * G.double()).sum(), [leaves[k] for k in names] + [xr])
    ref = dict(zip(names, grads[:-1]))
    gcn.train()
    xg = x.to(dev).requires_grad_(want_dx)
    y = gcn(xg)
    parity_gate(y.detach(), yr.detach(), 1e-4, "training-mode forward")
    (y * G.to(dev)).sum().backward()
    _compare_grads(_agcn_module_grads(gcn), ref, 1e-4)
    if want_dx:
        _grad_gate(xg.grad, grads[-1], 1e-4, "dx")
    else:
        assert xg.grad is None
    # fixed-order reductions (per-clip slices, K parts): a second run gives the same bits.  (At these sizes each channel's
    # BatchNorm statistics come from ONE workgroup; above 8 K elements per channel (64 K for tensors of a thousand workgroups
    # and more: bn_chunks, csrc/common.h) several add their fp64 partial sums
    # atomically, in no fixed order — the one reduction of the path that is not bit-reproducible.)
    first = {k: v.clone() for k, v in _agcn_module_grads(gcn).items()}
    for p in gcn.parameters():
        p.grad = None
    y2 = gcn(x.to(dev).requires_grad_(want_dx))
    (y2 * G.to(dev)).sum().backward()
    for k, v in _agcn_module_grads(gcn).items():
        assert torch.equal(v, first[k]), f"d{k}: the generic backward is not deterministic"


def test_tcn_gcn_unit_trains_end_to_end(dev):
    """A TCN_GCN_unit as the ST-TR family builds it (gcn1 = unit_agcn(in,out), tcn1 = Unit2D(out,out,9,stride), residual
    Unit2D(in,out,1,stride); forward relu-free sum as at ST_TR_new.py:355-372) assembled from the drop-in modules:
    loss.backward() reaches every parameter and the block's input, and matches the fp64 oracle."""
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    V, cin, cout, stride = 22, 64, 128, 2
    gcn, _, gp, _, gen = _random_stem(V, None, 3100, dev, cin=cin, c=cout)
    torch.manual_seed(3101)
    tcn, down = Unit2D(cout, cout, kernel_size=9, stride=stride), Unit2D(cin, cout, kernel_size=1, stride=stride)
    for m in (tcn, down):
        with torch.no_grad():
            m.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
            m.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        set_math_mode(m, "f32_valu")
    tp = so.tcn_params_from_state(tcn.state_dict(), stride=stride).to(torch.float64)
    dp = so.tcn_params_from_state(down.state_dict(), stride=stride).to(torch.float64)
    gp = gp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    tl = {"t_w": tp.conv_w, "t_b": tp.conv_b, "r_w": dp.conv_w, "r_b": dp.conv_b}
    for t in tl.values():
        t.requires_grad_(True)
    x = torch.randn(2, cin, 21, V, generator=gen)
    xr = x.double().requires_grad_(True)
    yr = so.tcn_forward(so.agcn_forward(xr, gp, training=True), tp, training=True) + so.tcn_forward(xr, dp, training=True)
    G = torch.randn(yr.shape, generator=gen)
    names = sorted(leaves)
    grads = torch.autograd.grad((yr * G.double()).sum(), [leaves[k] for k in names] + list(tl.values()) + [xr])
    gcn.train(); tcn.to(dev).train(); down.to(dev).train()
    xg = x.to(dev).requires_grad_(True)
    y = tcn(gcn(xg)) + down(xg)
    parity_gate(y.detach(), yr.detach(), 1e-4, "TCN_GCN_unit forward")
    (y * G.to(dev)).sum().backward()
    # inner ReLUs sit under the cotangent: a flipped mask bit moves a gradient by a finite amount (see the stem step test)
    _compare_grads(_agcn_module_grads(gcn), dict(zip(names, grads[:len(names)])), 2e-3)
    got = {"t_w": tcn.conv.weight.grad.squeeze(-1), "t_b": tcn.conv.bias.grad, "r_w": down.conv.weight.grad.squeeze(-1),
           "r_b": down.conv.bias.grad}
    for i, k in enumerate(tl):
        ref = grads[len(names) + i]
        scale = max(ref.abs().max().item(), grads[len(names) + (i & ~1)].abs().max().item())   # biases: zero under batch-stat BN
        assert (got[k].double().cpu() - ref).abs().max().item() <= 2e-3 * scale, k
    _grad_gate(xg.grad, grads[-1], 2e-3, "dx of the unit")


def test_two_chained_tcn_gcn_units_train(dev):
    """Two units as the ST-TR backbone chains them (ST_TR_new.py:10-16: (64,64,1) then (64,128,2)), every kernel in its default
    arithmetic (bf16x3 temporal convs on the one-wave kernels, fp32-MFMA graph convs and GEMM chain): the gradient reaches the
    FIRST unit's parameters and the chain's input through the second unit's dx, and matches autograd through the fp64 oracle."""
    from stgcn_amd import Unit2D
    from oracle import stgcn_oracle as so
    V = 22
    g1, _, gp1, _, gen = _random_stem(V, None, 4100, dev, cin=64, c=64)
    g2, _, gp2, _, _ = _random_stem(V, None, 4101, dev, cin=64, c=128)
    torch.manual_seed(4102)
    t1, t2, d2 = Unit2D(64, 64, kernel_size=9), Unit2D(128, 128, kernel_size=9, stride=2), Unit2D(64, 128, kernel_size=1, stride=2)
    for m, c in ((t1, 64), (t2, 128), (d2, 128)):
        with torch.no_grad():
            m.bn.weight.copy_(torch.rand(c, generator=gen) + 0.5)
            m.bn.bias.copy_(torch.randn(c, generator=gen) * 0.2)
    tp1 = so.tcn_params_from_state(t1.state_dict()).to(torch.float64)
    tp2 = so.tcn_params_from_state(t2.state_dict(), stride=2).to(torch.float64)
    dp2 = so.tcn_params_from_state(d2.state_dict(), stride=2).to(torch.float64)
    gp1, gp2 = gp1.to(torch.float64), gp2.to(torch.float64)
    l1 = _agcn_oracle_leaves(gp1)
    _agcn_oracle_leaves(gp2)
    tp1.conv_w.requires_grad_(True)
    x = torch.randn(2, 64, 14, V, generator=gen)
    xr = x.double().requires_grad_(True)
    h = so.tcn_forward(so.agcn_forward(xr, gp1, training=True), tp1, training=True) + xr           # unit 1: identity residual
    yr = so.tcn_forward(so.agcn_forward(h, gp2, training=True), tp2, training=True) + so.tcn_forward(h, dp2, training=True)
    G = torch.randn(yr.shape, generator=gen)
    names = sorted(l1)
    grads = torch.autograd.grad((yr * G.double()).sum(), [l1[k] for k in names] + [tp1.conv_w, xr])
    for m in (g1, g2):
        m.train()
    t1.to(dev).train(); t2.to(dev).train(); d2.to(dev).train()
    xg = x.to(dev).requires_grad_(True)
    hg = t1(g1(xg)) + xg
    y = t2(g2(hg)) + d2(hg)
    parity_gate(y.detach(), yr.detach(), 2e-4, "two chained units, forward", strict=False)
    (y * G.to(dev)).sum().backward()
    # (ReLUs of two units sit under the cotangent: a flipped mask bit moves a gradient by a finite amount)
    _compare_grads(_agcn_module_grads(g1), dict(zip(names, grads[:len(names)])), 5e-3)
    _grad_gate(t1.conv.weight.grad.squeeze(-1), grads[-2], 5e-3, "first unit's temporal weights")
    _grad_gate(xg.grad, grads[-1], 5e-3, "dx of the chain")


@pytest.mark.parametrize("math", ["bf16x3", "f32_valu"])
def test_stem_training_step_vs_oracle(math, dev):
    """loss.backward() through tcn0(gcn0(x)) in .train() (train_sttran.py:185-191): all 4,780 + 147,840 parameter
    gradients against autograd through the fp64 oracle, and the running statistics both BatchNorm layers keep."""
    from stgcn_amd import set_math_mode
    from stgcn_amd.graphs import SHREGraph
    from oracle import stgcn_oracle as so
    A = torch.from_numpy(SHREGraph("spatial").A.astype(np.float32))
    gcn, tcn, gp, tp, gen = _random_stem(22, A, 1200, dev)
    set_math_mode(tcn, math)
    gp, tp = gp.to(torch.float64), tp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    tleaves = {"t_w": tp.conv_w, "t_b": tp.conv_b, "t_bn_w": tp.bn.weight, "t_bn_b": tp.bn.bias}
    for t in tleaves.values():
        t.requires_grad_(True)
    leaves.update(tleaves)
    x = torch.randn(4, 3, 40, 22, generator=gen)
    aux = {}
    hr = so.agcn_forward(x.double(), gp, training=True)
    zr = so.tcn_forward(hr, tp, training=True, aux=aux)
    # cotangent free of both ReLU kinks: the output's and (through a mask on nothing — h feeds a conv) the inner one is
    # handled by keeping clips whose inner activations stay clear of zero at fp32 resolution
    G = _kink_free_cotangent(zr, gen)
    names = sorted(leaves)
    ref = dict(zip(names, torch.autograd.grad((zr * G.double()).sum(), [leaves[k] for k in names])))
    gcn.train(); tcn.train()
    z = tcn(gcn(x.to(dev)))
    parity_gate(z.detach(), zr.detach(), 1e-4, "training-mode stem forward")
    (z * G.to(dev)).sum().backward()
    got = _agcn_module_grads(gcn)
    got.update({"t_w": tcn.conv.weight.grad.flatten(1).reshape(128, 128, 9), "t_bn_w": tcn.bn.weight.grad,
                "t_bn_b": tcn.bn.bias.grad})
    # the inner ReLU (h = relu(...)) cannot be masked out of the loss: a flipped bit there moves gradients by a finite
    # amount, so the gate for this whole-stem test is 2e-3 of max|ref| (the per-module tests above hold 1e-4)
    ref.pop("t_b")
    _compare_grads(got, ref, 2e-3)
    parity_gate(tcn.bn.running_mean, aux["bn"]["running_mean"], 1e-4, "tcn running_mean")


def _check_grads_vs_golden(mods, g, rel, extra=None):
    """Module .grad tensors against the reference's own gradients (tests/golden/make_golden_bwd.py)."""
    got = dict(extra or {})
    for prefix, mod in mods.items():
        for k, p in mod.named_parameters():
            assert p.grad is not None, f"{prefix}{k}: no gradient"
            got[prefix + k] = p.grad
    bad = []
    for name, val in got.items():
        ref = torch.from_numpy(g["grad." + name]).double()
        val = val.double().cpu().reshape(ref.shape)
        scale = ref.abs().max().item()
        if name.endswith(".bias") and any(t in name for t in ("conv_a", "conv_d", "down.0", "tcn.conv")):
            scale = max(scale, float(np.abs(g["grad." + name.replace(".bias", ".weight")]).max()))   # structurally zero
        err = (val - ref).abs().max().item()
        if not (err <= rel * scale):
            bad.append(f"{name}: {err:.3e} > {rel:g}*{scale:.3e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("math", ["bf16x3", "f32_valu"])
def test_stem_backward_vs_reference_gradients(math, dev):
    """loss.backward() through the drop-in modules against the gradients the REFERENCE's modules produced for the same
    parameters, input and cotangent (fixture bwd_stem_shre_T20)."""
    from stgcn_amd import set_math_mode
    g = load_golden("bwd_stem_shre_T20")
    gcn = build_gcn(g, 3, 128, dev).train()
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev).train()
    set_math_mode(tcn, math)
    z = tcn(gcn(torch.from_numpy(g["x"]).to(dev)))
    parity_gate(z.detach(), g["z"], 1e-4, "train-mode stem forward")
    z.backward(torch.from_numpy(g["G"]).to(dev))
    _check_grads_vs_golden({"gcn.": gcn, "tcn.": tcn}, g, 1e-3)     # (inner ReLU kinks, see test_stem_training_step_vs_oracle)


@pytest.mark.parametrize("case,cin,cout", [("bwd_gcn_shre_64_64_identity", 64, 64), ("bwd_gcn_shre_64_128", 64, 128)])
def test_generic_unit_agcn_backward_vs_reference_gradients(case, cin, cout, dev):
    """unit_agcn(64,64) (identity residual) and unit_agcn(64,128) with x.requires_grad: parameter gradients AND dx against
    the gradients the REFERENCE's own module produced (tests/golden/make_golden_bwd.py::gcn_bwd_case)."""
    g = load_golden(case)
    gcn = build_gcn(g, cin, cout, dev).train()
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    y = gcn(x)
    parity_gate(y.detach(), g["y"], 1e-4, "train-mode forward")
    y.backward(torch.from_numpy(g["G"]).to(dev))
    _check_grads_vs_golden({"gcn.": gcn}, g, 1e-4, extra={"x": x.grad})


@pytest.mark.parametrize("math", ["bf16x3", "f32_valu"])
def test_strided_unit2d_backward_vs_reference_gradients(math, dev):
    from stgcn_amd import set_math_mode
    g = load_golden("bwd_tcn_64_128_k9_s2")
    tcn = build_tcn(g, 64, 128, 9, 2, True, dev).train()
    set_math_mode(tcn, math)
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    z = tcn(x)
    parity_gate(z.detach(), g["z"], 1e-4, "train-mode strided forward")
    z.backward(torch.from_numpy(g["G"]).to(dev))
    _check_grads_vs_golden({"tcn.": tcn}, g, 1e-4, extra={"x": x.grad})


@pytest.mark.parametrize("cin,cout,N,T,V,out_bf16", [
    (128, 128, 40, 180, 22, False),    # 1240 tiles on 256 workgroups: every workgroup runs several tiles (input prefetch
    (64, 128, 3, 5, 22, False),        #   across the tile boundary);  C_in != C_out, a single short tile
    (128, 256, 6, 70, 25, True),       # odd T*V (unaligned rows), two 128-channel groups, bf16 output
    (16, 128, 30, 200, 7, False),      # one channel chunk, narrow frames: many tiles per clip
    (128, 128, 2, 1, 22, False),       # T = 1
    (64, 64, 20, 180, 22, False),      # TCN_GCN_unit(64, 64): 64 output channels on the 128-channel tile (padded packing)
    (64, 64, 5, 33, 25, True),         # ... bf16 output, odd T*V
    (32, 128, 9, 61, 25, False),       # K3v6 with a single period per tile (two channel chunks), many tiles, odd T*V
    (256, 256, 3, 45, 22, False)])     # eight periods per tile, two output groups
def test_large_tile_temporal_conv_kernel(cin, cout, N, T, V, out_bf16, dev):
    """K3v4 (stand-alone temporal conv, K = 9, stride 1, bf16x3) against the fp32 VALU kernel on the whole batch and
    against the fp64 oracle on sampled clips; also in raw (pre-activation) mode, which the training forward uses."""
    from stgcn_amd import Unit2D, functional as F, set_math_mode
    from oracle import stgcn_oracle as so
    gen = torch.Generator().manual_seed(cin + cout + T + V)
    torch.manual_seed(7)
    m = Unit2D(cin, cout, kernel_size=9)
    with torch.no_grad():
        m.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
        m.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        m.bn.running_mean.copy_(torch.randn(cout, generator=gen) * 0.3)
        m.bn.running_var.copy_(torch.rand(cout, generator=gen) + 0.25)
    tp = so.tcn_params_from_state(m.state_dict()).to(torch.float64)
    x = torch.randn(N, cin, T, V, generator=gen)
    m = m.to(dev).eval()
    assert F.tcn_supported(cin, cout, T, V, 9, 1, F.MATH_BF16X3)
    xd = x.to(dev)
    with torch.no_grad():
        set_math_mode(m, "f32_valu")
        base = m(xd)
        set_math_mode(m, "bf16x3")
        m.out_bf16 = out_bf16
        y = m(xd)
    gate = 4e-3 if out_bf16 else 1e-4          # bf16 output: half an ulp of the stored value
    parity_gate(y.float(), base, gate, "bf16x3 large-tile kernel vs fp32 VALU kernel", strict=not out_bf16)
    sel = sorted({0, N // 2, N - 1})
    ref = so.tcn_forward(x[sel].double(), tp)
    parity_gate(y[sel].float(), ref, gate, "sampled clips vs oracle", strict=not out_bf16)


def test_unit2d_training_step_many_tiles(dev):
    """Training forward (raw conv through the persistent kernel, 320 tiles on 256 workgroups) and backward at a batch
    where workgroups run more than one tile / unit, against autograd through the fp64 oracle."""
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    torch.manual_seed(77)
    gen = torch.Generator().manual_seed(78)
    m = Unit2D(128, 128, kernel_size=9)
    with torch.no_grad():
        m.bn.weight.copy_(torch.rand(128, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.randn(128, generator=gen) * 0.2)
    set_math_mode(m, "bf16x3")
    tp = so.tcn_params_from_state(m.state_dict()).to(torch.float64)
    x = torch.randn(20, 128, 180, 22, generator=gen)
    leaves = [tp.conv_w, tp.bn.weight, tp.bn.bias]
    for t in leaves:
        t.requires_grad_(True)
    xr = x.double().requires_grad_(True)
    yr = so.tcn_forward(xr, tp, training=True)
    G = _kink_free_cotangent(yr, gen)
    grads = torch.autograd.grad((yr * G.double()).sum(), leaves + [xr])
    m = m.to(dev).train()
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    parity_gate(y.detach(), yr.detach(), 1e-4, "training-mode forward, many tiles")
    y.backward(G.to(dev))
    _grad_gate(m.conv.weight.grad.reshape(128, 128, 9), grads[0], 1e-4, "dW")
    _grad_gate(m.bn.weight.grad, grads[1], 1e-4, "dgamma")
    _grad_gate(m.bn.bias.grad, grads[2], 1e-4, "dbeta")
    _grad_gate(xd.grad, grads[3], 1e-4, "dx")


@pytest.mark.parametrize("N,T,V", [(2, 1, 22), (1, 3, 46), (3, 9, 7)])
def test_training_step_degenerate_shapes(N, T, V, dev):
    """T = 1, single clip, narrow frames: forward + backward of both modules still agree with the fp64 oracle."""
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 1300 + T + V, dev)
    gp, tp = gp.to(torch.float64), tp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    x = torch.randn(N, 3, T, V, generator=gen)
    hr = so.agcn_forward(x.double(), gp, training=True)
    G = _kink_free_cotangent(hr, gen)
    names = sorted(leaves)
    ref = dict(zip(names, torch.autograd.grad((hr * G.double()).sum(), [leaves[k] for k in names])))
    gcn.train()
    h = gcn(x.to(dev))
    parity_gate(h.detach(), hr.detach(), 1e-4, "graph conv, training forward")
    h.backward(G.to(dev))
    _compare_grads(_agcn_module_grads(gcn), ref, 1e-4)
    # temporal block on the same degenerate shape
    tl = [tp.conv_w, tp.bn.weight, tp.bn.bias]
    for t in tl:
        t.requires_grad_(True)
    xin = torch.randn(N, 128, T, V, generator=gen)
    xr = xin.double().requires_grad_(True)
    zr = so.tcn_forward(xr, tp, training=True)
    G2 = _kink_free_cotangent(zr, gen)
    g2 = torch.autograd.grad((zr * G2.double()).sum(), tl + [xr])
    tcn.train()
    xd = xin.to(dev).requires_grad_(True)
    z = tcn(xd)
    parity_gate(z.detach(), zr.detach(), 1e-4, "temporal block, training forward")
    z.backward(G2.to(dev))
    _grad_gate(tcn.conv.weight.grad.reshape(128, 128, 9), g2[0], 1e-4, "dW")
    _grad_gate(tcn.bn.weight.grad, g2[1], 1e-4, "dgamma")
    _grad_gate(xd.grad, g2[3], 1e-4, "dx")


def test_unit2d_backward_bf16_mode(dev):
    """STGCN_MATH_BF16 (operands rounded to bf16, the documented 1e-2 mode) also drives the backward kernels."""
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    torch.manual_seed(31)
    gen = torch.Generator().manual_seed(32)
    m = Unit2D(128, 128, kernel_size=9)
    set_math_mode(m, "bf16")
    tp = so.tcn_params_from_state(m.state_dict()).to(torch.float64)
    x = torch.randn(3, 128, 30, 22, generator=gen)
    leaves = [tp.conv_w, tp.bn.weight, tp.bn.bias]
    for t in leaves:
        t.requires_grad_(True)
    xr = x.double().requires_grad_(True)
    yr = so.tcn_forward(xr, tp, training=True)
    G = torch.randn(yr.shape, generator=gen) * (yr.detach() > 2e-2 * yr.detach().abs().max()).float()
    grads = torch.autograd.grad((yr * G.double()).sum(), leaves + [xr])
    m = m.to(dev).train()
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    parity_gate(y.detach(), yr.detach(), 1e-2, "bf16 training forward", strict=False)
    y.backward(G.to(dev))
    _grad_gate(m.conv.weight.grad.reshape(128, 128, 9), grads[0], 2e-2, "dW")
    _grad_gate(xd.grad, grads[3], 2e-2, "dx")


def test_unit_agcn_backward_more_clips_than_workgroups(dev):
    """N = 300 clips on the 256-workgroup grid of the graph-conv backward: 44 workgroups process two clips, so the
    per-workgroup accumulators (weight gradients, dPA, dM) carry over from one clip to the next."""
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = _random_stem(22, None, 1400, dev)
    gp = gp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    x = torch.randn(300, 3, 6, 22, generator=gen)
    yr = so.agcn_forward(x.double(), gp, training=True)
    G = _kink_free_cotangent(yr, gen)
    names = sorted(leaves)
    ref = dict(zip(names, torch.autograd.grad((yr * G.double()).sum(), [leaves[k] for k in names])))
    gcn.train()
    y = gcn(x.to(dev))
    parity_gate(y.detach(), yr.detach(), 1e-4, "training-mode forward, 300 clips")
    y.backward(G.to(dev))
    _compare_grads(_agcn_module_grads(gcn), ref, 1e-4)


@pytest.mark.parametrize("V,T,N", [(22, 40, 3), (46, 20, 2)])
def test_fused_stem_256_channels(V, T, N, dev):
    """C = 256 (two 128-channel output groups, 16 input-channel chunks): fused bf16x3 stem against the fp64 oracle."""
    from stgcn_amd import enable_stem_fusion
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 1500 + V, dev, c=256)
    x = torch.randn(N, 3, T, V, generator=gen)
    ref = so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64))
    with torch.no_grad():
        two = tcn(gcn(x.to(dev)))
        enable_stem_fusion(gcn, tcn)
        fused = tcn(gcn(x.to(dev)))
    parity_gate(two, ref, 1e-4, "two-stage, 256 channels")
    parity_gate(fused, ref, 1e-4, "fused, 256 channels")


@pytest.mark.parametrize("N,T,V,cout", [
    (64, 180, 22, 128),     # the stem's own size class: 18 frame chunks of 10 frames, 16-byte loads
    (8, 200, 46, 128),      # two-hand graph: 4-frame chunks, 3 x 3 blocks in the attention part
    (6, 500, 22, 64),       # BASELINE configs[2] frame count, 64 output channels
    (5, 63, 25, 128),       # odd T*V: the scalar-load path of the gather kernel
    (3, 37, 22, 256)])      # 256 output channels (8 channel blocks per chunk)
def test_stem_backward_moment_form_matches_gemm_chain_at_size(N, T, V, cout, dev):
    """The two HIP implementations of the stem-class graph-conv backward against each other at sizes the fp64 oracle does
    not reach in seconds: the moment form (one pass over dy / y, everything else from the forward's feature moments) and
    the generic chain of batched fp32 GEMMs (which rebuilds both branches and takes the BatchNorm statistics from them).
    Each is pinned to the oracle at small sizes; here they must agree on every gradient to 2e-4 of its tensor's max."""
    from stgcn_amd import functional as F
    gcn, _, _, _, gen = _random_stem(V, None, 5000 + T + V + cout, dev, c=cout)
    gcn.train()
    x = torch.randn(N, 3, T, V, generator=gen).to(dev)
    st = gcn._staged(dev)
    bn, d = gcn.bn, gcn.down[1]
    y, P, zm, zd, stats = F.agcn_forward_train(
        x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"], st["bdown"],
        (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var),
        (d.weight.detach(), d.bias.detach(), d.running_mean, d.running_var), 0.1, 1e-5, save=True)
    assert zm is None and zd is None                       # the moments path: no branch was kept
    # cotangent zero next to the ReLU kink (cf. _kink_free_cotangent): the moment form takes the mask from the forward's own
    # y, the chain from branches it rebuilds — an element whose pre-activation is within rounding of zero may differ, and a
    # flipped mask bit moves a gradient by a finite amount
    dy = torch.randn(y.shape, generator=gen).to(dev) * (y > 2e-2 * y.abs().max()).float()
    args = (x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"], st["bdown"], P, None, None,
            bn.weight.detach(), bn.bias.detach(), d.weight.detach(), d.bias.detach(), stats, dy)
    fused = F.agcn_backward_train(*args, y=y)              # moment form
    chain = F.agcn_backward_train(*args, y=None)           # GEMM chain (rebuilds zm / zd in its workspace)
    torch.cuda.synchronize()
    bad = []
    for k in sorted(chain):
        a, b = fused[k].double(), chain[k].double()
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), k
        scale = b.abs().max().item()
        if k in ("dbd", "dbdown", "dba"):                  # analytically zero (see _compare_grads): rounding noise both ways
            scale = max(scale, chain["dWd" if k == "dbd" else ("dWdown" if k == "dbdown" else "dWa")].abs().max().item())
        err = (a - b).abs().max().item()
        if err > 2e-4 * max(scale, 1e-30):
            bad.append(f"{k}: {err:.3e} vs 2e-4*{scale:.3e}")
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------
# round 3: host-side hardening
# ---------------------------------------------------------------------------------------
def test_step_stats_probes_the_channels_last_result_in_place(dev):
    """`bench.py --layout ntvc --gpus N>1` calls step_stats on the (N,C,T,V) VIEW of (N,T,V,C) memory that the
    fused stem returns under set_output_layout('channels_last'); it used to be refused (non-contiguous)."""
    from stgcn_amd import dist as sd, enable_stem_fusion, set_output_layout
    gcn, tcn, gp, tp, gen = _random_stem(22, None, 31, dev)
    enable_stem_fusion(gcn, tcn)
    x = torch.randn(5, 3, 40, 22, generator=gen).to(dev)
    with torch.no_grad():
        ref = tcn(gcn(x))
        set_output_layout(tcn, "channels_last")
        out = tcn(gcn(x))
    assert not out.is_contiguous() and out.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(out, ref)
    got, want = sd.step_stats(out, 5).cpu(), sd.step_stats(ref, 5).cpu()
    assert torch.equal(got, want)                                   # same 5 x 128 probes, same summation order
    probe = ref[:, :, 0, 0].double().cpu()
    assert torch.allclose(got.double(), torch.tensor([5.0, probe.sum().item(), probe.square().sum().item(), 0.0],
                                                     dtype=torch.float64), rtol=1e-5, atol=1e-3)
    sliced = ref[:, ::2]                                            # any positive clip / channel strides
    p2 = sliced[:, :, 0, 0].double().cpu()
    assert torch.allclose(sd.step_stats(sliced, 5).cpu()[1:3].double(),
                          torch.tensor([p2.sum().item(), p2.square().sum().item()], dtype=torch.float64), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("fused", [False, True])
def test_parameter_swap_by_data_assignment_restages(fused, dev):
    """``param.data = new`` (an EMA / weight swap) does not bump ``_version``; the staging cache is keyed
    on the storage address as well, so the next forward uses the new values (checked against the oracle)."""
    from stgcn_amd import enable_stem_fusion
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _random_stem(22, None, 77, dev)
    if fused:
        enable_stem_fusion(gcn, tcn)
    x = torch.randn(2, 3, 24, 22, generator=gen)
    with torch.no_grad():
        z0 = tcn(gcn(x.to(dev))).cpu()
        parity_gate(z0, so.stem_forward(x, gp, tp), 1e-4, "before the swap")
        v = (tcn.conv.weight._version, gcn.PA._version, gcn.bn.running_var._version)
        tcn.conv.weight.data = (torch.randn(tcn.conv.weight.shape, generator=gen) * 0.05).to(dev)
        gcn.PA.data = (torch.randn(3, 22, 22, generator=gen) * 0.1).to(dev)
        gcn.conv_d[1].weight.data = (torch.randn(gcn.conv_d[1].weight.shape, generator=gen) * 0.3).to(dev)
        gcn.bn.running_var.data = (torch.rand(128, generator=gen) + 0.5).to(dev)     # a buffer, swapped the same way
        assert v == (tcn.conv.weight._version, gcn.PA._version, gcn.bn.running_var._version)   # the premise of the test
        z1 = tcn(gcn(x.to(dev))).cpu()
    gcn_cpu = {k: t.detach().cpu() for k, t in gcn.state_dict().items()}
    tcn_cpu = {k: t.detach().cpu() for k, t in tcn.state_dict().items()}
    ref = so.stem_forward(x, so.agcn_params_from_state(gcn_cpu, gcn.A), so.tcn_params_from_state(tcn_cpu))
    parity_gate(z1, ref, 1e-4, "after the swap")
    assert (z1 - z0).abs().max() > 1e-2 * ref.abs().max()           # the swap is visible at all


def test_moment_form_backward_refuses_statistics_without_moments(dev):
    """stgcn_agcn_backward_train picks the moment form from (zm == NULL, y != NULL, no dx) and then reads the 63
    feature moments behind save_stats — which only a moments-path forward writes.  A forward that saved the branches now
    clears that block (validity mark), and the moment form answers NaN everywhere instead of a plausible wrong gradient;
    the properly paired calls are unaffected."""
    from stgcn_amd import functional as F
    gcn, tcn, gp, tp, gen = _random_stem(22, None, 13, dev)
    gcn.train()
    st = gcn._staged(dev)
    x = torch.randn(3, 3, 20, 22, generator=gen).to(dev)
    dy = torch.randn(3, 128, 20, 22, generator=gen).to(dev)
    bn, d = gcn.bn, gcn.down[1]
    def fwd(save):
        return F.agcn_forward_train(x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"],
                                    st["bdown"], (bn.weight.detach(), bn.bias.detach(), bn.running_mean.clone(), bn.running_var.clone()),
                                    (d.weight.detach(), d.bias.detach(), d.running_mean.clone(), d.running_var.clone()),
                                    bn.momentum, bn.eps, save=save)
    def bwd(P, zm, zd, stats, y):
        return F.agcn_backward_train(x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"],
                                     st["bdown"], P, zm, zd, bn.weight.detach(), bn.bias.detach(), d.weight.detach(),
                                     d.bias.detach(), stats, dy, need_dx=False, y=y)
    y1, P1, zm1, zd1, stats1 = fwd(True)               # moments path
    y2, P2, zm2, zd2, stats2 = fwd("branches")         # materialising path: branches saved, no moments
    assert zm1 is None and zm2 is not None
    parity_gate(y2, y1, 1e-5, "both forwards agree")
    good = bwd(P1, None, None, stats1, y1)             # moment form, properly paired
    chain = bwd(P2, zm2, zd2, stats2, y2)              # GEMM chain on the saved branches
    for k in ("dWd", "dWdown", "dgamma", "dbeta", "ddgamma", "dPA", "dWa", "dWb"):
        parity_gate(good[k], chain[k], 2e-4, f"moment form vs GEMM chain: {k}", strict=False)
    bad = bwd(P2, None, None, stats2, y2)              # the mis-paired call of the advisor's report
    for k in ("dWd", "dbd", "dWdown", "dbdown", "dgamma", "dbeta", "ddgamma", "ddbeta", "dPA", "dWa", "dWb"):
        assert torch.isnan(bad[k]).all(), f"{k}: a mis-paired moment-form backward must not return numbers"


# ---------------------------------------------------------------------------------------
# round 3: KF6 over the two joint halves of a wide frame (stem_bf16_v6w.hip; VERDICT r2 #2: configs[3], V = 46)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["bf16x3", "bf16"])
@pytest.mark.parametrize("N,T,V", [(3, 40, 46),      # LMDHG: halves 24 | 22
                                   (2, 200, 46),     # configs[3]'s clip length: 19 + 18 tiles per clip, interleaved
                                   (5, 13, 34),      # halves 20 | 14 (one column block in the second half)
                                   (2, 30, 48),      # 24 | 24: the widest frame whose halves the producer covers (<= 26 joints each)
                                   (2, 25, 40),      # 20 | 20
                                   (260, 12, 46)])   # more tiles than workgroups: the persistent loop, both halves per workgroup
def test_wide_frame_stem_on_the_one_wave_kernel(N, T, V, math, dev):
    """Frames of 32 < V <= 64 joints run through KF6 as two joint halves (the temporal conv never mixes joints; the
    aggregation still sums over all V joints).  Against the fp64 oracle, fused == two-stage within the gate, and the kernel
    name the library reports is the one-wave kernel (so a silent fallback to the eight-wave tile would show)."""
    from stgcn_amd import _capi, enable_stem_fusion, functional as F, set_math_mode
    from oracle import stgcn_oracle as so
    fl = F._flags({"bf16x3": F.MATH_BF16X3, "bf16": F.MATH_BF16}[math], False)
    assert _capi.lib().stgcn_stem_kernel_name(3, 128, T, V, 9, 3, fl).decode() == "stem_bf16_v6_kernel"
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 900 + T + V, dev)
    set_math_mode(tcn, math)
    enable_stem_fusion(gcn, tcn)
    x = torch.randn(N, 3, T, V, generator=gen)
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
    pick = sorted({0, N // 2, N - 1})
    aux = {}
    ref = so.stem_forward(x[pick].double(), gp.to(torch.float64), tp.to(torch.float64), aux=aux)
    rel, strict = MATH_GATES[math]
    parity_gate(gcn.last_attention[pick], aux["gcn"]["P"], 1e-4, "P")
    parity_gate(z[pick], ref, rel, f"wide stem V={V} T={T} {math}", strict)
    if N > 8:                                  # clip independence across the persistent loop: a clip alone == the clip in the batch
        with torch.no_grad():
            alone = tcn(gcn(x[N - 3:N - 2].to(dev)))
        assert torch.equal(alone[0], z[N - 3])


@pytest.mark.parametrize("T,V", [(20, 35), (4, 46), (30, 64), (30, 50), (12, 62)])
def test_wide_frames_outside_the_split_fall_back(T, V, dev):
    """Odd V (rows would lose their 8-byte alignment), clips too short for the fragments to fit the idle image buffer, and
    halves the producer cannot cover (more than 26 joints) keep the eight-wave kernel or the two-stage path — and stay
    inside the gate."""
    from stgcn_amd import _capi, enable_stem_fusion, functional as F
    from oracle import stgcn_oracle as so
    fl = F._flags(F.MATH_BF16X3, False)
    assert _capi.lib().stgcn_stem_kernel_name(3, 128, T, V, 9, 3, fl).decode() != "stem_bf16_v6_kernel"
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 950 + T + V, dev)
    enable_stem_fusion(gcn, tcn)
    x = torch.randn(2, 3, T, V, generator=gen)
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
    parity_gate(z, so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64)), 1e-4, f"fallback V={V} T={T}")


# ---------------------------------------------------------------------------------------
# round 3: KF7 — fp16 x fp16 + two block-scaled e4m3 residual products (stem_f16mx.hip, math mode "f16mx")
# ---------------------------------------------------------------------------------------
def _f16mx_name(T, V, C=128):
    from stgcn_amd import _capi, functional as F
    return _capi.lib().stgcn_stem_kernel_name(3, C, T, V, 9, 3, F._flags(F.MATH_F16MX, False)).decode()


@pytest.mark.parametrize("case", ["stem_shre_T180", "stem_shre_T500"])
def test_f16mx_stem_vs_golden(case, dev):
    """The reference's own stem outputs (fixtures generated from the imported reference) at the fp32 gate, on KF7."""
    from stgcn_amd import enable_stem_fusion
    g = load_golden(case)
    gcn = build_gcn(g, 3, 128, dev)
    tcn = build_tcn(g, 128, 128, 9, 1, True, dev, "f16mx")
    enable_stem_fusion(gcn, tcn)
    x = torch.from_numpy(g["skeleton"]).to(dev).permute(0, 3, 1, 2).contiguous()
    assert _f16mx_name(x.shape[2], 22) == "stem_f16mx_kernel"
    with torch.no_grad():
        z = tcn(gcn(x)).cpu()
    scale = float(g["z_eval_absmax"])
    err = (gather_flat(z, g["z_eval_idx"]).double() - torch.from_numpy(g["z_eval_val"]).double()).abs().max().item()
    assert err <= 1e-4 * scale, f"{case} f16mx: {err:.3e} vs {scale:.3e}"
    assert float(z.double().sum()) == pytest.approx(float(g["z_eval_sum"]), rel=1e-4, abs=1e-3 * scale)


@pytest.mark.parametrize("N,T,V", [(3, 37, 22), (1, 5, 22), (2, 64, 24), (1, 1, 22), (2, 23, 7), (8, 180, 22), (300, 20, 22), (2, 90, 16)])
def test_f16mx_stem_vs_oracle(N, T, V, dev):
    """Ragged shapes, one-frame clips, narrow frames, more tiles than workgroups — against the fp64 oracle at the max-norm
    gate of north_star (1e-4 of max|ref|)."""
    from stgcn_amd import enable_stem_fusion, set_math_mode
    from oracle import stgcn_oracle as so
    assert _f16mx_name(T, V) == "stem_f16mx_kernel"
    gcn, tcn, gp, tp, gen = _random_stem(V, None, 1200 + T + V, dev)
    set_math_mode(tcn, "f16mx")
    enable_stem_fusion(gcn, tcn)
    x = torch.randn(N, 3, T, V, generator=gen)
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
    pick = sorted({0, N // 2, N - 1})
    ref = so.stem_forward(x[pick].double(), gp.to(torch.float64), tp.to(torch.float64))
    parity_gate(z[pick], ref, 1e-4, f"f16mx N={N} T={T} V={V}", strict=False)    # (typically 2e-5; up to ~6e-5 on very short clips)
    if N > 8:
        with torch.no_grad():
            alone = tcn(gcn(x[N - 3:N - 2].to(dev)))
        assert torch.equal(alone[0], z[N - 3])                        # clip independence across the persistent loop


@pytest.mark.parametrize("unit", [1e-3, 1.0, 250.0, 3e4])
def test_f16mx_scales_follow_the_input_magnitude(unit, dev):
    """The e4m3 operands are pre-scaled by a per-clip bound (max|x| from K1 x weight norms from stgcn_stem_prepare), so the
    result is as accurate for skeletons in millimetres (|x| ~ 1e3-1e4) or in kilometres as for unit-scale ones: no
    saturation path.  One batch mixes clips of very different magnitude (the bound is per clip)."""
    from stgcn_amd import enable_stem_fusion, set_math_mode
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _random_stem(22, None, 1300, dev)
    set_math_mode(tcn, "f16mx")
    enable_stem_fusion(gcn, tcn)
    x = torch.randn(4, 3, 60, 22, generator=gen) * unit
    x[1] *= 1e-2
    x[2] *= 30.0
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
    ref = so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64))
    for n in range(4):                                                # per clip: each clip against ITS OWN scale
        parity_gate(z[n], ref[n], 1e-4, f"f16mx clip {n} at unit {unit:g}", strict=False)


@pytest.mark.parametrize("out_bf16", [False, True])
def test_f16mx_layout_fusion_is_bit_exact(out_bf16, dev):
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    gcn, tcn, gp, tp, gen = _random_stem(22, None, 1400, dev)
    set_math_mode(tcn, "f16mx")
    tcn.out_bf16 = out_bf16
    enable_stem_fusion(gcn, tcn)
    batch = torch.randn(21, 50, 22, 3, generator=gen).to(dev)
    x_view = batch.permute(0, 3, 1, 2)
    with torch.no_grad():
        base = tcn(gcn(x_view.contiguous()))
        assert torch.equal(tcn(gcn(x_view)), base)
        set_output_layout(tcn, "channels_last")
        z_cl = tcn(gcn(x_view))
    assert z_cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(z_cl, base)


def test_f16mx_fallbacks(dev):
    """Shapes outside KF7 (256 channels: the eight-wave kernel; wide frames: KF6 over the joint halves) silently keep the
    three-bf16 kernels at the same gate; the two-stage path ignores the flag."""
    from stgcn_amd import enable_stem_fusion, set_math_mode
    from oracle import stgcn_oracle as so
    assert _f16mx_name(40, 22, 256) == "stem_bf16_v4_kernel"
    assert _f16mx_name(40, 46) == "stem_bf16_v6_kernel"
    for V, c in ((22, 256), (46, 128)):
        gcn, tcn, gp, tp, gen = _random_stem(V, None, 1500 + V, dev, c=c)
        set_math_mode(tcn, "f16mx")
        x = torch.randn(2, 3, 40, V, generator=gen)
        ref = so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64))
        with torch.no_grad():
            two = tcn(gcn(x.to(dev)))
            enable_stem_fusion(gcn, tcn)
            fused = tcn(gcn(x.to(dev)))
        parity_gate(two, ref, 1e-4, f"two-stage V={V} C={c}")      # (neither runs KF7: the strict criterion holds)
        parity_gate(fused, ref, 1e-4, f"fused V={V} C={c}")
