"""GPU tests of the low-latency path of the AltFormer heads: the smaller tile forms of the token-major linear (64 x 64 and
32 x 64 beside 128 x 128), the plan that picks one (``VIT_TILE_AUTO``), the block entry point with it, the module switch
``set_low_latency`` at one clip, and the capture of that forward in a graph.

A smaller form changes which workgroup computes an output element, never how: the comparisons with the 128 x 128 form are
``torch.equal``.  Bit-equality would not notice a mistake both forms share, so the 32-row form also meets the kernel's
existing contract against fp64 (tests/altformer_ref.py, ``parity_gate(rel=1e-4)``)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import altformer_ref as ar
from _util import gather_flat, load_golden, parity_gate, sub_state

pytestmark = pytest.mark.gpu
REL = 1e-4
ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def _forms():
    from stgcn_amd import _capi
    return {"64": _capi.VIT_TILE_64, "32": _capi.VIT_TILE_32, "auto": _capi.VIT_TILE_AUTO}


# ---- the linear -----------------------------------------------------------------------------------------------------------
def _linear_inputs(M, K, Nout, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * M + K + Nout + seed)
    x = torch.randn(M, K, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    W = (torch.rand(Nout, K, generator=g) * 2 - 1) / K ** 0.5
    b = torch.randn(Nout, generator=g) * 0.5
    R = torch.randn(M, Nout, generator=g)
    lw, lb = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    return x, W, b, R, lw, lb


EPILOGUES = ("plain", "bias+ln", "bias+ln+gelu", "bias+residual_in_place")


def _run_linear(F, ep, t, math):
    x, W, b, R, lw, lb = t
    if ep == "plain":
        return F.vit_linear(x, W, None, math=math)
    if ep == "bias+ln":
        return F.vit_linear(x, W, b, ln=(lw, lb, ar.EPS), math=math)
    if ep == "bias+ln+gelu":
        return F.vit_linear(x, W, b, ln=(lw, lb, ar.EPS), gelu=True, math=math)
    y = R.clone()                                            # y aliases the residual: each element read and written once
    out = F.vit_linear(x, W, b, residual=y, math=math, y=y)
    assert out.data_ptr() == y.data_ptr()
    return out


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("kn", [(256, 768), (512, 256), (256, 100)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("M", [1, 22, 33, 180, 705])
def test_linear_every_form_equals_the_128_form(M, kn, math, dev):
    """M = 33 and 705 leave a partial row tile in every form (33 = 32 + 1, 705 = 5 * 128 + 65 = 11 * 64 + 1 = 22 * 32 + 1);
    Nout = 100 is no multiple of 32: the column guard."""
    from stgcn_amd import functional as F
    K, Nout = kn
    mode = getattr(F, "MATH_" + math.upper())
    t = tuple(v.to(dev) for v in _linear_inputs(M, K, Nout, dev))
    assert F.vit_linear_tile(M, K, Nout, mode) == (128, 128)
    assert F.vit_linear_tile(M, K, Nout, mode | _forms()["64"]) == (64, 64)
    assert F.vit_linear_tile(M, K, Nout, mode | _forms()["32"]) == (32, 64)
    for ep in EPILOGUES:
        want = _run_linear(F, ep, t, mode)
        assert torch.isfinite(want).all()
        for name, fl in _forms().items():
            got = _run_linear(F, ep, t, mode | fl)
            assert torch.equal(got, want), f"M={M} K={K} Nout={Nout} {math} {ep}: form {name} differs from 128 x 128 " \
                                           f"(max |diff| {(got - want).abs().max().item():.3e})"


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("shape", [(705, 256, 768), (33, 256, 100)], ids=lambda s: "x".join(map(str, s)))
def test_linear_32_row_form_vs_fp64(shape, math, dev):
    from stgcn_amd import functional as F
    M, K, Nout = shape
    x, W, b, R, lw, lb = _linear_inputs(M, K, Nout, dev, seed=5)
    mode = getattr(F, "MATH_" + math.upper()) | _forms()["32"]
    xd, Wd, bd, Rd, lwd, lbd = (v.to(dev) for v in (x, W, b, R, lw, lb))
    xn = TF.layer_norm(x.double(), (K,), lw.double(), lb.double(), ar.EPS)
    want = {"plain": x.double() @ W.double().T,
            "bias+ln+gelu": TF.gelu(xn @ W.double().T + b.double()),
            "bias+residual": x.double() @ W.double().T + b.double() + R.double()}
    got = {"plain": F.vit_linear(xd, Wd, None, math=mode),
           "bias+ln+gelu": F.vit_linear(xd, Wd, bd, ln=(lwd, lbd, ar.EPS), gelu=True, math=mode),
           "bias+residual": F.vit_linear(xd, Wd, bd, residual=Rd, math=mode)}
    for k in want:
        rel = parity_gate(got[k], want[k], REL, f"linear {shape} {math} 32-row form {k}")
        print(f"linear {shape} {math} 32-row form {k}: {rel:.3e}")


# ---- one block ------------------------------------------------------------------------------------------------------------
# (B, L, D, heads, hidden).  The first four are one clip's and a few clips' stages.  Their largest linear, 230 x 1536, is 24
# tiles of 128 x 128, and the plan must go below 128 x 128 at 186 such tiles (tests/test_vit_tile_plan.py), so whatever the
# cut, they cannot select the 128 x 128 form; the fifth (32 clips of a temporal stage at D = 256: 270 tiles of 128 x 128 in
# the qkv linear, 90 in the proj linear) is there for the larger forms.
BLOCK_SHAPES = [(3, 22, 256, 8, 512), (1, 180, 512, 8, 1024), (5, 46, 512, 8, 1024), (1, 22, 512, 8, 1024), (32, 180, 256, 8, 512)]


def _block_args(shape, dev):
    B, L, D, heads, hidden = shape
    sd = {k: v.to(dev) for k, v in ar.random_block_state(D, hidden, True, seed=B + L + D).items()}
    g = torch.Generator().manual_seed(L + B)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    pair = lambda n: (sd[n + ".weight"], sd[n + ".bias"])
    return x.to(dev), (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))


@pytest.mark.parametrize("mode", ["f32", "mixed"])
@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_with_auto_tiles_equals_the_unflagged_call(shape, mode, dev):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    B, L, D, heads, hidden = shape
    x, params = _block_args(shape, dev)
    math = HEAD_MATH[mode]
    want = F.vit_block_forward(x, *params, heads, ar.EPS, (D // heads) ** -0.5, math)
    got = F.vit_block_forward(x, *params, heads, ar.EPS, (D // heads) ** -0.5, math | _forms()["auto"])
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), f"block {shape} {mode}: max |diff| {(got - want).abs().max().item():.3e}"


def test_block_cases_select_every_form():
    """No GPU work: the plan, asked for the four linears of every block case above."""
    from stgcn_amd import functional as F
    chosen = {}
    for B, L, D, heads, hidden in BLOCK_SHAPES:
        M = B * L
        chosen[(B, L, D)] = {F.vit_linear_tile(M, K, Nout, _forms()["auto"]) for K, Nout in ((D, 3 * D), (D, D), (D, hidden), (hidden, D))}
    assert set().union(*chosen.values()) == {(128, 128), (64, 64), (32, 64)}, chosen


@pytest.mark.parametrize("mode", ["f32", "default"])
@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_reference_block_cases_with_auto_tiles(name, mode, dev):
    """The six block cases of the reference fixture, through the module with ``small_tiles``, at their existing gate."""
    from stgcn_amd.altformer import Block, set_head_math, set_low_latency
    ref = load_golden("altformer_reference")
    blk = ar.build_block(Block, name).to(dev)
    set_head_math(blk, None if mode == "default" else mode)
    set_low_latency(blk, min_tokens=0)
    xd = ar.make_input(name).to(dev)
    with torch.no_grad():
        assert blk.small_tiles and blk.uses_hip(xd)
        y = blk(xd)
    key = f"case.{name}.y"
    got = gather_flat(y.cpu(), ref[key + "_idx"].astype(np.int64))
    print(f"{name} {mode} auto tiles: {parity_gate(got, ref[key + '_val'], REL, f'{name} {mode} y, auto tiles'):.3e}")


# ---- training refuses the field -------------------------------------------------------------------------------------------
def test_training_entry_points_reject_a_tile_field(dev):
    from stgcn_amd import functional as F
    from stgcn_amd._capi import StgcnError
    shape = (2, 22, 256, 8, 512)
    x, params = _block_args(shape, dev)
    flat = [t for pair in params for t in pair]
    for name, fl in _forms().items():
        with pytest.raises(StgcnError) as e:
            F.vit_block_forward_train(x, flat, 8, ar.EPS, 32 ** -0.5, F.MATH_F32 | fl)
        assert e.value.code == ERR_ARG and "stgcn_vit_block_forward_train" in str(e.value), name
        dy = torch.randn(44, 512, device=dev)
        a = torch.randn(44, 256, device=dev)
        dx = torch.full((44, 256), 7.0, device=dev)
        with pytest.raises(StgcnError) as e:
            F.vit_linear_backward(dy, a, params[4][0], dx_accumulate=dx, math=F.MATH_F32 | fl)
        assert e.value.code == ERR_ARG and "stgcn_vit_linear_backward" in str(e.value), name
        torch.cuda.synchronize()
        assert (dx == 7.0).all(), "a refused call wrote its output"
    y, _ = F.vit_block_forward_train(x, flat, 8, ar.EPS, 32 ** -0.5, F.MATH_F32)          # field 0 still runs
    assert torch.equal(y, F.vit_block_forward(x, *params, 8, ar.EPS, 32 ** -0.5, F.MATH_F32))


# ---- the module at one clip -----------------------------------------------------------------------------------------------
def _model(style, dev):
    import stgcn_amd
    g = load_golden("model_altformer_shre")
    torch.manual_seed(int(g["model_seed"]))
    model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style, graph="graph.SHRE",
                                       graph_args={"labeling_mode": "spatial"})
    model.gcn0.load_state_dict(sub_state(g, "gcn."), strict=True)
    model.tcn0.load_state_dict(sub_state(g, "tcn."), strict=True)
    model = model.to(dev).eval()
    model.gcn0.A = torch.from_numpy(g["A_fixed"]).clone()
    return model, torch.from_numpy(g["skeleton"]).to(dev)


def _run_recording(model, x):
    from stgcn_amd.altformer import Block
    calls = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: calls.append(mod.uses_hip(args[0])))
             for m in model.modules() if isinstance(m, Block)]
    with torch.no_grad():
        out = model(x)
    for h in hooks:
        h.remove()
    return out, calls


@pytest.mark.parametrize("style", ["ST", "TS"])
def test_one_clip_runs_every_block_on_hip(style, dev):
    import stgcn_amd
    from stgcn_amd.altformer import Block
    model, clips = _model(style, dev)
    clip = clips[:1].contiguous()
    _, calls = _run_recording(model, clip)
    assert len(calls) == 12 and not any(calls), "the default policy keeps one clip on the torch path"
    stgcn_amd.set_low_latency(model, min_tokens=0)
    a, calls = _run_recording(model, clip)
    assert len(calls) == 12 and all(calls), "set_low_latency(min_tokens=0): every block on the HIP path"
    b, _ = _run_recording(model, clip)
    assert torch.equal(a, b), "two runs of the low-latency path differ"
    for m in model.modules():
        if isinstance(m, Block):
            m.force_torch = True
    t, calls = _run_recording(model, clip)
    assert not any(calls)
    print(f"{style} one clip, low latency vs torch path: {parity_gate(a, t, REL, f'{style} one clip'):.3e}")
    assert torch.equal(a.argmax(1), t.argmax(1))


@pytest.mark.parametrize("style", ["ST", "TS"])
def test_one_clip_forward_captures_and_replays(style, dev):
    """The forward is captured once (one stream, workspaces from torch's allocator inside the capture) and replayed with two
    other clips copied into the static input; each replay equals the eager low-latency result for that clip."""
    import stgcn_amd
    model, clips = _model(style, dev)
    stgcn_amd.set_low_latency(model, min_tokens=0)
    with torch.no_grad():
        eager = [model(clips[i:i + 1].contiguous()).clone() for i in range(3)]      # also warms the modules' caches
        static_in = clips[:1].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = model(static_in)
        for i in (1, 2):
            static_in.copy_(clips[i:i + 1])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, eager[i]), f"{style}: replay with clip {i} differs from the eager result"
    assert not torch.equal(eager[1], eager[2])
