"""GPU tests of the heads' bf16 TRAINING mode (``VIT_TRAIN_BF16``; include/stgcn_hip.h, DESIGN section 15 "bf16").

Three kinds of reference:
* fp64 products of operands rounded to bf16 by torch on the CPU, for ``stgcn_vit_linear_backward`` alone: a bf16 x bf16 product
  is exact in fp32, so the kernel differs from it by the order of its fp32 sums only and holds the fp32 contract (1e-4, both
  criteria of ``parity_gate``);
* fp64 autograd (``altformer_train_ref.grads64``) and the reference's gradient fixture, for a block: 1e-2 of max|.| per tensor,
  the project's gate for bf16 operands (``MATH_GATES['bf16']``, max-norm only);
* the fp64 emulation of the mode (tests/altformer_bf16_train_ref.py), for a block: ||kernels - emulation|| <= 0.45 ||emulation -
  fp64|| per tensor.  0.45 sits between the largest ratio an fp32 run of the emulation reaches on the CPU (0.26: the kernels'
  fp32 noise) and the smallest ratio a single missing rounding point produces (0.675), so the bound tells "the same rounding
  points" from "one missing or extra".  ``dmlp.fc2.bias`` sums unrounded values, the emulation equals fp64 there: 1e-4 of fp64.

The mode under test is ``HEAD_TRAIN_MATH['bf16']``, whose qkv forward runs in f32.  The entry points also take the bit with a
bf16x3 qkv forward; that combination holds the 1e-2 gate and is tested for it, but not the L2 bound (0.40-0.49 measured: the
emulation has an unrounded qkv forward, and one with a bf16x3 qkv forward gives the same 0.49 on the CPU).
"""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF
from torch.nn.parallel import parallel_apply

import altformer_bf16_train_ref as br
import altformer_ref as ar
import altformer_train_ref as tr
from _util import MATH_GATES, gather_flat, load_golden, parity_gate
from test_altformer_gpu import gate_on_device, small_head, whole_model
from test_altformer_train_gpu import block_params, compare_grads, named_grads, set_force_torch, step

pytestmark = pytest.mark.gpu
REL32 = MATH_GATES["f32"][0]
GATE, GATE_STRICT = MATH_GATES["bf16"]
L2_BOUND = 0.45
LINEAR_SHAPES = [(1, 256, 256), (1, 512, 1536), (33, 32, 4), (129, 512, 512), (300, 256, 200), (1000, 256, 768), (1472, 512, 1536),
                 (5760, 1024, 512), (126720, 256, 768)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def train_bf16():
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    return HEAD_TRAIN_MATH["bf16"]


# ---- stgcn_vit_linear_backward with the bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_backward_bf16_vs_fp64_of_rounded_operands(shape, dev):
    from stgcn_amd import functional as F
    M, K, Nout = shape
    g = torch.Generator(device=dev).manual_seed(M + K + Nout)
    dy = torch.randn(M, Nout, generator=g, device=dev) * (0.25 + 3.75 * torch.rand(M, 1, generator=g, device=dev))
    a = torch.randn(M, K, generator=g, device=dev) + 0.5
    W = (torch.rand(Nout, K, generator=g, device=dev) * 2 - 1) / K ** 0.5
    h = torch.randn(M, K, generator=g, device=dev) * 1.5
    old = torch.randn(M, K, generator=g, device=dev)
    mode = F.MATH_BF16X3 | F.VIT_TRAIN_BF16
    assert F.vit_linear_backward_bf16_supported(M, K, Nout)
    rdy, ra, rW = (t.cpu().bfloat16().double().to(dev) for t in (dy, a, W))      # rounded here, not by the kernel
    assert not torch.equal(rdy, dy.double()) and not torch.equal(ra, a.double())
    base = rdy @ rW
    h64 = h.double().requires_grad_(True)
    TF.gelu(h64).sum().backward()
    for dgelu, accum in itertools.product((False, True), repeat=2):
        want = base * h64.grad if dgelu else base
        if accum:
            want = want + old.double()
        dx, _, _ = F.vit_linear_backward(dy, a, W, h_pre=h if dgelu else None, dx_accumulate=old.clone() if accum else None,
                                         need_dw=False, math=mode)
        gate_on_device(dx, want, REL32, f"linear backward bf16 {shape} dx gelu'={dgelu} accumulate={accum}")
    _, dW, db = F.vit_linear_backward(dy, a, W, need_dx=False, math=mode)
    gate_on_device(dW, rdy.T @ ra, REL32, f"linear backward bf16 {shape} dW")
    gate_on_device(db, dy.double().sum(0), REL32, f"linear backward bf16 {shape} db (the unrounded column sums)")
    _, dW2, none = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=False, math=mode)
    assert none is None and torch.equal(dW, dW2), "the weight gradient is bit-identical from run to run"
    if M >= 129:
        _, dW32, _ = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=False, math=F.MATH_F32)
        assert not torch.equal(dW, dW32), "the bit changes the arithmetic"


# ---- one block ------------------------------------------------------------------------------------------------------------------
def run_block(blk, x, dy, math, s1=None, s2=None):
    from stgcn_amd import functional as F
    ps = [None if p is None else p.detach() for p in block_params(blk)]
    args = (blk.attn.num_heads, blk.norm1.eps, blk.attn.scale, math, s1, s2)
    y, saved = F.vit_block_forward_train(x, ps, *args)
    g = F.vit_block_backward(x, ps, saved, dy, *args)
    return y, {"x": g["x"], **{k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS)}}


@functools.lru_cache(maxsize=None)
def case_reference(name, factors):
    """Inputs, fp64 autograd and the emulation of a block case: computed once, on the CPU, shared and left unchanged."""
    x, sd, dy, scale, s1, s2 = br.case_inputs(name, factors)
    kw = dict(scale=scale, s1=s1, s2=s2)
    return (x, sd, dy, scale, s1, s2), tr.grads64(x, sd, dy, **kw), br.grads_bf16(x, sd, dy, **kw)


def gate_block(what, y, g, ref64, emu):
    """The three gates of a block result against fp64 autograd and the emulation; prints every figure before it asserts."""
    (y64, g64), (ye, ge) = ref64, emu
    rows = [("y", y, y64, ye)] + [("d" + k, g[k], g64[k], ge[k]) for k in g64]
    figures = []
    for k, got, want, em in rows:
        got = got.detach().double().cpu()
        rel = ((got - want).abs().max() / want.abs().max()).item()
        ratio = br.l2_ratio(got, em, want) if k != "dmlp.fc2.bias" else float("nan")
        print(f"{what} {k}: vs fp64 {rel:.3e}; L2 ratio to the emulation {ratio:.3f}")
        figures.append((k, got, want, rel, ratio))
    for k, got, want, rel, ratio in figures:
        parity_gate(got, want, GATE, f"{what} {k}", GATE_STRICT)
        if k == "dmlp.fc2.bias":
            parity_gate(got, want, REL32, f"{what} {k} (unrounded sums)", False)
        else:
            assert ratio <= L2_BOUND, f"{what} {k}: L2 ratio to the emulation {ratio:.3f} > {L2_BOUND}"


def gate_stored(out, ref, key, what):
    if key in ref:
        rel = parity_gate(out, ref[key], GATE, what, GATE_STRICT)
    else:
        rel = parity_gate(gather_flat(out.detach().cpu(), ref[key + "_idx"].astype(np.int64)), ref[key + "_val"], GATE, what, GATE_STRICT)
    print(f"{what}: vs the fixture {rel:.3e}")


@pytest.mark.parametrize("factors", [False, True], ids=["plain", "stochastic_depth"])
@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_gradients_bf16(name, factors, dev):
    from stgcn_amd.altformer import Block
    (x, _, dy, _, s1, s2), ref64, emu = case_reference(name, factors)
    blk = ar.build_block(Block, name).to(dev)
    on = lambda t: None if t is None else t.to(dev)       # noqa: E731
    y, g = run_block(blk, x.to(dev), dy.to(dev), train_bf16(), on(s1), on(s2))
    if g["attn.qkv.bias"] is None:
        assert "attn.qkv.bias" not in ref64[1]
        del g["attn.qkv.bias"]
    if not factors:            # the reference project's own gradients
        ref, fwd, pre = load_golden("altformer_train_reference"), load_golden("altformer_reference"), f"case.{name}."
        gate_stored(y, fwd, pre + "y", f"{name} bf16 y")
        for k, v in g.items():
            gate_stored(v, ref, pre + "d" + k, f"{name} bf16 d{k}")
    gate_block(f"{name} bf16 {'masked' if factors else 'plain'}", y, g, ref64, emu)
    if factors:
        dropped = ((s1 == 0) & (s2 == 0)).to(dev)
        if dropped.any():
            assert torch.equal(g["x"][dropped], dy.to(dev)[dropped]), "a sequence with both branches dropped: dx = dy"
        y32, _ = run_block(blk, x.to(dev), dy.to(dev), 0, on(s1), on(s2))
        assert not torch.equal(y, y32), "the bit changes the forward"


@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_with_a_bf16x3_qkv_forward_holds_the_gate(name, dev):
    """The other arithmetic the contract allows for the qkv forward: 1e-2 of max|.| against fp64 on every tensor.  Its L2
    ratios to the emulation are printed, not bounded (see the module docstring)."""
    from stgcn_amd import _capi
    from stgcn_amd.altformer import Block
    (x, _, dy, _, s1, s2), (y64, g64), (ye, ge) = case_reference(name, True)
    blk = ar.build_block(Block, name).to(dev)
    y, g = run_block(blk, x.to(dev), dy.to(dev), _capi.VIT_TRAIN_BF16 | _capi.MATH_BF16X3, s1.to(dev), s2.to(dev))
    rels = {"y": parity_gate(y, y64, GATE, f"{name} y", GATE_STRICT)}
    for k, v in g64.items():
        rels["d" + k] = parity_gate(g[k], v, GATE, f"{name} d{k}", GATE_STRICT)
    ratios = {k: br.l2_ratio(g[k], ge[k], g64[k]) for k in g64 if k != "mlp.fc2.bias"}
    print(f"{name} bit | bf16x3: worst vs fp64 {max(rels.values()):.3e}; largest L2 ratio {max(ratios.values()):.3f} on "
          f"d{max(ratios, key=ratios.get)}")


def test_dropped_sequence_passes_dy_through_exactly(dev):
    """Both factors 0 for sequence 1: its dx is dy bit for bit, whatever the arithmetic of the products."""
    from stgcn_amd.altformer import Block
    name = "st_spatial_L22_D256"
    blk = ar.build_block(Block, name).to(dev)
    x, dy = ar.make_input(name).to(dev), tr.make_dy(name).to(dev)
    s1 = torch.full((x.shape[0],), 1 / 0.9, device=dev)
    s2 = s1.clone()
    s1[1] = s2[1] = 0.0
    s2[2] = 0.0
    y, g = run_block(blk, x, dy, train_bf16(), s1, s2)
    assert torch.equal(g["x"][1], dy[1]) and torch.equal(y[1], x[1]) and not torch.equal(g["x"][2], dy[2])


def test_streaming_plan_bf16(dev):
    """L = 300: the streaming attention forward and backward between the bf16 linears.  The input was checked on the CPU first
    (python tests/altformer_bf16_train_ref.py): emulation error 4.4e-3 <= 5e-3, fp32-noise L2 ratio 0.12 <= 0.3, with the
    q / k factor 4 of the fixture cases."""
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import Block
    x, sd, dy, scale, s1, s2 = br.stream_inputs()
    B, L, D = x.shape
    assert L > 256 and F.vit_block_train_bf16_supported(L, D, ar.HEADS, 2 * D) and not F.vit_block_train_supported(L, D, ar.HEADS, 2 * D)
    kw = dict(scale=scale, s1=s1, s2=s2)
    ref64, emu = tr.grads64(x, sd, dy, **kw), br.grads_bf16(x, sd, dy, **kw)
    assert max(br.max_rel(emu[1][k], ref64[1][k]) for k in ref64[1]) <= 5e-3, "the input keeps the emulation inside half the gate"
    blk = Block(dim=D, num_heads=ar.HEADS, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer())
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).eval()
    y, g = run_block(blk, x.to(dev), dy.to(dev), train_bf16(), s1.to(dev), s2.to(dev))
    gate_block("stream L300 D256 bf16", y, g, ref64, emu)


def test_two_runs_are_bit_identical_over_slabs_and_splits(dev):
    """3000 x 22 x 256 with factors: three slabs of whole sequences, several ranges in every weight-gradient reduction."""
    from stgcn_amd import _capi
    from stgcn_amd.altformer import Block
    blk = ar.build_block(Block, "st_spatial_L22_D256").to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(3000, 22, 256, device=dev, generator=g)
    dy = torch.randn(3000, 22, 256, device=dev, generator=g)
    s1, s2 = (t.to(dev) for t in tr.make_scales(3000, 1))
    assert 3000 * 22 > 2 * 32768 and _capi.lib().stgcn_vit_block_backward_ws_bytes(3000, 22, 256, 512) == \
        _capi.lib().stgcn_vit_block_backward_ws_bytes(6000, 22, 256, 512), "the input is walked in slabs"
    y1, g1 = run_block(blk, x, dy, train_bf16(), s1, s2)
    y2, g2 = run_block(blk, x, dy, train_bf16(), s1, s2)
    assert torch.equal(y1, y2) and len(g1) == 13
    for k in g1:
        assert torch.isfinite(g1[k]).all() and torch.equal(g1[k], g2[k]), f"d{k} differs between two runs"


# ---- poisoned, guard-banded buffers ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _poison_reference(L):
    if L == 22:
        return case_reference("st_spatial_L22_D256", True)[:2]
    B, D = 3, 256
    g = torch.Generator().manual_seed(900 + L)
    sd = ar.random_block_state(D, 2 * D, seed=901 + L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    dy = torch.randn(B, L, D, generator=g)
    s1, s2 = tr.make_scales(B, 902 + L)
    scale = (D // ar.HEADS) ** -0.5
    return (x.contiguous(), sd, dy, scale, s1, s2), tr.grads64(x, sd, dy, scale=scale, s1=s1, s2=s2)


def make_block_train_bf16(L, dev):
    from stgcn_amd.altformer import Block
    (x, sd, dy, scale, s1, s2), (want_y, want) = _poison_reference(L)
    D = x.shape[-1]
    blk = Block(dim=D, num_heads=ar.HEADS, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer())
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).eval()
    xd, dyd, s1d, s2d = (t.to(dev) for t in (x, dy, s1, s2))

    def run():
        y, g = run_block(blk, xd, dyd, train_bf16(), s1d, s2d)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def gate(o, what):
        parity_gate(o["y"], want_y, GATE, f"{what} y", GATE_STRICT)
        for k, v in want.items():
            parity_gate(o["d" + k], v, GATE, f"{what} d{k}", GATE_STRICT)
    return run, gate


@pytest.mark.parametrize("L", [22, 257])
def test_block_train_bf16_under_poisoned_guard_banded_buffers(L, dev):
    """Nothing outside ``saved``, the workspace and the outputs is written, and no poison is read into a result: the outputs are
    finite, inside the gate and bit-identical under a NaN fill and a huge-number fill."""
    from _util import HostileCase as Case, run_under_both_fills
    run_under_both_fills(Case(f"vit_block_train_bf16-L{L}", functools.partial(make_block_train_bf16, L), True), dev)


# ---- modules ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def spy(monkeypatch):
    """The ``math`` of every call of functional.vit_block_forward_train / vit_block_backward."""
    from stgcn_amd import functional as F
    seen = {"forward": [], "backward": []}
    fwd, bwd = F.vit_block_forward_train, F.vit_block_backward

    def forward(x, params, heads, eps, scale, math=0, *a, **k):
        seen["forward"].append(math)
        return fwd(x, params, heads, eps, scale, math, *a, **k)

    def backward(x, params, saved, dy, heads, eps, scale, math=0, *a, **k):
        seen["backward"].append(math)
        return bwd(x, params, saved, dy, heads, eps, scale, math, *a, **k)
    monkeypatch.setattr(F, "vit_block_forward_train", forward)
    monkeypatch.setattr(F, "vit_block_backward", backward)
    return seen


def max_rel(got, want):
    return ((got.double() - want.double()).abs().max() / want.double().abs().max()).item()


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_head_logits_bf16_vs_the_torch_path(cls_name, dev, spy):
    from stgcn_amd.altformer import set_train_math
    head = small_head(dev, cls_name)                    # .eval(); its parameters require gradients: the training path
    set_train_math(head, "bf16")
    z = torch.randn(6, 128, 40, 22, device=dev)
    out = head(z)
    assert len(spy["forward"]) == 4 and all(m == train_bf16() for m in spy["forward"])
    set_force_torch(head, True)
    want = head(z)
    rel = max_rel(out, want)
    print(f"{cls_name} logits bf16 vs torch ops: {rel:.3e} of max|logit|")
    assert torch.isfinite(out).all() and rel <= GATE


def test_st_spatial_stage_gradients_bf16_vs_the_torch_path(dev, spy):
    """Two blocks and a mean pooling (no max pooling, whose gradient moves between tokens at this error level): every parameter
    gradient and dz within 1e-2 of max|.| of the torch path's, in .train() with the same seed (the same masks)."""
    from stgcn_amd.altformer import set_train_math
    head = small_head(dev, "ST").train()
    set_train_math(head, "bf16")
    z = torch.randn(6, 128, 40, 22, device=dev)

    class Stage(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.head = head

        def forward(self, x):
            return self.head.Spatial_forward_features(x)
    stage = Stage()
    out, dz, grads = step(stage, z, 77)
    assert len(spy["forward"]) == 2 == len(spy["backward"]) and all(m == train_bf16() for m in spy["forward"] + spy["backward"])
    set_force_torch(head, True)
    out_t, dz_t, grads_t = step(stage, z, 77)
    got = {k: v for k, v in grads.items() if v is not None}
    want = {k: v for k, v in grads_t.items() if v is not None}
    assert got.keys() == want.keys() and len(want) == 27, "27 parameter gradients; with dz, 28 gradient tensors"
    figures = [("out", out, out_t), ("dz", dz, dz_t)] + [("d" + k, got[k], want[k]) for k in want]
    for k, a, b in figures:
        print(f"ST spatial stage bf16 {k}: {max_rel(a, b):.3e}")
    for k, a, b in figures:
        assert torch.isfinite(a).all() and max_rel(a, b) <= GATE, k


UNUSED = ("Spatial_cls_token", "cls_token", "Spatial_norm.", "Temporal_norm.", "weighted_mean.", "fcn.")


def check_training_step(module, inp, blocks, spy, loss):
    def is_unused(k):
        return any(part.startswith(UNUSED) for part in (k, k.split(".", 1)[-1]))
    out, _, grads = step(module, inp, 5, loss, need_dz=False)
    assert len(spy["forward"]) == blocks == len(spy["backward"]), "every Block ran the training entry points"
    assert all(m == train_bf16() for m in spy["forward"] + spy["backward"]), "with the bit"
    for k, v in grads.items():
        if not k.startswith(("gcn0.", "tcn0.")):         # the stem's own parameters: whatever its own tests say, but finite
            assert (v is None) == is_unused(k), k
        assert v is None or torch.isfinite(v).all(), k
    out2, _, grads2 = step(module, inp, 5, loss, need_dz=False)
    assert torch.equal(out, out2)
    for k, v in grads.items():
        assert v is None or torch.equal(v, grads2[k]), f"d{k} differs between two steps from the same seed"


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_whole_head_trains_in_bf16(cls_name, dev, spy):
    from stgcn_amd.altformer import set_train_math
    head = small_head(dev, cls_name).train()
    set_train_math(head, "bf16")
    check_training_step(head, torch.randn(6, 128, 40, 22, device=dev), 4, spy, lambda o: (o * o).sum())


def test_whole_model_trains_in_bf16(dev, spy):
    from stgcn_amd.altformer import set_train_math
    model, g = whole_model(None, dev)
    set_train_math(model, "bf16")
    model.train()
    labels = torch.arange(8, device=dev) % 14
    ce = torch.nn.CrossEntropyLoss()
    check_training_step(model, torch.from_numpy(g["skeleton"]).to(dev), 24, spy, lambda o: ce(o, labels))


def test_without_set_train_math_no_call_carries_the_bit(dev, spy):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import set_head_math
    head = small_head(dev, "ST").train()
    step(head, torch.randn(6, 128, 40, 22, device=dev), 5)
    set_head_math(head, "bf16")                       # the inference mode leaves training in its default arithmetic
    step(head, torch.randn(6, 128, 40, 22, device=dev), 5)
    assert len(spy["forward"]) == 8 == len(spy["backward"])
    assert all(m & F.VIT_TRAIN_BF16 == 0 for m in spy["forward"] + spy["backward"])


def test_replicas_send_their_bf16_gradients_to_the_master(dev, spy):
    """Each replica runs what the same half runs on the master alone (same kernels, same shapes: the same bits), and the sum of
    two gradients is one fp32 addition, so the fp32 gate of the f32 replica test holds here too."""
    from stgcn_amd.altformer import set_train_math
    from test_data_parallel import _replicas
    head = small_head(dev, "ST")                      # .eval(): no masks, so the halves can be compared one by one
    set_train_math(head, "bf16")
    z = torch.randn(8, 128, 40, 22, device=dev)
    want = None
    for half in (z[:4], z[4:]):
        _, _, gh = step(head, half, 1, lambda o: o.sum())
        want = gh if want is None else {k: None if v is None else v + gh[k] for k, v in want.items()}
    for p in head.parameters():
        p.grad = None
    n = len(spy["forward"])
    outs = parallel_apply(_replicas(head, 2), [(z[:4],), (z[4:],)], devices=[dev, dev])
    (outs[0].sum() + outs[1].sum()).backward()
    assert len(spy["forward"]) == n + 8 and all(m == train_bf16() for m in spy["forward"] + spy["backward"])
    compare_grads(named_grads(head), want, "two bf16 replicas vs the sum of the halves")
