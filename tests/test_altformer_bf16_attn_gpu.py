"""GPU tests of the training attention on bf16 matrix operands (``VIT_TRAIN_ATTN_BF16``; include/stgcn_hip.h, DESIGN section 15
"bf16 attention", csrc/vit_attention_train_bf16.hip).

References: fp64 autograd of the unrounded attention / block, and the fp64 emulation of the contract
(tests/altformer_bf16_attn_ref.py).  Bounds, none of them taken from the kernels:

* the two kernels alone, per tensor of out, dq, dk, dv: ``||kernel - emulation|| <= ATTN_L2_BOUND ||emulation - fp64||`` with
  ``ATTN_L2_BOUND`` = 0.1.  On the CPU an fp32 torch run of the emulation (the kernels' fp32 noise) reaches 0.039 at most and a
  single missing rounding point moves the most affected tensor by 0.225 at least (tests/test_altformer_bf16_attn_host.py
  measures both); 0.1 is their geometric mean.  And ``||kernel - fp64|| <= (1 + ATTN_L2_BOUND) EMULATION_DISTANCE ||fp64||``,
  the largest distance of the emulation from fp64 that the host test measures on these same inputs, plus the same margin;
* one block, ``HEAD_TRAIN_MATH['bf16'] | VIT_TRAIN_ATTN_BF16``: every tensor within ``MATH_GATES['bf16']`` (1e-2 of max|.|) of
  fp64 autograd, and within ``BLOCK_L2_BOUND`` = 0.8 of the emulation in the same L2 ratio.  That bound is twice what the fp32
  run of the block emulation reaches (0.39), so it catches gross errors only (plain-bf16 scores: 2.06): a missing weak point
  of the attention drowns in the fp32 noise of a whole block, and only the attention-level test above can see it.

Whole-head gradients are not compared in the max norm (the max pooling's ties)."""
import functools

import pytest
import torch
from torch.nn.parallel import parallel_apply

import altformer_bf16_attn_ref as at
import altformer_bf16_train_ref as br
import altformer_ref as ar
import altformer_train_ref as tr
from _util import MATH_GATES, parity_gate
from test_altformer_bf16_train_gpu import UNUSED, _poison_reference, case_reference, max_rel, run_block, spy  # noqa: F401 (spy: a fixture)
from test_altformer_gpu import small_head
from test_altformer_train_gpu import compare_grads, named_grads, set_force_torch, step

pytestmark = pytest.mark.gpu
REL32 = MATH_GATES["f32"][0]
GATE, GATE_STRICT = MATH_GATES["bf16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def modes():
    """(the bf16 training mode, the same with the bf16 attention)."""
    from stgcn_amd import _capi
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    return HEAD_TRAIN_MATH["bf16"], HEAD_TRAIN_MATH["bf16"] | _capi.VIT_TRAIN_ATTN_BF16


# ---- the two kernels alone ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attention_reference(kind, L, hd):
    """Inputs, the fp64 attention and the emulation of one case: computed once, on the CPU, shared and left unchanged."""
    qkv, dout, heads, scale = at.attention_case(kind, L, hd)
    return (qkv, dout, heads, scale), at.attention_grads64(qkv, dout, heads, scale), at.attention_grads(qkv, dout, heads, scale)


def run_attention(qkv, dout, heads, scale):
    from stgcn_amd import functional as F
    out = F.vit_attention_train_bf16(qkv, heads, scale)
    dqkv = F.vit_attention_backward_bf16(qkv, out, dout, heads, scale)
    B, L, D3 = qkv.shape
    g = dqkv.reshape(B, L, 3, D3 // 3)
    return {"out": out, "dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}


@pytest.mark.parametrize("kind,L,hd", at.ATTN_CASES, ids=[f"{k}-L{L}-hd{hd}" for k, L, hd in at.ATTN_CASES])
def test_attention_kernels_vs_the_emulation(kind, L, hd, dev):
    from stgcn_amd import functional as F
    (qkv, dout, heads, scale), g64, ge = attention_reference(kind, L, hd)
    assert F.vit_attention_train_bf16_supported(L, heads, hd)
    qd, dd = qkv.to(dev), dout.to(dev)
    got = run_attention(qd, dd, heads, scale)
    figures = []
    for t in at.TENSORS:
        g = got[t].double().cpu()
        ratio = br.l2_ratio(g, ge[t], g64[t])
        dist = (g - g64[t]).norm().item()
        print(f"{kind} L{L} hd{hd} {t}: L2 ratio to the emulation {ratio:.4f}; ||kernel - fp64|| / ||fp64|| "
              f"{dist / max(g64[t].norm().item(), 1e-300):.3e}")
        figures.append((t, g, ratio, dist))
    for t, g, ratio, dist in figures:
        assert torch.isfinite(g).all(), t
        assert ratio <= at.ATTN_L2_BOUND, f"{t}: L2 ratio to the emulation {ratio:.4f} > {at.ATTN_L2_BOUND}"
        assert dist <= (1 + at.ATTN_L2_BOUND) * at.EMULATION_DISTANCE[t] * g64[t].norm().item(), t
    again = run_attention(qd, dd, heads, scale)
    for t in at.TENSORS:
        assert torch.equal(got[t], again[t]), f"{t} differs between two runs"


def test_attention_bf16_is_not_the_fp32_kernel(dev):
    from stgcn_amd import functional as F
    (qkv, dout, heads, scale), _, _ = attention_reference("derived", 180, 32)
    qd = qkv.to(dev)
    assert not torch.equal(F.vit_attention_train_bf16(qd, heads, scale), F.vit_attention(qd, heads, scale))


# ---- one block --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_emulation(name, factors):
    (x, sd, dy, scale, s1, s2), _, _ = case_reference(name, factors)
    return at.block_grads(x, sd, dy, scale=scale, s1=s1, s2=s2)


def gate_block(what, y, g, ref64, emu, l2_bound):
    """The gate against fp64 autograd and the L2 bound against the emulation; prints every figure before it asserts."""
    (y64, g64), (ye, ge) = ref64, emu
    rows = [("y", y, y64, ye)] + [("d" + k, g[k], g64[k], ge[k]) for k in g64]
    figures = []
    for k, got, want, em in rows:
        got = got.detach().double().cpu()
        rel = ((got - want).abs().max() / want.abs().max()).item()
        ratio = br.l2_ratio(got, em, want) if k != "dmlp.fc2.bias" and em is not None else float("nan")
        print(f"{what} {k}: vs fp64 {rel:.3e}; L2 ratio to the emulation {ratio:.3f}")
        figures.append((k, got, want, ratio))
    for k, got, want, ratio in figures:
        parity_gate(got, want, GATE, f"{what} {k}", GATE_STRICT)
        if k == "dmlp.fc2.bias":
            parity_gate(got, want, REL32, f"{what} {k} (unrounded sums)", False)
        elif l2_bound is not None:
            assert ratio <= l2_bound, f"{what} {k}: L2 ratio to the emulation {ratio:.3f} > {l2_bound}"


def block_on(dev, name, factors, math):
    from stgcn_amd.altformer import Block
    (x, _, dy, _, s1, s2), ref64, _ = case_reference(name, factors)
    blk = ar.build_block(Block, name).to(dev)
    on = lambda t: None if t is None else t.to(dev)       # noqa: E731
    y, g = run_block(blk, x.to(dev), dy.to(dev), math, on(s1), on(s2))
    if g["attn.qkv.bias"] is None:
        del g["attn.qkv.bias"]
    return y, g, ref64


@pytest.mark.parametrize("factors", [False, True], ids=["plain", "stochastic_depth"])
@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_gradients_with_the_bf16_attention(name, factors, dev):
    base, mode = modes()
    y, g, ref64 = block_on(dev, name, factors, mode)
    gate_block(f"{name} bf16 + bf16 attention {'masked' if factors else 'plain'}", y, g, ref64, block_emulation(name, factors),
               at.BLOCK_L2_BOUND)
    if factors:
        y0, g0, _ = block_on(dev, name, factors, base)
        assert not torch.equal(y, y0) and not torch.equal(g["attn.qkv.weight"], g0["attn.qkv.weight"]), "the bit changes the arithmetic"


@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_the_flag_on_f32_linears_holds_the_gate(name, dev):
    """The bit on top of the f32 low bits alone (fp32 linears, bf16 attention): 1e-2 of max|.| against fp64 on every tensor."""
    from stgcn_amd import _capi
    y, g, ref64 = block_on(dev, name, True, _capi.MATH_F32 | _capi.VIT_TRAIN_ATTN_BF16)
    gate_block(f"{name} f32 + bf16 attention", y, g, ref64, (None, dict.fromkeys(ref64[1])), None)


def test_streaming_plan_is_untouched_by_the_flag(dev):
    """L = 300: the plan leaves the fp32 streaming kernels in place, so the flag changes no bit."""
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import Block
    x, sd, dy, scale, s1, s2 = br.stream_inputs()
    B, L, D = x.shape
    assert L > 256 and F.vit_block_train_bf16_supported(L, D, ar.HEADS, 2 * D) and not F.vit_block_train_attn_bf16_supported(L, D, ar.HEADS, 2 * D)
    blk = Block(dim=D, num_heads=ar.HEADS, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer())
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).eval()
    base, mode = modes()
    args = (x.to(dev), dy.to(dev))
    y0, g0 = run_block(blk, *args, base, s1.to(dev), s2.to(dev))
    y1, g1 = run_block(blk, *args, mode, s1.to(dev), s2.to(dev))
    assert torch.equal(y0, y1) and len(g0) == 13
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"d{k} differs with the flag at a streaming length"


def test_two_runs_are_bit_identical_over_slabs(dev):
    """3000 x 22 x 256 with factors: three slabs of whole sequences."""
    from stgcn_amd.altformer import Block
    blk = ar.build_block(Block, "st_spatial_L22_D256").to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(3000, 22, 256, device=dev, generator=g)
    dy = torch.randn(3000, 22, 256, device=dev, generator=g)
    s1, s2 = (t.to(dev) for t in tr.make_scales(3000, 1))
    mode = modes()[1]
    y1, g1 = run_block(blk, x, dy, mode, s1, s2)
    y2, g2 = run_block(blk, x, dy, mode, s1, s2)
    assert torch.equal(y1, y2) and len(g1) == 13
    for k in g1:
        assert torch.isfinite(g1[k]).all() and torch.equal(g1[k], g2[k]), f"d{k} differs between two runs"


# ---- poisoned, guard-banded buffers ----------------------------------------------------------------------------------------------
def make_block_train_attn_bf16(L, dev):
    from stgcn_amd.altformer import Block
    (x, sd, dy, scale, s1, s2), (want_y, want) = _poison_reference(L)
    D = x.shape[-1]
    blk = Block(dim=D, num_heads=ar.HEADS, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer())
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).eval()
    xd, dyd, s1d, s2d = (t.to(dev) for t in (x, dy, s1, s2))
    mode = modes()[1]

    def run():
        y, g = run_block(blk, xd, dyd, mode, s1d, s2d)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def gate(o, what):
        parity_gate(o["y"], want_y, GATE, f"{what} y", GATE_STRICT)
        for k, v in want.items():
            parity_gate(o["d" + k], v, GATE, f"{what} d{k}", GATE_STRICT)
    return run, gate


@pytest.mark.parametrize("L", [22, 256])
def test_block_under_poisoned_guard_banded_buffers(L, dev):
    """Nothing outside ``saved``, the workspace and the outputs is written, and no poison is read into a result: the outputs are
    finite, inside the gate and bit-identical under a NaN fill and a huge-number fill."""
    from _util import HostileCase as Case, run_under_both_fills
    run_under_both_fills(Case(f"vit_block_train_attn_bf16-L{L}", functools.partial(make_block_train_attn_bf16, L), True), dev)


# ---- modules ----------------------------------------------------------------------------------------------------------------------
def both_switches(module):
    from stgcn_amd.altformer import set_train_attention_math, set_train_math
    set_train_math(module, "bf16")
    set_train_attention_math(module, "bf16")


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_head_logits_vs_the_torch_path(cls_name, dev, spy):  # noqa: F811
    head = small_head(dev, cls_name)                    # .eval(); its parameters require gradients: the training path
    both_switches(head)
    z = torch.randn(6, 128, 40, 22, device=dev)
    out = head(z)
    assert len(spy["forward"]) == 4 and all(m == modes()[1] for m in spy["forward"])
    set_force_torch(head, True)
    want = head(z)
    rel = max_rel(out, want)
    print(f"{cls_name} logits bf16 + bf16 attention vs torch ops: {rel:.3e} of max|logit|")
    assert torch.isfinite(out).all() and rel <= GATE


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_whole_head_trains_with_both_switches(cls_name, dev, spy):  # noqa: F811
    head = small_head(dev, cls_name).train()
    both_switches(head)
    z = torch.randn(6, 128, 40, 22, device=dev)

    def is_unused(k):
        return any(part.startswith(UNUSED) for part in (k, k.split(".", 1)[-1]))
    out, _, grads = step(head, z, 5, need_dz=False)
    assert len(spy["forward"]) == 4 == len(spy["backward"]), "every Block ran the training entry points"
    assert all(m == modes()[1] for m in spy["forward"] + spy["backward"]), "with both bits, forward and backward"
    for k, v in grads.items():
        assert (v is None) == is_unused(k), k
        assert v is None or torch.isfinite(v).all(), k
    out2, _, grads2 = step(head, z, 5, need_dz=False)
    assert torch.equal(out, out2)
    for k, v in grads.items():
        assert v is None or torch.equal(v, grads2[k]), f"d{k} differs between two steps from the same seed"


def test_without_the_switch_no_call_carries_the_bit(dev, spy):  # noqa: F811
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import set_train_attention_math, set_train_math
    head = small_head(dev, "ST").train()
    set_train_math(head, "bf16")
    step(head, torch.randn(6, 128, 40, 22, device=dev), 5)
    set_train_attention_math(head, "bf16")
    set_train_attention_math(head, None)
    step(head, torch.randn(6, 128, 40, 22, device=dev), 5)
    assert len(spy["forward"]) == 8 == len(spy["backward"])
    assert all(m == modes()[0] and m & F.VIT_TRAIN_ATTN_BF16 == 0 for m in spy["forward"] + spy["backward"])


def test_replicas_send_their_gradients_to_the_master(dev, spy):  # noqa: F811
    """Each replica runs what the same half runs on the master alone (same kernels, same shapes: the same bits), and the sum of
    two gradients is one fp32 addition, so the fp32 gate of the f32 replica test holds here too."""
    from test_data_parallel import _replicas
    head = small_head(dev, "ST")                      # .eval(): no masks, so the halves can be compared one by one
    both_switches(head)
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
    assert len(spy["forward"]) == n + 8 and all(m == modes()[1] for m in spy["forward"] + spy["backward"])
    compare_grads(named_grads(head), want, "two replicas with the bf16 attention vs the sum of the halves")
