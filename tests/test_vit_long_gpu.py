"""GPU tests of the streaming attention kernel (vit_attention_stream.hip) and of what it opens: sequences of 256 < L <= 4096
tokens through ``stgcn_vit_attention_stream``, ``stgcn_vit_block_forward``, ``Block`` and the ST / TS heads.  References are
fp64 (tests/altformer_ref.py), the gate is the resident kernel's: 1e-4, both criteria of ``parity_gate``."""
import functools

import pytest
import torch

import altformer_ref as ar
from _util import MATH_GATES, hostile_allocations, parity_gate
from entry_points import peaked_qkv

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
assert REL == 1e-4 and MATH_GATES["f32"][1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def attention_case(B, L, heads, hd, scale):
    """Input and fp64 reference of one attention case: computed once, shared by the tests that use it, never written to."""
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd)
    return qkv, ar.attention64(qkv, heads, hd ** -0.5 if scale is None else scale)


# ---- 1. the streaming entry point against fp64 ---------------------------------------------------------------------------
# 257 and 513 leave one valid key in the last tile for every power-of-two tile width, 512 has no masked key, 1 / 31 / 33 / 64 /
# 65 are the single-tile path and its edges, 1000 has a short last query block; 4096 is the cap.
STREAM_SHAPES = [(3, L, 8) for L in (1, 31, 33, 64, 65, 256, 257, 300, 500, 512, 513, 1000)] + [(1, 4096, 2)]


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: f"B{s[0]}-L{s[1]}-H{s[2]}")
def test_stream_entry_point_vs_fp64(shape, hd, dev):
    from stgcn_amd import functional as F
    B, L, heads = shape
    for scale in (None, 0.37):
        qkv, want = attention_case(B, L, heads, hd, scale)
        out = F.vit_attention_stream(qkv.to(dev), heads, scale)
        rel = parity_gate(out, want, REL, f"stream attention L={L} hd={hd} scale={scale}")
        print(f"stream attention B={B} L={L} heads={heads} hd={hd} scale={scale}: {rel:.3e}")
    if L > 256:                                  # the public wrapper routes what the resident kernel cannot take
        assert torch.equal(F.vit_attention(qkv.to(dev), heads, 0.37), out)


# ---- 2. streaming against resident ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [22, 180, 256])
def test_stream_agrees_with_resident(L, hd, dev):
    from stgcn_amd import functional as F
    heads = 8
    qkv, want = attention_case(3, L, heads, hd, None)
    qd = qkv.to(dev)
    res, stream = F.vit_attention(qd, heads), F.vit_attention_stream(qd, heads)
    parity_gate(res, want, REL, f"resident L={L} hd={hd} vs fp64")
    parity_gate(stream, want, REL, f"stream L={L} hd={hd} vs fp64")
    print(f"L={L} hd={hd}: stream vs resident {parity_gate(stream, res, REL, f'stream vs resident L={L} hd={hd}'):.3e}")


# ---- 3. the running maximum, on planted inputs ---------------------------------------------------------------------------
PLANTED_L, PLANTED_HD, PLANTED_B, PLANTED_HEADS = 500, 64, 2, 4


def planted_profile(case):
    j = torch.arange(PLANTED_L, dtype=torch.float32)
    if case == "rising":       # the maximum moves up in every tile, every tile rescales, early tiles underflow after the rescale
        return -60 + 120 * j / (PLANTED_L - 1)
    if case == "falling":      # the first tile fixes the maximum, later tiles contribute exp(-large)
        return 60 - 120 * j / (PLANTED_L - 1)
    prof = torch.full((PLANTED_L,), -100.0)
    prof[PLANTED_L - 1 if case == "spike_last" else 0] = 100.0
    return prof


@functools.lru_cache(maxsize=None)
def planted_case(case):
    """q = 8 u + noise and k_j = profile[j] / (8 scale) u + noise along one seeded unit vector u per head: the score of key j is
    profile[j] for every query, up to noise of a few tenths.  v is plain noise."""
    B, L, heads, hd = PLANTED_B, PLANTED_L, PLANTED_HEADS, PLANTED_HD
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(4242)
    u = torch.randn(heads, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    prof = planted_profile(case)
    qkv = torch.empty(B, L, 3, heads, hd)
    qkv[:, :, 0] = 8.0 * u + 0.01 * torch.randn(B, L, heads, hd, generator=g)
    qkv[:, :, 1] = (prof / (8.0 * scale))[None, :, None, None] * u + 0.01 * torch.randn(B, L, heads, hd, generator=g)
    qkv[:, :, 2] = torch.randn(B, L, heads, hd, generator=g)
    s = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0].double(), qkv[:, :, 1].double()) * scale
    qkv = qkv.reshape(B, L, 3 * heads * hd)
    return qkv, s, ar.attention64(qkv, heads, scale)


@pytest.mark.parametrize("case", ["rising", "falling", "spike_last", "spike_first"])
def test_running_maximum_on_planted_scores(case, dev):
    from stgcn_amd import functional as F
    qkv, s, want = planted_case(case)
    lo, hi = s.min(dim=-1).values, s.max(dim=-1).values
    if case in ("rising", "falling"):            # about -60 .. +60 for every query: exp(range) overflows fp32
        assert (hi - lo).min().item() > 89 and hi.min().item() > 50 and lo.max().item() < -50, (lo.max().item(), hi.min().item())
        first, last = s[..., :64].max(dim=-1).values, s[..., -64:].max(dim=-1).values
        assert ((last - first).min().item() > 89) if case == "rising" else ((first - last).min().item() > 89)
    else:                                        # as test_attention_subtracts_the_row_maximum: exp(89) > fp32 max
        assert hi.min().item() > 89 and lo.max().item() < -89, (lo.max().item(), hi.min().item())
        at = s.argmax(dim=-1)
        assert bool((at == (PLANTED_L - 1 if case == "spike_last" else 0)).all())
    assert torch.isfinite(want).all() and want.abs().max().item() > 0.5, "the fp64 reference itself"
    out = F.vit_attention_stream(qkv.to(dev), PLANTED_HEADS)
    print(f"planted {case}: {parity_gate(out, want, REL, f'planted scores, {case}'):.3e}")


# ---- 4. many workgroups --------------------------------------------------------------------------------------------------
# (B, L, heads, hd): the first is 1200 * 8 pairs of 3 query blocks = 28,800 workgroups; the second 4097 * 8 pairs of 2 query
# blocks = 65,552, past the 65,535 that a grid's y and z dimensions (and 16-bit index arithmetic) stop at.
@pytest.mark.parametrize("shape", [(1200, 300, 8, 32), (4097, 129, 8, 32)], ids=lambda s: "x".join(map(str, s)))
def test_many_workgroups(shape, dev):
    from stgcn_amd import functional as F
    B, L, heads, hd = shape
    g = torch.Generator(device=dev).manual_seed(B + L)
    qkv = torch.randn(B, L, 3, heads, hd, generator=g, device=dev)
    qkv[:, :, :2] *= 2.3
    qkv = qkv.reshape(B, L, 3 * heads * hd)
    out = F.vit_attention_stream(qkv, heads)
    idx = ar.sample_idx(B, 64, 77).long()
    idx[0], idx[1] = 0, B - 1                    # the first and the last workgroups are in the sample
    want = ar.attention64(qkv[idx.to(dev)].cpu(), heads, hd ** -0.5)
    print(f"many workgroups {shape}: {parity_gate(out[idx.to(dev)], want, REL, f'many workgroups {shape}'):.3e}")
    assert torch.isfinite(out).all()


# ---- 5. bit-identical reruns ---------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(dev):
    from stgcn_amd import functional as F
    qkv, _ = attention_case(3, 500, 8, 64, None)
    qd = qkv.to(dev)
    assert torch.equal(F.vit_attention_stream(qd, 8), F.vit_attention_stream(qd, 8))


# ---- 6. buffer discipline ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [257, 513])
def test_stream_under_poisoned_guard_banded_buffers(L, hd, dev):
    """Input and output between 1 MiB guard bands, everything pre-filled with NaN bytes, then with huge finite values: the guards
    stay intact, every element of ``out`` is written and equals the run on plain buffers bit for bit (a read past the end of
    qkv, or of a key past L, would bring the poison in), and qkv is unchanged."""
    from stgcn_amd import functional as F
    B, heads = 3, 8
    qkv, want = attention_case(B, L, heads, hd, None)
    plain = F.vit_attention_stream(qkv.to(dev), heads)
    parity_gate(plain, want, REL, f"plain buffers L={L} hd={hd}")
    for fill in (0xFF, 0x7F):
        with hostile_allocations(fill) as h:
            qd = torch.empty(qkv.shape, device=dev, dtype=torch.float32)
            qd.copy_(qkv)
            out = F.vit_attention_stream(qd, heads)
            torch.cuda.synchronize()
            h.check()
            assert [r[2] for r in h.records][:2] == [(B, L, 3 * heads * hd), (B, L, heads * hd)], "qkv and out are guard-banded"
        assert torch.isfinite(out).all(), f"fill 0x{fill:02X}: an element of out was not written, or poison was read"
        assert torch.equal(out, plain), f"fill 0x{fill:02X}: the result depends on what surrounds the buffers"
        assert torch.equal(qd.cpu(), qkv), "qkv was written to"


# ---- 7. the block entry point --------------------------------------------------------------------------------------------
BLOCK_SHAPES = [(3, 300, 512, 8, 1024), (2, 500, 256, 8, 512), (70, 500, 256, 8, 512)]      # the last: 35,000 tokens = two slabs


@functools.lru_cache(maxsize=None)
def block_case(shape, dev):
    """State, input and the fp64 restatement (on the device: the CPU would take tens of seconds at 35,000 tokens)."""
    B, L, D, heads, hidden = shape
    sd = ar.random_block_state(D, hidden, True, seed=B + L + D)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    want = ar.block64(x.to(dev), sdd, heads=heads)[0].cpu()
    pair = lambda n: (sdd[n + ".weight"], sdd[n + ".bias"])       # noqa: E731
    return x.to(dev), want, (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))


@pytest.mark.parametrize("mode", ["f32", "default"])
@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_entry_point_vs_fp64(shape, mode, dev):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH, _default_head_math
    B, L, D, heads, hidden = shape
    assert F.vit_block_forward_supported(L, D, heads, hidden) and not F.vit_block_supported(L, D, heads, hidden)
    xd, want, params = block_case(shape, dev)
    math = _default_head_math() if mode == "default" else HEAD_MATH[mode]
    scale = (D // heads) ** -0.5
    y = F.vit_block_forward(xd, *params, heads, ar.EPS, scale, math)
    print(f"block {shape} {mode}: {parity_gate(y, want, REL, f'block {shape} {mode}'):.3e}")
    if B * L > 32768:                            # two slabs (65 + 5 sequences) against the two halves of the batch, one slab each
        h = B // 2
        halves = torch.cat([F.vit_block_forward(xd[:h].contiguous(), *params, heads, ar.EPS, scale, math),
                            F.vit_block_forward(xd[h:].contiguous(), *params, heads, ar.EPS, scale, math)])
        assert torch.equal(y, halves), "the slab walk changes the result"


# ---- 8. module routing ---------------------------------------------------------------------------------------------------
def test_block_module_routes_long_sequences(dev):
    from stgcn_amd.altformer import Block
    torch.manual_seed(5)
    blk = Block(256, 8, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer())
    ar.prepare_block(blk, 5)
    blk = blk.to(dev).eval()
    blk.hip_min_tokens = 0
    x = torch.randn(4, 300, 256, device=dev)
    with torch.no_grad():
        assert blk.uses_hip(x) and blk.hip_applies(x), "a 300-token sequence runs on the kernels"
        assert blk.uses_hip(x[:, :256]) and not blk.uses_hip(torch.randn(1, 4097, 256, device=dev))
        y = blk(x)
        blk.force_torch = True
        assert not blk.uses_hip(x)
        t = blk(x)
        blk.force_torch = False
    print(f"Block (4, 300, 256) HIP vs torch path: {parity_gate(y, t, REL, 'Block at L = 300, HIP vs torch path'):.3e}")
    blk.hip_train_min_tokens = 0
    xg = x.clone().requires_grad_()
    assert not blk.trains_on_hip(xg) and not blk.uses_hip(xg), "training stops at 256 tokens per sequence"
    assert blk.trains_on_hip(x[:, :256].clone().requires_grad_())
    out = blk(xg)
    parity_gate(out.detach(), t, 1e-5, "torch path under autograd vs torch path")
    out.sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all() and xg.grad.abs().sum().item() > 0
    assert all(p.grad is not None for p in blk.parameters())


# ---- 9. a head at a long clip --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_head_at_300_frames(cls_name, dev):
    from stgcn_amd import altformer
    from stgcn_amd.altformer import Block, set_hip_min_tokens
    torch.manual_seed(11)
    head = getattr(altformer, cls_name)(14, num_frame=300, num_joints=22, in_chans=128, embed_dim_ratio=256, depth=2, num_heads=8,
                                        mlp_ratio=2., qkv_bias=True, drop_path_rate=0.1)
    with torch.no_grad():
        for n, p in head.named_parameters():
            if n.endswith("pos_embed"):
                p.copy_(0.05 * torch.randn(p.shape))
    set_hip_min_tokens(head, 0)
    head = head.to(dev).eval()
    z = torch.randn(2, 128, 300, 22, device=dev)
    blocks = [m for m in head.modules() if isinstance(m, Block)]
    calls = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: calls.append((args[0].shape[1], mod.uses_hip(args[0])))) for m in blocks]
    with torch.no_grad():
        logits = head(z)
        for hk in hooks:
            hk.remove()
        assert len(calls) == 4 and all(on for _, on in calls), calls
        assert sorted(L for L, _ in calls) == [22, 22, 300, 300]
        for m in blocks:
            m.force_torch = True
        want = head(z)
    print(f"{cls_name} at 300 frames: {parity_gate(logits, want, REL, f'{cls_name} at 300 frames, HIP vs torch path'):.3e}")
    assert torch.equal(logits.argmax(1), want.argmax(1))
