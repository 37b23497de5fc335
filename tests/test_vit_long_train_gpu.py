"""GPU tests of the streaming attention backward (vit_attention_bwd_stream.hip) and of what it opens: training on sequences of
256 < L <= 4096 tokens through ``stgcn_vit_attention_backward_stream``, ``stgcn_vit_block_forward_train`` /
``stgcn_vit_block_backward``, ``Block`` under ``set_long_training`` and the ST / TS heads.  References are fp64 autograd
(tests/altformer_ref.py, tests/altformer_train_ref.py), the gate is the project's fp32 gate: 1e-4, both criteria of
``parity_gate``."""
import functools

import pytest
import torch
import torch.nn as nn

import altformer_ref as ar
import altformer_train_ref as tr
from _util import MATH_GATES, hostile_allocations, parity_gate
from entry_points import attention_grad64, peaked_qkv
from test_altformer_train_gpu import TRAIN_STRICT, PinnedMax, compare_grads, set_force_torch, step
from test_vit_long_gpu import PLANTED_B, PLANTED_HD, PLANTED_HEADS, PLANTED_L, planted_case

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
def backward_case(B, L, heads, hd, scale, dev):
    """Inputs (on the device) and the fp64 gradient (on the host) of one case: computed once, shared by the tests that use it,
    never written to.  ``out`` is the streaming forward's, as the training block hands it over."""
    from stgcn_amd import functional as F
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd).to(dev)
    dout = torch.randn(B, L, heads * hd, generator=torch.Generator().manual_seed(L + hd)).to(dev)
    _, want = attention_grad64(qkv, dout, heads, hd ** -0.5 if scale is None else scale)
    return qkv, F.vit_attention_stream(qkv, heads, scale), dout, want.cpu()


# ---- 1. the streaming entry point against fp64 autograd ------------------------------------------------------------------
# 64-row tiles and 128-row query / key blocks: 1 / 31 / 33 / 64 / 65 are the single tile and its edges, 127 / 128 / 129 one
# block and the first row of a second one (three idle waves), 257 and 513 leave one valid row in the last tile, 300 and 1000
# have a short last block; 4096 is the cap (head_dim 32 only: the fp64 reference of one case is enough of a 4096 x 4096 matrix).
STREAM_SHAPES = [(3, L, 8, hd) for L in (1, 31, 33, 64, 65, 127, 128, 129, 256, 257, 300, 513) for hd in (32, 64)] \
    + [(2, 1000, 2, 32), (2, 1000, 2, 64), (1, 4096, 1, 32)]


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: f"B{s[0]}-L{s[1]}-H{s[2]}-hd{s[3]}")
def test_stream_backward_vs_fp64(shape, dev):
    from stgcn_amd import functional as F
    B, L, heads, hd = shape
    for scale in (None, 0.37):
        qkv, out, dout, want = backward_case(B, L, heads, hd, scale, dev)
        dqkv = F.vit_attention_backward_stream(qkv, out, dout, heads, scale)
        rel = parity_gate(dqkv, want, REL, f"stream attention backward L={L} hd={hd} scale={scale}")
        print(f"stream attention backward B={B} L={L} heads={heads} hd={hd} scale={scale}: {rel:.3e}")
        assert torch.equal(dqkv, F.vit_attention_backward_stream(qkv, out, dout, heads, scale)), "two runs differ"
    if L > 256:                                  # the public wrapper routes what the resident kernel cannot take
        assert torch.equal(F.vit_attention_backward(qkv, out, dout, heads, 0.37), dqkv)


# ---- 2. streaming against resident ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [22, 180, 256])
def test_stream_backward_agrees_with_resident(L, hd, dev):
    from stgcn_amd import functional as F
    heads = 8
    qkv, out, dout, want = backward_case(3, L, heads, hd, None, dev)
    res, stream = F.vit_attention_backward(qkv, out, dout, heads), F.vit_attention_backward_stream(qkv, out, dout, heads)
    parity_gate(res, want, REL, f"resident backward L={L} hd={hd} vs fp64")
    parity_gate(stream, want, REL, f"stream backward L={L} hd={hd} vs fp64")
    print(f"L={L} hd={hd}: stream vs resident {parity_gate(stream, res, REL, f'stream vs resident backward L={L} hd={hd}'):.3e}")


# ---- 3. the recomputed statistics, on planted inputs ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rising", "falling", "spike_last", "spike_first"])
def test_stream_backward_on_planted_scores(case, dev):
    """The whole dqkv is gated, not its three parts: |dq| ~ 0.3 comes out of cancellation against |k| ~ 100, and in the spike
    cases the true dq / dk are about 1e-82, so a per-part gate would reject fp32 arithmetic itself."""
    from stgcn_amd import functional as F
    qkv, s, _ = planted_case(case)
    lo, hi = s.min(dim=-1).values, s.max(dim=-1).values
    if case in ("rising", "falling"):            # about -60 .. +60 for every query: exp(range) overflows fp32
        assert (hi - lo).min().item() > 89 and hi.min().item() > 50 and lo.max().item() < -50, (lo.max().item(), hi.min().item())
        first, last = s[..., :64].max(dim=-1).values, s[..., -64:].max(dim=-1).values
        assert ((last - first).min().item() > 89) if case == "rising" else ((first - last).min().item() > 89)
    else:                                        # exp(89) > fp32 max
        assert hi.min().item() > 89 and lo.max().item() < -89, (lo.max().item(), hi.min().item())
        at = s.argmax(dim=-1)
        assert bool((at == (PLANTED_L - 1 if case == "spike_last" else 0)).all())
    dout = torch.randn(PLANTED_B, PLANTED_L, PLANTED_HEADS * PLANTED_HD, generator=torch.Generator().manual_seed(99)).to(dev)
    qd = qkv.to(dev)
    _, want = attention_grad64(qd, dout, PLANTED_HEADS, PLANTED_HD ** -0.5)
    assert torch.isfinite(want).all() and want.abs().max().item() > 0.5, "the fp64 reference itself"
    dqkv = F.vit_attention_backward_stream(qd, F.vit_attention_stream(qd, PLANTED_HEADS), dout, PLANTED_HEADS)
    assert torch.isfinite(dqkv).all()
    print(f"planted {case}: {parity_gate(dqkv, want, REL, f'planted scores backward, {case}'):.3e}")


# ---- 4. the block entry points -------------------------------------------------------------------------------------------
BLOCK_SHAPES = [(3, 300, 512, 8, 1024), (2, 500, 256, 8, 512), (70, 500, 256, 8, 512)]      # the last: 35,000 tokens = two slabs
MODES = sorted(TRAIN_STRICT)


@functools.lru_cache(maxsize=None)
def block_case(shape, dev):
    """State, input, upstream gradient, stochastic-depth factors and the fp64 gradients (computed on the device: the CPU would
    take minutes at 35,000 tokens), shared by the three arithmetic modes."""
    B, L, D, heads, hidden = shape
    sd = ar.random_block_state(D, hidden, True, seed=B + L + D)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    dy = torch.randn(B, L, D, generator=g)
    s1, s2 = tr.make_scales(B, L + 1)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    x, dy, s1, s2 = x.to(dev), dy.to(dev), s1.to(dev), s2.to(dev)
    want_y, want = tr.grads64(x, sdd, dy, heads=heads, s1=s1, s2=s2)
    params = [sdd[k] for k in tr.PARAMS]
    return x, dy, s1, s2, params, want_y.cpu(), {k: v.cpu() for k, v in want.items()}


def run_block(x, dy, params, heads, mode, s1, s2):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    args = (heads, ar.EPS, (x.shape[-1] // heads) ** -0.5, HEAD_MATH[mode], s1, s2)
    y, saved = F.vit_block_forward_train(x, params, *args)
    g = F.vit_block_backward(x, params, saved, dy, *args)
    return y, {"x": g["x"], **{k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS)}}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_entry_points_vs_fp64(shape, mode, dev):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    B, L, D, heads, hidden = shape
    assert F.vit_block_train_long_supported(L, D, heads, hidden) and not F.vit_block_train_supported(L, D, heads, hidden)
    x, dy, s1, s2, params, want_y, want = block_case(shape, dev)
    assert (s1 == 0).any() and (s1 > 1).any() and (s2 == 0).any() and not torch.equal(s1, s2)
    strict = TRAIN_STRICT[mode]
    y, g = run_block(x, dy, params, heads, mode, s1, s2)
    print(f"long block {shape} {mode} y: {parity_gate(y, want_y, REL, f'long block {shape} {mode} y', strict):.3e}")
    for k, v in want.items():
        print(f"long block {shape} {mode} d{k}: {parity_gate(g[k], v, REL, f'long block {shape} {mode} d{k}', strict):.3e}")
    # without masks the training forward is the eval forward, bit for bit
    scale = (D // heads) ** -0.5
    y_eval = F.vit_block_forward(x, params[0:2], params[2:4], params[4:6], params[6:8], params[8:10], params[10:12], heads, ar.EPS,
                                 scale, HEAD_MATH[mode])
    assert torch.equal(F.vit_block_forward_train(x, params, heads, ar.EPS, scale, HEAD_MATH[mode])[0], y_eval)
    y2, g2 = run_block(x, dy, params, heads, mode, s1, s2)
    assert torch.equal(y, y2)
    for k in g:
        assert torch.equal(g[k], g2[k]), f"{mode}: d{k} differs between two runs"
    if B * L > 32768:                            # two slabs (65 + 5 sequences) against the two halves of the batch, one slab each
        h = B // 2
        halves = [run_block(x[a:b].contiguous(), dy[a:b].contiguous(), params, heads, mode, s1[a:b].contiguous(),
                            s2[a:b].contiguous())[1]["x"] for a, b in ((0, h), (h, B))]
        assert torch.equal(g["x"], torch.cat(halves)), "the slab walk changes dx"


# ---- 5. buffer discipline ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [257, 513])
def test_stream_backward_under_poisoned_guard_banded_buffers(L, hd, dev):
    """Inputs, result and workspace between 1 MiB guard bands, everything pre-filled with NaN bytes, then with huge finite
    values: the guards stay intact, every element of dqkv is written and equals the run on plain buffers bit for bit (a read
    past a buffer's end, of a row past L, or of a statistic that nobody wrote, would bring the poison in), the inputs are
    unchanged."""
    from stgcn_amd import functional as F
    B, heads = 3, 8
    qkv, out, dout, want = backward_case(B, L, heads, hd, None, dev)
    plain = F.vit_attention_backward_stream(qkv, out, dout, heads)
    parity_gate(plain, want, REL, f"plain buffers L={L} hd={hd}")
    for fill in (0xFF, 0x7F):
        with hostile_allocations(fill) as h:
            copies = []
            for t in (qkv, out, dout):
                c = torch.empty(t.shape, device=dev, dtype=torch.float32)
                c.copy_(t)
                copies.append(c)
            dqkv = F.vit_attention_backward_stream(*copies, heads)
            torch.cuda.synchronize()
            h.check()
            shapes = [r[2] for r in h.records]
            assert shapes[:4] == [(B, L, 3 * heads * hd), (B, L, heads * hd), (B, L, heads * hd), (B, L, 3 * heads * hd)]
            assert len(shapes) == 5, "the three inputs, dqkv and the workspace are guard-banded"
        assert torch.isfinite(dqkv).all(), f"fill 0x{fill:02X}: an element of dqkv was not written, or poison was read"
        assert torch.equal(dqkv, plain), f"fill 0x{fill:02X}: the result depends on what surrounds the buffers"
        for c, t, n in zip(copies, (qkv, out, dout), ("qkv", "out", "dout")):
            assert torch.equal(c, t), f"{n} was written to"


def test_long_block_backward_under_poisoned_guard_banded_buffers(dev):
    """The same conditions around one block at L = 300: `saved` (written by the training forward) and the backward's workspace,
    whose tail is the streaming attention backward's statistics."""
    shape = (3, 300, 256, 8, 512)
    B, L, D, heads, hidden = shape
    x, dy, s1, s2, params, _, _ = block_case(shape, dev)
    y, plain = run_block(x, dy, params, heads, "f32", s1, s2)
    for fill in (0xFF, 0x7F):
        with hostile_allocations(fill) as h:
            xc = torch.empty(x.shape, device=dev, dtype=torch.float32)
            xc.copy_(x)
            yh, g = run_block(xc, dy, params, heads, "f32", s1, s2)
            torch.cuda.synchronize()
            h.check()
            assert len(h.records) >= 4 + 13, "x, saved, y, the workspace and the thirteen gradients are guard-banded"
        assert torch.equal(yh, y), f"fill 0x{fill:02X}: y depends on what surrounds the buffers"
        for k, v in plain.items():
            assert torch.isfinite(g[k]).all(), f"fill 0x{fill:02X}: d{k} holds poison"
            assert torch.equal(g[k], v), f"fill 0x{fill:02X}: d{k} depends on what the buffers held or on what surrounds them"
        assert torch.equal(xc, x), "x was written to"


# ---- 6. the module -------------------------------------------------------------------------------------------------------
def test_block_module_trains_long_sequences_on_request(dev):
    from stgcn_amd.altformer import Block, set_long_training
    torch.manual_seed(5)
    blk = Block(256, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.1)
    ar.prepare_block(blk, 5)
    blk = blk.to(dev).train()
    blk.hip_train_min_tokens = 0
    x = torch.randn(4, 300, 256, device=dev)
    xg = x.clone().requires_grad_()
    assert not blk.trains_on_hip(xg), "off by default"
    set_long_training(blk)
    assert blk.trains_on_hip(xg) and blk.trains_on_hip(x[:, :256].clone().requires_grad_())
    assert not blk.trains_on_hip(torch.randn(1, 4097, 256, device=dev, requires_grad=True)), "4097 tokens are never covered"
    set_long_training(blk, False)
    assert not blk.trains_on_hip(xg) and blk.trains_on_hip(x[:, :256].clone().requires_grad_())
    set_long_training(blk)
    out, dx, grads = step(blk, x, 31)
    blk.force_torch = True
    assert not blk.trains_on_hip(xg)
    out_t, dx_t, grads_t = step(blk, x, 31)
    print(f"Block (4, 300, 256) training, HIP vs torch path: y {parity_gate(out, out_t, REL, 'long Block y'):.3e}",
          f"dx {parity_gate(dx, dx_t, REL, 'long Block dx'):.3e}")
    compare_grads(grads, grads_t, "long Block")


# ---- 7. the heads at a long clip -----------------------------------------------------------------------------------------
@pytest.fixture
def pinned_max(monkeypatch):
    from stgcn_amd import altformer
    pin = PinnedMax()
    monkeypatch.setattr(altformer, "max_over_tokens", pin)
    return pin


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_head_trains_at_300_frames(cls_name, dev, pinned_max):
    from stgcn_amd import altformer
    from stgcn_amd.altformer import Block, set_hip_min_tokens, set_long_training
    torch.manual_seed(11)
    head = getattr(altformer, cls_name)(14, num_frame=300, num_joints=22, in_chans=128, embed_dim_ratio=256, depth=2, num_heads=8,
                                        mlp_ratio=2., qkv_bias=True, drop_path_rate=0.1)
    with torch.no_grad():
        for n, p in head.named_parameters():
            if n.endswith("pos_embed"):
                p.copy_(0.05 * torch.randn(p.shape))
    set_hip_min_tokens(head, 0)
    set_long_training(head)
    head = head.to(dev).train()
    z = torch.randn(2, 128, 300, 22, device=dev)
    labels = torch.tensor([3, 11], device=dev)
    ce = nn.CrossEntropyLoss()
    blocks = [m for m in head.modules() if isinstance(m, Block)]
    calls = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: calls.append((args[0].shape[1], mod.trains_on_hip(args[0])))) for m in blocks]
    out, dz, grads = step(head, z, 77, lambda o: ce(o, labels))
    for hk in hooks:
        hk.remove()
    assert len(calls) == 4 and all(on for _, on in calls), calls
    assert sorted(L for L, _ in calls) == [22, 22, 300, 300]
    set_force_torch(head, True)
    pinned_max.second_run()
    out_t, dz_t, grads_t = step(head, z, 77, lambda o: ce(o, labels))
    what = f"{cls_name} training at 300 frames"
    print(f"{what} logits: {parity_gate(out, out_t, REL, what + ' logits'):.3e}")
    print(f"{what} dz: {parity_gate(dz, dz_t, REL, what + ' dz'):.3e}")
    compare_grads(grads, grads_t, what)
