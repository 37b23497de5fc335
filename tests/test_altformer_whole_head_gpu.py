"""GPU tests of the whole AltFormer head in one call: the pooling kernel (``stgcn_vit_pool``) and the pooled classifier
(``stgcn_vit_pool_classify``) against fp64 torch on the CPU, and ``set_whole_head`` against the per-block path of the same
module (the blocks and the first embedding are the same kernels on the same inputs, so only the glue differs), against the
reference's logits (tests/golden/model_altformer_shre.npz), under graph capture, in every arithmetic mode, in replicas, and on
the calls that must keep today's path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF
from torch.nn.parallel import parallel_apply

from _util import MATH_GATES, parity_gate
from test_altformer_gpu import small_head, whole_model

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
assert MATH_GATES["f32"] == (REL, True)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


# ---- the pooling kernel ---------------------------------------------------------------------------------------------------
# one token; the heads' joints and frames; L above one pass of the token lanes; one
# clip of TS (the narrow form, 88 workgroups); enough sequences for the wide form (1024 workgroups and more), with a last chunk
# of D that is not full in the wide and in the narrow form
POOL_SHAPES = [(7, 1, 64), (7, 22, 256), (3, 46, 512), (5, 180, 256), (2, 257, 64), (22, 180, 256), (1030, 22, 256), (600, 5, 328), (3, 5, 100)]
_pool_inputs = {}


def pool_input(shape):
    """Drawn entirely below zero (a zero-initialised accumulator would win every maximum); shared, never written."""
    if shape not in _pool_inputs:
        g = torch.Generator().manual_seed(sum(shape))
        S, L, D = shape
        _pool_inputs[shape] = -(0.5 + torch.rand(S, L, D, generator=g) * (1 + 3 * torch.rand(S, 1, D, generator=g)))
    return _pool_inputs[shape]


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_max_is_the_selection_bit_for_bit(shape, dev):
    from stgcn_amd import functional as F
    x = pool_input(shape)
    assert x.max().item() < 0
    out = F.vit_pool(x.to(dev), "max")
    assert out.shape == (shape[0], shape[2]) and torch.equal(out.cpu(), x.max(dim=1).values)
    # the maximum planted at the first and at the last token (alternating over the columns), far above everything else
    S, L, D = shape
    y = x.clone()
    y[:, 0, 0::2] = 3.0 + torch.arange(S, dtype=torch.float32)[:, None]
    y[:, L - 1, 1::2] = 5.0 + torch.arange(S, dtype=torch.float32)[:, None]
    out = F.vit_pool(y.to(dev), "max").cpu()
    assert torch.equal(out, y.max(dim=1).values)
    assert torch.equal(out[:, 1::2], y[:, L - 1, 1::2]) and (L > 1 or torch.equal(out[:, 0::2], y[:, 0, 0::2]))


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_mean_vs_fp64(shape, dev):
    from stgcn_amd import functional as F
    x = pool_input(shape)
    out = F.vit_pool(x.to(dev), "mean")
    rel = parity_gate(out, x.double().mean(dim=1), REL, f"pool mean {shape}")
    print(f"pool mean {shape}: {rel:.3e}")
    assert torch.equal(out, F.vit_pool(x.to(dev), "mean"))


# ---- the pooled classifier -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("classes", [1, 14, 28])
@pytest.mark.parametrize("LD", [(1, 64), (22, 512), (180, 512), (257, 128), (3, 4096), (7, 192)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("N", [1, 5])
def test_pool_classify_vs_fp64(N, LD, classes, mode, dev):
    from stgcn_amd import functional as F
    L, D = LD
    g = torch.Generator().manual_seed(1000 * N + L + D + classes)
    x = torch.randn(N, L, D, generator=g) * (0.25 + 3.75 * torch.rand(N, 1, D, generator=g)) + torch.randn(N, 1, 1, generator=g)
    lw, lb = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W = (torch.rand(classes, D, generator=g) * 2 - 1) / D ** 0.5
    b = torch.randn(classes, generator=g) * 0.5
    eps = 1e-5
    x64 = x.double()
    pooled = x64.max(dim=1).values if mode == "max" else x64.mean(dim=1)
    want = TF.layer_norm(pooled, (D,), lw.double(), lb.double(), eps) @ W.double().T + b.double()
    xd, lwd, lbd, Wd, bd = (t.to(dev) for t in (x, lw, lb, W, b))
    out = F.vit_pool_classify(xd, lwd, lbd, eps, Wd, bd, mode=mode)
    rel = parity_gate(out, want, REL, f"pool_classify N={N} L={L} D={D} classes={classes} {mode}")
    print(f"pool_classify N={N} L={L} D={D} classes={classes} {mode}: {rel:.3e}")
    assert torch.equal(out, F.vit_pool_classify(xd, lwd, lbd, eps, Wd, bd, mode=mode))
    nb = F.vit_pool_classify(xd, lwd, lbd, eps, Wd, None, mode=mode)
    parity_gate(nb, want - b.double(), REL, "pool_classify without a bias")


# ---- the whole head against the per-block path ------------------------------------------------------------------------------
def stem_output(N, T, V, dev, layout="contiguous", seed=5):
    g = torch.Generator().manual_seed(seed)
    z = torch.relu(torch.randn(N, 128, T, V, generator=g)).to(dev)        # the stem ends in a ReLU
    return z.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else z


def both_paths(head, z):
    """(whole-head logits, per-block logits of the same module), the one-call path confirmed by ``runs_whole`` and by the
    blocks' forward never being entered."""
    import stgcn_amd
    from stgcn_amd.altformer import Block
    entered = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: entered.append(1)) for m in head.modules() if isinstance(m, Block)]
    with torch.no_grad():
        stgcn_amd.set_whole_head(head, False)
        assert not head.runs_whole(z)
        want = head(z)
        per_block = len(entered)
        stgcn_amd.set_whole_head(head)
        assert head.runs_whole(z)
        got = head(z)
        assert len(entered) == per_block > 0, "the whole-head forward entered a Block"
        again = head(z)
    for h in hooks:
        h.remove()
    assert got.shape == want.shape and torch.equal(got, again), "two whole-head runs differ"
    return got, want


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_small_head_matches_the_per_block_path(cls_name, layout, dev):
    head = small_head(dev, cls_name)
    got, want = both_paths(head, stem_output(3, 40, 22, dev, layout))
    print(f"{cls_name} {layout}: whole head vs per-block {parity_gate(got, want, REL, f'{cls_name} {layout} whole head'):.3e}")


def test_more_than_one_slab(dev):
    head = small_head(dev, "ST", num_frame=180, depth=1)
    got, want = both_paths(head, stem_output(10, 180, 22, dev))           # 39,600 tokens: two slabs in stage 1
    print(f"two slabs: {parity_gate(got, want, REL, 'ST 10 x 180 x 22 whole head'):.3e}")


def test_streaming_length(dev):
    from stgcn_amd import functional as F
    head = small_head(dev, "TS", num_frame=300, depth=1)
    assert F.vit_block_attention_form(44, 300, 256, 8, 512) == "stream"
    got, want = both_paths(head, stem_output(2, 300, 22, dev))
    print(f"streaming: {parity_gate(got, want, REL, 'TS 2 x 300 x 22 whole head'):.3e}")


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("style", ["ST", "TS", None])
def test_fixture_logits_and_argmax(style, layout, dev):
    import stgcn_amd
    from stgcn_amd.altformer import Block, _Head
    model, g = whole_model(style, dev, "default", layout, "hip")
    stgcn_amd.set_whole_head(model)
    entered, whole = [], []
    hooks = [m.register_forward_pre_hook(lambda mod, args: entered.append(1)) for m in model.modules() if isinstance(m, Block)]
    hooks += [m.register_forward_pre_hook(lambda mod, args: whole.append(mod.runs_whole(args[0])))
              for m in model.modules() if isinstance(m, _Head)]
    with torch.no_grad():
        logits = model(torch.from_numpy(g["skeleton"]).to(dev)).cpu()
    for h in hooks:
        h.remove()
    used = [m for n, m in (("ST", model.modelA), ("TS", model.modelB)) if style in (n, None)]
    assert whole == [True] * len(used) and not entered, "the one-call path was not taken"
    if style is None:
        want = g["logits_ST"].astype(np.float64) + g["logits_TS"].astype(np.float64)
    else:
        want = g[f"logits_{style}"]
    rel = parity_gate(logits, want, REL, f"whole model, whole head {style} {layout}")
    print(f"whole model, whole head style={style} {layout}: max|err|/max|logit| = {rel:.3e}")
    if style is not None:
        assert np.array_equal(logits.argmax(1).numpy(), g[f"argmax_{style}"])
    else:
        assert np.array_equal(logits.argmax(1).numpy(), want.argmax(1))


# ---- modes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "mixed", "bf16x3", "bf16"])
def test_modes(mode, dev):
    from stgcn_amd.altformer import set_head_math
    head = small_head(dev, "ST")
    set_head_math(head, mode)
    got, want = both_paths(head, stem_output(3, 40, 22, dev))
    rel, strict = MATH_GATES["bf16"] if mode == "bf16" else (REL, True)
    print(f"{mode}: whole head vs per-block {parity_gate(got, want, rel, f'whole head {mode}', strict=strict):.3e}")


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_low_latency_with_split_attention_at_one_clip(cls_name, dev):
    """The glue is NOT bit-compatible with the per-block path's torch ops (the second embedding is the library's fp32 GEMM, not
    torch's; the mean is summed in another order), so the result is held to the fp32 gate, not to equality."""
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import set_low_latency
    head = small_head(dev, cls_name)
    set_low_latency(head, min_tokens=0, split_attention=True)
    assert F.vit_block_attention_form(22 if cls_name == "TS" else 1, 40, 512 if cls_name == "ST" else 256, 8,
                                      1024 if cls_name == "ST" else 512, head.blocks[0]._hip_flags(torch.zeros(1, 40, 1), False)) \
        == "resident_split"
    got, want = both_paths(head, stem_output(1, 40, 22, dev))
    print(f"{cls_name} low latency + split: {parity_gate(got, want, REL, f'{cls_name} one clip, split attention'):.3e}")


def test_blocks_that_disagree_take_the_per_block_path(dev):
    import stgcn_amd
    from stgcn_amd.altformer import HEAD_MATH
    head = small_head(dev, "ST")
    z = stem_output(2, 40, 22, dev)
    with torch.no_grad():
        want = head(z)
        stgcn_amd.set_whole_head(head)
        head.Spatial_blocks[1].math_mode = HEAD_MATH["f32"]
        assert not head.runs_whole(z)
        head.Spatial_blocks[0].math_mode = HEAD_MATH["f32"]
        assert head.runs_whole(z)
        head.Spatial_blocks[0].math_mode = head.Spatial_blocks[1].math_mode = None
        head.blocks[1].small_tiles = True
        assert not head.runs_whole(z) and torch.equal(head(z), want)


# ---- capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_one_clip_captures_under_a_graph(cls_name, dev):
    import stgcn_amd
    head = small_head(dev, cls_name)
    stgcn_amd.set_low_latency(head, min_tokens=0)
    stgcn_amd.set_whole_head(head)
    z = stem_output(1, 40, 22, dev)
    with torch.no_grad():
        assert head.runs_whole(z)
        eager = head(z)
        torch.cuda.synchronize()
        static = z.clone()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            head(static)                                  # warm-up on the side stream, as torch's recipe has it
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            out = head(static)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        other = stem_output(1, 40, 22, dev, seed=6)
        static.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, head(other)) and not torch.equal(out, eager)


# ---- fallbacks ------------------------------------------------------------------------------------------------------------------
def test_fallbacks_give_todays_result(dev):
    import stgcn_amd
    head = small_head(dev, "ST")
    z = stem_output(2, 40, 22, dev)
    cpu_head = small_head(torch.device("cpu"), "ST")
    with torch.no_grad():
        cpu_want = cpu_head(z.cpu())
        head.blocks[0].force_torch = True
        forced_want = head(z)
        head.blocks[0].force_torch = False
    zg = z.clone().requires_grad_()
    grad_want = head(zg)
    stgcn_amd.set_whole_head(head)
    stgcn_amd.set_whole_head(cpu_head)
    with torch.no_grad():
        assert head.runs_whole(z)
        assert not cpu_head.runs_whole(z.cpu()) and torch.equal(cpu_head(z.cpu()), cpu_want)
        head.blocks[0].force_torch = True
        assert not head.runs_whole(z) and torch.equal(head(z), forced_want)
        head.blocks[0].force_torch = False
        assert head.runs_whole(z) and not head.runs_whole(z.double()) and not head.runs_whole(z[:, :, ::2])
    # under autograd (the parameters require gradients, and so does the input): today's path, every gradient
    assert not head.runs_whole(zg) and not head.runs_whole(z)
    out = head(zg)
    assert torch.equal(out, grad_want)
    out.sum().backward()
    unused = ("Spatial_cls_token", "cls_token", "Spatial_norm.", "Temporal_norm.", "weighted_mean.", "fcn.")
    for k, p in head.named_parameters():
        assert (p.grad is not None) != k.startswith(unused), k
    assert zg.grad is not None and zg.grad.abs().sum().item() > 0
    head.train()                                          # stochastic depth draws: today's path, no error
    with torch.no_grad():
        assert not head.runs_whole(z) and head(z).shape == (2, 14)


# ---- replicas ------------------------------------------------------------------------------------------------------------------
def test_replicas_give_the_masters_result(dev):
    import stgcn_amd
    from test_data_parallel import _replicas
    head = small_head(dev, "ST")
    stgcn_amd.set_whole_head(head)
    z = stem_output(8, 40, 22, dev)
    halves = [(z[:4],), (z[4:],)]
    with torch.no_grad():
        assert head.runs_whole(z[:4])
        want = [head(h) for (h,) in halves]
        for _ in range(2):
            replicas = _replicas(head, 2)
            assert all(r.whole_head and r.runs_whole(z[:4]) for r in replicas)
            got = parallel_apply(replicas, halves, devices=[dev, dev])
            for o, w in zip(got, want):
                assert torch.equal(o, w)
        dp = torch.nn.DataParallel(head, device_ids=[dev.index or 0])
        assert torch.equal(dp(z), head(z))
