"""The ST-ViT head on the GPU: the patch embedding (``stgcn_vit_patch_embed``) against the fp64 restatement in both layouts and
both arithmetics, the class-token pooling, and the whole ``ViT`` of the reference configuration through the HIP path against
the reference fixture and tests/stvit_ref.py - gates, determinism, poisoned buffers, non-finite input, the low-latency forms
and a captured graph.  (The capture is the last test of the file: the allocation patch of the buffer test is process-wide.)"""
import pytest
import torch
import torch.nn.functional as TF

import stvit_ref as sr
from _util import MATH_GATES, hostile_allocations, load_golden, parity_gate

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
HEAD_GATES = {"f32": 1e-4, "mixed": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}     # of max|logit|


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return load_golden("stvit_reference")


@pytest.fixture(scope="module")
def embed_refs():
    """Per embedding case: the seeded tensors and the fp64 results with and without bias / position table, computed once."""
    out = {}
    for name, (N, C, T, V, p1, p2, E) in sr.EMBED_CASES.items():
        z, W, bias, cls, pos = sr.embed_case(name)
        out[name] = dict(z=z, W=W, bias=bias, cls=cls, pos=pos, full=sr.embed64(z, W, bias, cls, pos, p1, p2),
                         plain=sr.embed64(z, W, None, cls, None, p1, p2))
    return out


@pytest.fixture(scope="module")
def whole(dev):
    """The reference configuration, seeded and prepared as the fixture's module was, on the GPU with the HIP path forced, the
    input, and the fp64 logits of tests/stvit_ref.py for both poolings - computed once and left unchanged."""
    import stgcn_amd
    from stgcn_amd.vit import ViT
    torch.manual_seed(sr.MODEL_SEED)
    model = sr.prepare(ViT(**sr.CONFIG).eval())
    z = sr.make_input()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref = {pool: sr.vit64(z, sd, sr.CONFIG["p1"], sr.CONFIG["p2"], sr.CONFIG["depth"], sr.CONFIG["heads"], pool)[0] for pool in ("cls", "mean")}
    model = model.to(dev)
    stgcn_amd.set_hip_min_tokens(model, 0)
    return model, z.to(dev), ref


def _layout(z, layout, dev):
    zd = z.to(dev)
    return zd if layout == "nchw" else zd.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("layout", ["nchw", "ntvc"])
@pytest.mark.parametrize("name", sorted(sr.EMBED_CASES))
def test_patch_embed(name, layout, math, embed_refs, dev):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    N, C, T, V, p1, p2, E = sr.EMBED_CASES[name]
    r = embed_refs[name]
    n, w = (T // p1) * (V // p2), V // p2
    z = _layout(r["z"], layout, dev)
    assert F._is_channels_last(z) == (layout == "ntvc")
    W, bias, cls, pos = (r[k].to(dev) for k in ("W", "bias", "cls", "pos"))
    x = F.vit_patch_embed(z, W, bias, cls, pos, p1, p2, HEAD_MATH[math])
    assert x.shape == (N, n + 1, E)
    print(f"{name} {layout} {math}: cut {F.vit_patch_embed_cut(N, C, T, V, p1, p2, E, HEAD_MATH[math], layout == 'ntvc')}, "
          f"err {(x.double().cpu() - r['full']).abs().max().item() / r['full'].abs().max().item():.3e}")
    parity_gate(x, r["full"], REL, f"{name} {layout} {math}")
    # the class row is cls + pos[0] exactly, in every clip
    assert torch.equal(x[:, 0], (cls + pos[0]).expand(N, E))
    # rows are placed at 1 + a w + b: each patch row against its own patch, computed apart from the others
    a, b = (T // p1) - 1, w - 1
    patch = r["z"][:, :, a * p1:(a + 1) * p1, b * p2:(b + 1) * p2].double().permute(0, 2, 3, 1).reshape(N, -1)
    want = patch @ r["W"].double().T + r["bias"].double() + r["pos"][1 + a * w + b].double()
    parity_gate(x[:, 1 + a * w + b], want, REL, f"{name}: row of patch ({a}, {b})")
    # without bias and position table: the plain product, the class row the class token
    y = F.vit_patch_embed(z, W, None, cls, None, p1, p2, HEAD_MATH[math])
    parity_gate(y[:, 1:], r["plain"][:, 1:], REL, f"{name} {layout} {math} plain")
    assert torch.equal(y[:, 0], cls.expand(N, E))
    # bit-identical from run to run
    assert torch.equal(x, F.vit_patch_embed(z, W, bias, cls, pos, p1, p2, HEAD_MATH[math]))


@pytest.mark.parametrize("NLD", [(2, 100, 512), (5, 7, 192), (1, 1, 64)], ids=lambda s: "x".join(map(str, s)))
def test_pool_cls(NLD, dev):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    N, L, D = NLD
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, L, D, generator=g).to(dev)
    ln_w, ln_b = (1 + 0.2 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
    Wc, bc = (torch.randn(9, D, generator=g) / D ** 0.5).to(dev), torch.randn(9, generator=g).to(dev)
    assert torch.equal(F.vit_pool(x, "cls"), x[:, 0])
    want = TF.linear(TF.layer_norm(x[:, 0].double(), (D,), ln_w.double(), ln_b.double(), 1e-5), Wc.double(), bc.double())
    parity_gate(F.vit_pool_classify(x, ln_w, ln_b, 1e-5, Wc, bc, mode="cls"), want, REL, f"pool_classify cls {NLD}")
    # with the bit clear nothing moved: the maximum is still the selection, the mean still sum / L in the kernel's order
    assert torch.equal(F.vit_pool(x, "max"), x.max(dim=1).values)
    parity_gate(F.vit_pool(x, "mean"), x.double().mean(dim=1), REL, f"pool mean {NLD}")
    for mode in ("mean", "max"):
        a = F.vit_pool_classify(x, ln_w, ln_b, 1e-5, Wc, bc, mode=mode)
        pooled = x.double().mean(dim=1) if mode == "mean" else x.double().max(dim=1).values
        parity_gate(a, TF.linear(TF.layer_norm(pooled, (D,), ln_w.double(), ln_b.double(), 1e-5), Wc.double(), bc.double()), REL, mode)
        assert torch.equal(a, F.vit_pool_classify(x, ln_w, ln_b, 1e-5, Wc, bc, mode=mode))
    with pytest.raises(_capi.StgcnError) as e:
        _capi.call("stgcn_vit_pool", F._dev_ptr(x, "x"), F._dev_ptr(torch.empty(N, D, device=dev), "out"), N, L, D,
                   _capi.VIT_POOL_CLS | _capi.VIT_POOL_MAX, F._stream(dev))
    assert e.value.code == -1


@pytest.mark.parametrize("pool", ["cls", "mean"])
@pytest.mark.parametrize("math", sorted(HEAD_GATES))
def test_whole_vit(math, pool, whole, golden, dev):
    import stgcn_amd
    model, z, ref = whole
    stgcn_amd.set_head_math(model, math)
    model.pool = pool
    try:
        with torch.no_grad():
            assert model.uses_hip(z) and all(layer.uses_hip(torch.empty(2, 100, 512, device=dev)) for layer in model.transformer.layers)
            out = model(z)
            again = model(z)
            last = model(z.contiguous(memory_format=torch.channels_last))
    finally:
        stgcn_amd.set_head_math(model, None)
        model.pool = "cls"
    gate = HEAD_GATES[math]
    for what, want in (("stvit_ref", ref[pool]), ("fixture", torch.from_numpy(golden[f"logits_{pool}_f64"]))):
        err = (out.double().cpu() - want).abs().max().item() / want.abs().max().item()
        print(f"whole ViT {math} pool={pool} against {what}: {err:.3e} (gate {gate:g})")
        parity_gate(out, want, gate, f"whole ViT {math} {pool} vs {what}", strict=False)
    assert torch.equal(out, again), "two runs differ"
    assert torch.equal(out, last), "the channels-last input, read in place, gives another result"


def test_uncovered_layers_take_the_torch_path(whole, dev):
    """head_dim 48 has no attention kernel: the layers run on torch ops between the HIP embedding and the HIP classifier; and
    one layer of the reference configuration forced onto torch ops leaves the others on HIP.  Both still match."""
    import stgcn_amd
    from stgcn_amd.vit import ViT
    cfg = dict(time_len=8, joint=6, p1=4, p2=2, num_classes=5, dim=192, depth=2, heads=4, mlp_dim=192, channels=32, dim_head=48)
    torch.manual_seed(77)
    small = sr.prepare(ViT(**cfg).eval(), seed=78)
    zs = sr.make_input(3, 32, 8, 6, seed=79)
    sd = {k: v.detach().clone() for k, v in small.state_dict().items()}
    want = sr.vit64(zs, sd, 4, 2, 2, 4, "cls", dim_head=48)[0]
    small = small.to(dev)
    stgcn_amd.set_hip_min_tokens(small, 0)
    zd = zs.to(dev)
    with torch.no_grad():
        assert small.embed_on_hip(zd) and small.head_on_hip(torch.empty(3, 7, 192, device=dev)) and not small.uses_hip(zd)
        assert not any(l.uses_hip(torch.empty(3, 7, 192, device=dev)) for l in small.transformer.layers)
        parity_gate(small(zd), want, REL, "head_dim 48", strict=False)
    model, z, ref = whole
    model.transformer.layers[2].force_torch = True
    try:
        with torch.no_grad():
            assert not model.uses_hip(z) and model.transformer.layers[1].uses_hip(torch.empty(2, 100, 512, device=dev))
            parity_gate(model(z), ref["cls"], REL, "one layer on torch ops", strict=False)
    finally:
        model.transformer.layers[2].force_torch = False


def test_hostile_buffers(whole):
    model, z, ref = whole
    with torch.no_grad():
        clean = model(z)
        for fill in (0xFF, 0x7F):
            with hostile_allocations(fill) as h:
                a = model(z)
                torch.cuda.synchronize()
                h.check()
            assert h.records, "no allocation went through torch.empty - the case would test nothing"
            assert torch.equal(a, clean), f"fill=0x{fill:02X}: the result depends on what a buffer held before"


def test_nan_stays_in_its_clip(whole):
    model, z, ref = whole
    bad = z.clone()
    bad[1, 5, 100, 7] = float("nan")
    with torch.no_grad():
        clean, out = model(z), model(bad)
    assert not torch.isfinite(out[1]).any(), "the clip with the NaN has finite logits"
    assert torch.equal(out[0], clean[0]), "the NaN of one clip moved another clip's logits"


def test_low_latency_one_clip_and_captured_graph(whole, dev):
    import stgcn_amd
    from stgcn_amd import _capi
    model, z, ref = whole
    one = z[:1].contiguous()
    subs = [model] + list(model.transformer.layers)
    with torch.no_grad():
        for s in subs:
            s.small_tiles = False
        probe = torch.empty(1, 100, 512, device=dev)
        assert not any(l._hip_flags(probe) & _capi.VIT_TILE_MASK for l in model.transformer.layers)
        big = model(one)                                   # 128 x 128 tiles, threshold 0
        stgcn_amd.set_low_latency(model, min_tokens=0)
        try:
            assert model.uses_hip(one)
            assert all(l.uses_hip(probe) and l._hip_flags(probe) & _capi.VIT_TILE_AUTO for l in model.transformer.layers)
            eager = model(one)
            assert torch.equal(eager, big), "the small tile forms moved a bit of the logits"
            parity_gate(eager, ref["cls"][:1], REL, "one clip", strict=False)
            static_in = one.clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = model(static_in)
            static_in.copy_(z[1:2])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, model(z[1:2].contiguous())), "replay differs from the eager result"
        finally:
            stgcn_amd.set_low_latency(model, enabled=False)
            stgcn_amd.set_hip_min_tokens(model, 0)
