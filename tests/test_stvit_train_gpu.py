"""GPU tests of training the ST-ViT layers on HIP (``stgcn_vit_block_forward_train_drop`` / ``stgcn_vit_block_backward_drop``):
one layer with its three dropout masks against the fp64 restatement (tests/stvit_train_ref.py), bit-equality with the older
pair and across the tile forms, the masks' offsets across slabs of sequences, the modules against their torch-op path under
one seed, non-finite input and poisoned, guard-banded buffers.

Gates: the training tests' own (test_altformer_train_gpu.py): ``parity_gate`` at ``REL`` with ``TRAIN_STRICT`` per arithmetic,
1e-2 of max|.| per tensor for the 'bf16' training arithmetic, ``MODEL_STRICT`` for whole modules."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import altformer_train_ref as tr
import stvit_ref as sr
import stvit_train_ref as vr
from _util import MATH_GATES, parity_gate
from test_altformer_train_gpu import MODEL_STRICT, TRAIN_STRICT, compare_grads, named_grads
from _util import HostileCase as Case, run_under_both_fills

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
BF16_REL = 1e-2          # the 'bf16' training arithmetic: 1e-2 of max|.| per tensor, the max-norm criterion
EPS = sr.LN_EPS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


class Ref:
    """A case on the device and its fp64 gradients (the restatement differentiated on the device), made once per module run
    and never changed: without and with stochastic-depth factors."""

    def __init__(self, name, dev):
        self.B, self.L, self.D, self.heads, self.hidden = vr.CASES[name]
        x, dy, sd, masks = vr.make_case(name)
        self.x, self.dy = x.to(dev), dy.to(dev)
        self.sd = {k: v.to(dev) for k, v in sd.items()}
        self.masks = tuple(m.to(dev) for m in masks)
        self.scale = (self.D // self.heads) ** -0.5
        self.s1, self.s2 = (s.to(dev) for s in tr.make_scales(self.B, 77, keep=0.75))
        self.want = {}

    def params(self):
        return [self.sd.get(k) for k in tr.PARAMS]          # attn.qkv.bias: None

    def fp64(self, scales):
        if scales not in self.want:
            s1, s2 = (self.s1, self.s2) if scales else (None, None)
            y, g = vr.grads64(self.x, self.sd, self.dy, self.masks, s1, s2, self.heads, self.scale, EPS)
            self.want[scales] = (y.cpu(), {k: v.cpu() for k, v in g.items()})
        return self.want[scales]


_REFS = {}


def ref_of(name, dev):
    if name not in _REFS:
        _REFS[name] = Ref(name, dev)
    return _REFS[name]


def run_layer(r, math, masks="own", scales=False, x=None, dy=None, rows=None):
    """forward_train + backward of a case.  ``masks``: 'own' | None (the older pair) | a 3-tuple; ``rows``: a slice of sequences."""
    from stgcn_amd import functional as F
    if masks == "own":
        masks = r.masks
    x, dy = r.x if x is None else x, r.dy if dy is None else dy
    s1, s2 = (r.s1, r.s2) if scales else (None, None)
    if rows is not None:
        x, dy = x[rows].contiguous(), dy[rows].contiguous()
        masks = None if masks is None else tuple(None if m is None else m[rows].contiguous() for m in masks)
        s1, s2 = (None if s is None else s[rows].contiguous() for s in (s1, s2))
    args = (r.heads, EPS, r.scale, math, s1, s2)
    y, saved = F.vit_block_forward_train(x, r.params(), *args, drop=masks)
    g = F.vit_block_backward(x, r.params(), saved, dy, *args, drop=masks)
    return y, {"x": g["x"], **{k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS) if g[n] is not None}}


def gate_all(y, g, want, rel, strict, what):
    want_y, want_g = want
    assert set(g) == set(want_g) and len(g) == 12, "dx and all eleven parameter gradients"
    print(f"{what} y: {parity_gate(y, want_y, rel, what + ' y', strict):.3e}")
    for k, v in want_g.items():
        print(f"{what} d{k}: {parity_gate(g[k], v, rel, f'{what} d{k}', strict):.3e}")


# ---- 1. parity against fp64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(TRAIN_STRICT))
@pytest.mark.parametrize("name", ["vit", "odd"])
def test_layer_with_masks_vs_fp64(name, mode, dev):
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of(name, dev)
    assert all(not m[0].any() for m in r.masks) and all((m == 2.0).any() and (m[-1] == 0).any() for m in r.masks)
    y, g = run_layer(r, HEAD_TRAIN_MATH[mode])
    gate_all(y, g, r.fp64(False), REL, TRAIN_STRICT[mode], f"{name} {mode}")
    assert torch.equal(g["x"][0], r.dy[0]), "the sequence with all three masks zero: dx == dy exactly"
    assert torch.equal(y[0], r.x[0]), "and y == x"


@pytest.mark.parametrize("attn", [False, True], ids=["f32_attention", "bf16_attention"])
@pytest.mark.parametrize("name", ["vit", "odd"])
def test_layer_with_masks_vs_fp64_in_bf16_training_math(name, attn, dev):
    from stgcn_amd._capi import VIT_TRAIN_ATTN_BF16
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of(name, dev)
    y, g = run_layer(r, HEAD_TRAIN_MATH["bf16"] | (VIT_TRAIN_ATTN_BF16 if attn else 0))
    gate_all(y, g, r.fp64(False), BF16_REL, False, f"{name} bf16 attn_bf16={attn}")
    assert torch.equal(g["x"][0], r.dy[0])


@pytest.mark.parametrize("name", ["vit", "odd"])
def test_layer_with_masks_and_stochastic_depth_vs_fp64(name, dev):
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of(name, dev)
    assert (r.s1 == 0).any() and (r.s1 > 1).any() and (r.s2 == 0).any() and not torch.equal(r.s1, r.s2)
    y, g = run_layer(r, HEAD_TRAIN_MATH["f32"], scales=True)
    gate_all(y, g, r.fp64(True), REL, True, f"{name} f32 masks and stochastic depth")


# ---- 2. bit-equality with the older entry points and across the tile forms ---------------------------------------------------------
def assert_same(a, b, what):
    (ya, ga), (yb, gb) = a, b
    assert torch.equal(ya, yb), f"{what}: y differs"
    assert set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), f"{what}: d{k} differs"


@pytest.mark.parametrize("mode", ["f32", "mixed", "bf16"])
@pytest.mark.parametrize("name", ["vit", "odd"])
def test_no_masks_and_masks_of_ones_are_the_older_pair_bit_for_bit(name, mode, dev):
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of(name, dev)
    math = HEAD_TRAIN_MATH[mode]
    for scales in (False, True):
        old = run_layer(r, math, masks=None, scales=scales)
        assert_same(run_layer(r, math, masks=(None, None, None), scales=scales), old, f"{name} {mode} NULL masks")
        ones = tuple(torch.ones_like(m) for m in r.masks)
        assert_same(run_layer(r, math, masks=ones, scales=scales), old, f"{name} {mode} masks of 1.0")
        assert_same(run_layer(r, math, masks=(ones[0], None, ones[2]), scales=scales), old, f"{name} {mode} two masks of 1.0")


@pytest.mark.parametrize("mode", ["f32", "mixed", "bf16"])
@pytest.mark.parametrize("name", ["vit", "odd"])
def test_tile_forms_are_bit_equal(name, mode, dev):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of(name, dev)
    math = HEAD_TRAIN_MATH[mode]
    base = run_layer(r, math, scales=True)
    for tile in ("VIT_TILE_AUTO", "VIT_TILE_64", "VIT_TILE_32"):
        assert_same(run_layer(r, math | getattr(_capi, tile), scales=True), base, f"{name} {mode} {tile}")
    with pytest.raises(_capi.StgcnError) as e:
        F.vit_block_forward_train(r.x, r.params(), r.heads, EPS, r.scale, math | _capi.VIT_TILE_64)
    assert e.value.code == -1, "the older pair still refuses a tile field"


# ---- 3. slab offsets ------------------------------------------------------------------------------------------------------------------
def test_masks_follow_the_slabs_of_sequences(dev):
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of("slabs", dev)
    per = vr.K_SLAB_ROWS // r.L
    assert r.B == per + 3 and r.B * r.L > vr.K_SLAB_ROWS, "two slabs of sequences, the second of 3"
    # give the short second slab masks of its own kind: its first sequence all zero, its second all one, its third drawn
    masks = tuple(m.clone() for m in r.masks)
    for m in masks:
        m[per], m[per + 1] = 0.0, 1.0
    math = HEAD_TRAIN_MATH["f32"]
    y, g = run_layer(r, math, masks=masks, scales=True)
    y2, g2 = run_layer(r, math, masks=masks, scales=True)
    assert_same((y, g), (y2, g2), "two runs of the single call")
    ya, ga = run_layer(r, math, masks=masks, scales=True, rows=slice(0, per))
    yb, gb = run_layer(r, math, masks=masks, scales=True, rows=slice(per, r.B))
    assert torch.equal(y, torch.cat((ya, yb))), "y of the single call is the two slabs' calls, bit for bit"
    assert torch.equal(g["x"], torch.cat((ga["x"], gb["x"]))), "dx too"
    assert torch.equal(g["x"][per], r.dy[per]) and torch.equal(y[per], r.x[per]), "the second slab's all-zero sequence"
    for k in ga:
        if k != "x":
            print(f"slabs d{k}: {parity_gate(g[k], ga[k].double() + gb[k].double(), REL, f'slabs d{k}'):.3e}")
    # masks read at the first slab's rows for the second slab would give another result
    wrong = tuple(torch.cat((m[:per], m[:3])) for m in masks)
    yw, _ = run_layer(r, math, masks=wrong, scales=True)
    assert not torch.equal(yw[per:], y[per:])


# ---- 4. modules -----------------------------------------------------------------------------------------------------------------------
def small_vit(dev, depth=2, dropout=0.1):
    from stgcn_amd import set_hip_min_tokens
    from stgcn_amd.vit import ViT
    torch.manual_seed(sr.MODEL_SEED)
    model = sr.prepare(ViT(**dict(sr.CONFIG, depth=depth), dropout=dropout, emb_dropout=0.0)).to(dev)
    set_hip_min_tokens(model, 0)
    return model


def set_force_torch(module, flag):
    from stgcn_amd.altformer import HipSwitches
    for m in module.modules():
        if isinstance(m, HipSwitches):
            m.force_torch = flag


def step(module, inp, seed, loss, need_dz=True):
    for p in module.parameters():
        p.grad = None
    z = inp.detach().clone().requires_grad_(need_dz)
    torch.manual_seed(seed)
    out = module(z)
    loss(out).backward()
    return out.detach(), z.grad, named_grads(module)


def layers_of(module):
    from stgcn_amd.vit import Layer
    return [m for m in module.modules() if isinstance(m, Layer)]


def both_paths(model, vit, inp, seed, loss, what, need_dz=True, expect_layers=2):
    """One step with the layers on HIP (asserted by a forward pre-hook on each) and one with everything on torch ops, same seed."""
    ran = []
    hooks = [l.register_forward_pre_hook(lambda mod, args: ran.append(mod.trains_on_hip(args[0]))) for l in layers_of(vit)]
    out, dz, grads = step(model, inp, seed, loss, need_dz)
    for h in hooks:
        h.remove()
    assert len(ran) == expect_layers and all(ran), "every Layer ran on the HIP training path"
    set_force_torch(vit, True)
    try:
        assert not any(l.trains_on_hip(torch.zeros(2, 100, 512, device=inp.device, requires_grad=True)) for l in layers_of(vit))
        out_t, dz_t, grads_t = step(model, inp, seed, loss, need_dz)
    finally:
        set_force_torch(vit, False)
    strict = MODEL_STRICT["default"]
    print(f"{what} logits: {parity_gate(out, out_t, REL, what + ' logits', strict):.3e}")
    if need_dz:
        print(f"{what} dz: {parity_gate(dz, dz_t, REL, what + ' dz', strict):.3e}")
    return out, grads, grads_t


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval_with_grad"])
def test_vit_trains_on_hip_like_the_torch_path(training, dev):
    """Depth 2, dropout 0.1.  In .train() both paths draw their masks from the generator after the same seed:
    ``Layer.draw_dropout`` makes the torch path's calls in its order, so the masks agree (this test is what confirms it on
    the GPU: a mask off by one element moves the result far beyond the gate)."""
    model = small_vit(dev).train(training)
    z = sr.make_input().to(dev)
    assert model.trains_on_hip(z.requires_grad_(True)) and not model.uses_hip(z)
    w = torch.randn(sr.CLIPS, sr.CONFIG["num_classes"], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    loss = lambda o: (o * w).sum()      # noqa: E731
    what = f"ViT {'train' if training else 'eval'}"
    out, grads, grads_t = both_paths(model, model, z.detach(), 77, loss, what)
    assert all(v is not None for v in grads.values())
    compare_grads(grads, grads_t, what, MODEL_STRICT["default"])
    if training:
        assert all(m is not None for l in layers_of(model) for m in l.draw_dropout(torch.zeros(2, 100, 512, device=dev)))
        assert not torch.equal(step(model, z, 78, loss)[0], out), "another seed draws other masks"
        assert torch.equal(step(model, z, 77, loss)[0], out), "the same seed reproduces the run bit for bit"
    else:
        assert all(l.draw_dropout(torch.zeros(2, 100, 512, device=dev)) == (None, None, None) for l in layers_of(model))


class StemAndViT(nn.Module):
    """gcn0 -> tcn0 (the fused stem) -> ViT, what the reference's ST_GCN_Trans runs with ``all_layers=False``."""

    def __init__(self, vit):
        super().__init__()
        import stgcn_amd
        from stgcn_amd.graphs import SHREGraph
        A = torch.from_numpy(SHREGraph("spatial").A.astype(np.float32))
        self.gcn0 = stgcn_amd.unit_agcn(3, 128, A)
        self.tcn0 = stgcn_amd.Unit2D(128, 128, kernel_size=9)
        self.v = vit
        stgcn_amd.enable_stem_fusion(self.gcn0, self.tcn0)

    def forward(self, x):
        return self.v(self.tcn0(self.gcn0(x.permute(0, 3, 1, 2))))


def test_one_training_step_through_the_fused_stem(dev):
    torch.manual_seed(3)
    model = StemAndViT(small_vit(dev)).to(dev).train()
    x = torch.randn(4, 180, 22, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    labels = torch.arange(4, device=dev) % 14
    ce = nn.CrossEntropyLoss()
    out, grads, grads_t = both_paths(model, model.v, x, 5, lambda o: ce(o, labels), "stem + ViT", need_dz=False)
    head = {k: v for k, v in grads.items() if k.startswith("v.")}
    assert head and all(v is not None for v in head.values())
    compare_grads(head, {k: v for k, v in grads_t.items() if k.startswith("v.")}, "stem + ViT", MODEL_STRICT["default"])
    assert any(not k.startswith("v.") and v is not None for k, v in grads.items()), "the stem got its gradients"


def test_uncovered_cpu_and_disabled_layers_train_through_torch_ops(dev, monkeypatch):
    from stgcn_amd.altformer import Block
    from stgcn_amd.vit import Attention, FeedForward, Layer, PreNorm
    torch.manual_seed(2)
    odd = Layer(PreNorm(384, Attention(384, heads=8, dim_head=48, dropout=0.1)), PreNorm(384, FeedForward(384, 768, dropout=0.1))).to(dev)
    odd.hip_train_min_tokens = 0
    x = torch.randn(4, 22, 384, device=dev, requires_grad=True)
    assert not odd.trains_on_hip(x), "head_dim 48"
    odd(x).sum().backward()
    assert x.grad is not None and all(p.grad is not None for p in odd.parameters())
    cpu = Layer(PreNorm(256, Attention(256, heads=8, dim_head=32, dropout=0.1)), PreNorm(256, FeedForward(256, 256, dropout=0.1)))
    cpu.hip_train_min_tokens = 0
    xc = torch.randn(2, 22, 256, requires_grad=True)
    assert not cpu.trains_on_hip(xc)
    cpu(xc).sum().backward()
    assert all(p.grad is not None for p in cpu.parameters())
    ok = cpu.to(dev)
    xd = torch.randn(2, 22, 256, device=dev, requires_grad=True)
    assert ok.trains_on_hip(xd), "covered, with all three dropouts live"
    ok.hip_train_min_tokens = 45
    assert not ok.trains_on_hip(xd), "44 tokens under a threshold of 45"
    ok.hip_train_min_tokens = 0
    monkeypatch.setenv("STGCN_VIT_TRAIN", "0")
    assert not ok.trains_on_hip(xd)
    for p in ok.parameters():
        p.grad = None
    ok(xd).sum().backward()
    assert xd.grad is not None and all(p.grad is not None for p in ok.parameters())
    monkeypatch.delenv("STGCN_VIT_TRAIN")
    with torch.no_grad():
        assert not ok.trains_on_hip(xd)
    blk = Block(256, 8, mlp_ratio=2., qkv_bias=True, drop=0.1).to(dev).train()
    blk.hip_train_min_tokens = 0
    assert not blk.trains_on_hip(torch.randn(2, 22, 256, device=dev)), "a Block with an active nn.Dropout: torch ops, as before"


# ---- 5. non-finite input and hostile buffers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_a_nan_stays_in_its_sequence(mode, dev):
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of("odd", dev)
    x = r.x.clone()
    x[2, 5, 17] = float("nan")          # sequence 2: drawn masks, kept by neither an all-zero nor an all-one mask
    y, g = run_layer(r, HEAD_TRAIN_MATH[mode], x=x)
    for t, what in ((y, "y"), (g["x"], "dx")):
        assert torch.isnan(t[2]).any(), f"{what} of the sequence that holds the NaN is non-finite"
        assert torch.isfinite(t[:2]).all(), f"{what} of every other sequence stays finite"


def make_drop_case(name, mode, tile, dev):
    from stgcn_amd import _capi
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    r = ref_of(name, dev)
    want = r.fp64(True)
    math = HEAD_TRAIN_MATH[mode] | getattr(_capi, tile)
    rel, strict = (BF16_REL, False) if mode == "bf16" else (REL, TRAIN_STRICT[mode])

    def run():
        y, g = run_layer(r, math, scales=True)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def gate(o, what):
        parity_gate(o["y"], want[0], rel, f"{what} y", strict)
        for k, v in want[1].items():
            parity_gate(o["d" + k], v, rel, f"{what} d{k}", strict)
    return run, gate


DROP_CASES = [Case(f"vit_block_train_drop-{n}-{m}-{t}", lambda dev, n=n, m=m, t=t: make_drop_case(n, m, t, dev), True)
              for n, m, t in (("vit", "f32", "VIT_TILE_AUTO"), ("odd", "f32", "VIT_TILE_32"), ("odd", "bf16", "VIT_TILE_64"))]


@pytest.mark.parametrize("case", DROP_CASES, ids=lambda c: c.id)
def test_drop_pair_under_poisoned_guard_banded_buffers(case, dev):
    run_under_both_fills(case, dev)
