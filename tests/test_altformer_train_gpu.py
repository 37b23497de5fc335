"""GPU tests of the AltFormer heads' HIP training path: the three backward entry points against fp64 autograd of the same
formula, one block's forward_train + backward against the reference's gradient fixture
(tests/golden/make_golden_altformer_train.py) and, with stochastic-depth factors, against the fp64 restatement
(tests/altformer_train_ref.py); bit-equality with the eval forward, run-to-run determinism, and the modules' path rule up to
the whole model and nn.DataParallel replicas, against the same modules on their torch-op path."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF
from torch.nn.parallel import parallel_apply

import altformer_ref as ar
import altformer_train_ref as tr
from _util import MATH_GATES, gather_flat, load_golden, parity_gate
from entry_points import TRAIN_STRICT, attention_grad64, run_block
from test_altformer_gpu import LINEAR_SHAPES, gate_on_device, peaked_qkv, small_head, whole_model

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
MODES = sorted(TRAIN_STRICT)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref():
    return load_golden("altformer_train_reference")


# ---- 4. the backward entry points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_backward_vs_fp64(shape, math, dev):
    """dgrad with every (GELU', accumulate) combination, wgrad and bias gradient, against fp64 products on the device."""
    from stgcn_amd import functional as F
    M, K, Nout = shape
    g = torch.Generator(device=dev).manual_seed(M + K + Nout)
    dy = torch.randn(M, Nout, generator=g, device=dev) * (0.25 + 3.75 * torch.rand(M, 1, generator=g, device=dev))
    a = torch.randn(M, K, generator=g, device=dev) + 0.5
    W = (torch.rand(Nout, K, generator=g, device=dev) * 2 - 1) / K ** 0.5
    h = torch.randn(M, K, generator=g, device=dev) * 1.5
    old = torch.randn(M, K, generator=g, device=dev)
    mode = getattr(F, "MATH_" + math.upper())
    assert F.vit_linear_backward_supported(M, K, Nout, mode)
    base = dy.double() @ W.double()
    h64 = h.double().requires_grad_(True)
    TF.gelu(h64).sum().backward()
    for dgelu, accum in itertools.product((False, True), repeat=2):
        want = base * h64.grad if dgelu else base
        if accum:
            want = want + old.double()
        dx, _, _ = F.vit_linear_backward(dy, a, W, h_pre=h if dgelu else None, dx_accumulate=old.clone() if accum else None,
                                         need_dw=False, math=mode)
        gate_on_device(dx, want, REL, f"linear backward {shape} {math} dx gelu'={dgelu} accumulate={accum}")
    _, dW, db = F.vit_linear_backward(dy, a, W, need_dx=False, math=mode)
    gate_on_device(dW, dy.double().T @ a.double(), REL, f"linear backward {shape} {math} dW")
    gate_on_device(db, dy.double().sum(0), REL, f"linear backward {shape} {math} db")
    _, dW2, none = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=False, math=mode)
    assert none is None and torch.equal(dW, dW2), "the weight gradient is bit-identical from run to run"


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [1, 22, 46, 64, 65, 150, 180, 256])
def test_attention_backward_vs_fp64(L, hd, dev):
    from stgcn_amd import functional as F
    B, heads = 9, 8
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd)
    dout = torch.randn(B, L, heads * hd, generator=torch.Generator().manual_seed(L + hd))
    for scale in (None, 0.37):
        _, want = attention_grad64(qkv, dout, heads, scale or hd ** -0.5)
        out = F.vit_attention(qkv.to(dev), heads, scale=scale)
        dqkv = F.vit_attention_backward(qkv.to(dev), out, dout.to(dev), heads, scale=scale)
        rel = parity_gate(dqkv, want, REL, f"attention backward L={L} hd={hd} scale={scale}")
        print(f"attention backward L={L} hd={hd} scale={scale}: {rel:.3e}")
        assert torch.equal(dqkv, F.vit_attention_backward(qkv.to(dev), out, dout.to(dev), heads, scale=scale))


@pytest.mark.parametrize("D", [256, 512])
def test_layernorm_backward_vs_fp64(D, dev):
    from stgcn_amd import functional as F
    M = 3001
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, D, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dn, dres = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    ar.layer_norm64(x64, w64, b64).backward(dn.double())
    for res in (False, True):
        dx, dw, db = F.vit_layernorm_backward(x.to(dev), dn.to(dev), w.to(dev), ar.EPS, dres=dres.to(dev) if res else None)
        print(f"layernorm backward D={D} residual={res}: dx",
              f"{parity_gate(dx, x64.grad + (dres.double() if res else 0), REL, 'layernorm dx'):.3e}",
              f"dweight {parity_gate(dw, w64.grad, REL, 'layernorm dweight'):.3e}",
              f"dbias {parity_gate(db, b64.grad, REL, 'layernorm dbias'):.3e}")


# ---- 5.-7. one block --------------------------------------------------------------------------------------------------------
def block_params(blk):
    return list(blk._weights())


def gate_stored(out, ref, key, what, strict):
    if key in ref:
        rel = parity_gate(out, ref[key], REL, what, strict)
    else:
        rel = parity_gate(gather_flat(out.detach().cpu(), ref[key + "_idx"].astype(np.int64)), ref[key + "_val"], REL, what, strict)
    print(f"{what}: {rel:.3e}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_gradients_vs_reference_case(name, mode, ref, dev):
    from stgcn_amd.altformer import Block
    pre = f"case.{name}."
    x, dy = ar.make_input(name), tr.make_dy(name)
    assert torch.equal(gather_flat(dy, ref[pre + "dy_idx"].astype(np.int64)), torch.from_numpy(ref[pre + "dy_val"]))
    blk = ar.build_block(Block, name).to(dev)
    y, g = run_block(blk, x.to(dev), dy.to(dev), mode)
    fwd = load_golden("altformer_reference")
    gate_stored(y, fwd, pre + "y", f"{name} {mode} y", TRAIN_STRICT[mode])
    for k, v in g.items():
        if v is None:
            assert k == "attn.qkv.bias" and pre + "dattn.qkv.bias_absmax" not in ref
            continue
        gate_stored(v, ref, pre + "d" + k, f"{name} {mode} d{k}", TRAIN_STRICT[mode])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_with_stochastic_depth_vs_fp64(name, mode, dev):
    from stgcn_amd.altformer import Block
    B, L, D, _, _, seed = ar.BLOCK_CASES[name]
    x, dy = ar.make_input(name), tr.make_dy(name)
    s1, s2 = tr.make_scales(B, seed)
    assert (s1 == 0).any() and (s1 > 1).any() and (s2 == 0).any() and not torch.equal(s1, s2)
    blk = ar.build_block(Block, name)
    want_y, want = tr.grads64(x, blk.state_dict(), dy, scale=blk.attn.scale, s1=s1, s2=s2)
    blk = blk.to(dev)
    y, g = run_block(blk, x.to(dev), dy.to(dev), mode, s1.to(dev), s2.to(dev))
    print(f"{name} {mode} masked y: {parity_gate(y, want_y, REL, f'{name} {mode} masked y', TRAIN_STRICT[mode]):.3e}")
    for k, v in want.items():
        print(f"{name} {mode} masked d{k}: {parity_gate(g[k], v, REL, f'{name} {mode} masked d{k}', TRAIN_STRICT[mode]):.3e}")
    dropped = (s1 == 0) & (s2 == 0)
    if dropped.any():
        assert torch.equal(g["x"][dropped.to(dev)], dy.to(dev)[dropped.to(dev)]), "a sequence with both branches dropped: dx = dy"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["st_spatial_L22_D256", "st_temporal_L180_D512"])
def test_forward_train_is_bit_equal_to_the_eval_forward(name, mode, dev):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH, Block
    blk = ar.build_block(Block, name).to(dev)
    x = ar.make_input(name).to(dev)
    ps = [None if p is None else p.detach() for p in block_params(blk)]
    a, m = blk.attn, blk.mlp
    y_eval = F.vit_block_forward(x, ps[0:2], ps[2:4], ps[4:6], ps[6:8], ps[8:10], ps[10:12], a.num_heads, ar.EPS, a.scale,
                                 HEAD_MATH[mode])
    y_train, _ = F.vit_block_forward_train(x, ps, a.num_heads, ar.EPS, a.scale, HEAD_MATH[mode])
    assert torch.equal(y_eval, y_train)


def test_two_runs_are_bit_identical_at_batch_size(dev):
    """3000 x 22 x 256: three slabs of whole sequences and more than one split of every weight-gradient reduction."""
    from stgcn_amd import _capi
    from stgcn_amd.altformer import Block
    blk = ar.build_block(Block, "st_spatial_L22_D256").to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(3000, 22, 256, device=dev, generator=g)
    dy = torch.randn(3000, 22, 256, device=dev, generator=g)
    s1, s2 = (t.to(dev) for t in tr.make_scales(3000, 1))
    assert 3000 * 22 > 2 * 32768 and _capi.lib().stgcn_vit_block_backward_ws_bytes(3000, 22, 256, 512) == \
        _capi.lib().stgcn_vit_block_backward_ws_bytes(6000, 22, 256, 512), "the input is walked in slabs"
    for mode in ("f32", "mixed"):
        y1, g1 = run_block(blk, x, dy, mode, s1, s2)
        y2, g2 = run_block(blk, x, dy, mode, s1, s2)
        assert torch.equal(y1, y2)
        for k in g1:
            assert torch.equal(g1[k], g2[k]), f"{mode}: d{k} differs between two runs"


# ---- 8.-10. modules -----------------------------------------------------------------------------------------------------------
def named_grads(module):
    return {k: None if p.grad is None else p.grad.clone() for k, p in module.named_parameters()}


def set_force_torch(module, flag):
    from stgcn_amd.altformer import Block
    for m in module.modules():
        if isinstance(m, Block):
            m.force_torch = flag


def step(module, inp, seed, loss=lambda out: (out * out).sum(), need_dz=True):
    """Zero the gradients, seed, run forward + backward; returns (output, input gradient or None, parameter gradients)."""
    for p in module.parameters():
        p.grad = None
    z = inp.detach().clone().requires_grad_(need_dz)
    torch.manual_seed(seed)
    out = module(z)
    loss(out).backward()
    return out.detach(), z.grad, named_grads(module)


class PinnedMax:
    """Stand-in for altformer.max_over_tokens while two arithmetic paths are compared.  The gradient of a maximum goes to the
    token that holds it, so where two tokens tie to within the forward's own tolerance the two paths may pick different ones
    and their gradients then differ by whole elements, not by rounding (seen: one pick of 33,792 differs, the two candidates
    one ulp apart, and 24 % of max|dz| with it).  The first run records its picks, the second takes the same tokens - after
    asserting that each is its own maximum to within 2 * REL * max|x|, i.e. that only such ties can have been re-decided."""

    def __init__(self):
        self.picks, self.replay = [], None

    def __call__(self, x):
        if self.replay is None:
            idx = x.argmax(dim=1, keepdim=True)
            self.picks.append(idx)
        else:
            idx = self.replay.pop(0)
            gap = (x.max(dim=1, keepdim=True).values - x.gather(1, idx)).max().item()
            assert gap <= 2 * REL * x.abs().max().item(), f"pooling picks differ beyond a tie: {gap:.3e}"
        return x.gather(1, idx).squeeze(1)

    def second_run(self):
        self.replay, self.picks = self.picks, []

    def record(self):
        self.replay, self.picks = None, []


@pytest.fixture
def pinned_max(monkeypatch):
    from stgcn_amd import altformer
    pin = PinnedMax()
    monkeypatch.setattr(altformer, "max_over_tokens", pin)
    return pin


def compare_grads(got, want, what, strict=True):
    assert got.keys() == want.keys()
    for k in want:
        assert (got[k] is None) == (want[k] is None), f"{what}: {k} has a gradient on one path only"
        if want[k] is not None:
            print(f"{what} d{k}: {parity_gate(got[k], want[k], REL, f'{what} d{k}', strict):.3e}")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval_with_grad"])
@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_head_trains_on_hip_like_the_torch_path(cls_name, training, dev, pinned_max):
    from stgcn_amd.altformer import Block, DropPath
    head = small_head(dev, cls_name).train(training)
    z = torch.randn(6, 128, 40, 22, device=dev)
    blocks = [m for m in head.modules() if isinstance(m, Block)]
    assert sum(isinstance(b.drop_path, DropPath) for b in blocks) == 2, "stochastic depth is active in two of the four blocks"
    ran = []
    hooks = [b.register_forward_pre_hook(lambda mod, args: ran.append(mod.trains_on_hip(args[0]))) for b in blocks]
    out, dz, grads = step(head, z, 77)
    for h in hooks:
        h.remove()
    assert len(ran) == 4 and all(ran), "every block ran on the HIP training path"
    set_force_torch(head, True)
    assert not any(b.trains_on_hip(torch.zeros(2, 22, b.norm1.normalized_shape[0], device=dev, requires_grad=True)) for b in blocks)
    pinned_max.second_run()
    out_t, dz_t, grads_t = step(head, z, 77)
    pinned_max.record()
    what = f"{cls_name} {'train' if training else 'eval'}"
    print(f"{what} logits: {parity_gate(out, out_t, REL, what + ' logits'):.3e}")
    print(f"{what} dz: {parity_gate(dz, dz_t, REL, what + ' dz'):.3e}")
    compare_grads(grads, grads_t, what)
    if training:
        set_force_torch(head, False)
        out2, _, _ = step(head, z, 78)
        assert not torch.equal(out, out2), "another seed draws other masks"
        assert torch.equal(step(head, z, 77)[0], out), "the same seed reproduces the run bit for bit"


def test_uncovered_shape_and_cpu_block_train_through_torch_ops(dev):
    from stgcn_amd.altformer import Block
    torch.manual_seed(2)
    blk = Block(384, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.1, norm_layer=ar.norm_layer()).to(dev).train()   # head_dim 48
    blk.hip_train_min_tokens = 0
    x = torch.randn(4, 22, 384, device=dev, requires_grad=True)
    assert not blk.trains_on_hip(x)
    blk(x).sum().backward()
    assert x.grad is not None and all(p.grad is not None for p in blk.parameters())
    cpu = Block(256, 8, mlp_ratio=2., qkv_bias=True).train()
    cpu.hip_train_min_tokens = 0
    xc = torch.randn(2, 22, 256, requires_grad=True)
    assert not cpu.trains_on_hip(xc)
    cpu(xc).sum().backward()
    assert all(p.grad is not None for p in cpu.parameters())
    ok = Block(256, 8, mlp_ratio=2., qkv_bias=True, drop=0.1).to(dev).train()
    ok.hip_train_min_tokens = 0
    assert not ok.trains_on_hip(torch.randn(2, 22, 256, device=dev)), "an active nn.Dropout: torch ops"
    assert ok.eval().trains_on_hip(torch.randn(2, 22, 256, device=dev))
    with torch.no_grad():
        assert not ok.trains_on_hip(torch.randn(2, 22, 256, device=dev)) and ok.hip_applies(torch.randn(2, 22, 256, device=dev))


def check_stem_grads(got, want, strict):
    """test_data_parallel._check_stem_grads with the criterion as an argument: structurally zero biases (rounding noise on
    both sides) are held against the scale of the matching weight's gradient, everything else goes through parity_gate."""
    from test_data_parallel import _STRUCTURAL_ZERO
    for name, g in got.items():
        if not name.startswith(("gcn0.", "tcn0.")):
            continue
        assert g is not None, f"{name}: no gradient"
        w = _STRUCTURAL_ZERO.get(name)
        if w is None and name.endswith(".bias") and name.startswith(("gcn0.conv_a.", "gcn0.conv_d.")):
            w = name[:-len("bias")] + "weight"
        if w is None:
            print(f"stem d{name}: {parity_gate(g, want[name], REL, name, strict):.3e}")
        else:
            err = (g - want[name]).abs().max().item()
            assert err <= REL * max(want[name].abs().max().item(), want[w].abs().max().item()), f"{name}: {err:.3e}"


# Through the twelve blocks of a head the bf16x3 products' error adds up: 'mixed' stays at 1.1e-5 of max|.| on every
# gradient of the whole model, but then misses the second criterion on one or two of its 337 tensors (measured ratio to its
# bound: 1.0-1.9) - the reason it is not the default training arithmetic.  It is tested with the criterion it holds.
MODEL_STRICT = {"default": True, "mixed": False}


@pytest.mark.parametrize("mode", sorted(MODEL_STRICT))
@pytest.mark.parametrize("style", ["ST", "TS", None])
def test_whole_model_training_step_matches_the_torch_path(style, mode, dev, pinned_max):
    """8 fixture clips through stgcn_amd.ST_GCN_AltFormer in .train() (stochastic depth on, BatchNorm on batch statistics):
    CrossEntropyLoss, one backward; logits, stem and head gradients against the same model with its blocks on torch ops."""
    from stgcn_amd.altformer import Block
    from stgcn_amd.altformer import DEFAULT_TRAIN_MATH, set_head_math
    assert DEFAULT_TRAIN_MATH == "f32"
    model, g = whole_model(style, dev)
    if mode != "default":
        set_head_math(model, mode)
    model.train()
    x = torch.from_numpy(g["skeleton"]).to(dev)
    labels = torch.arange(8, device=dev) % 14
    ce = nn.CrossEntropyLoss()
    ran = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: ran.append(mod.trains_on_hip(args[0])))
             for m in model.modules() if isinstance(m, Block)]
    out, _, grads = step(model, x, 5, lambda o: ce(o, labels), need_dz=False)
    for h in hooks:
        h.remove()
    assert len(ran) == (24 if style is None else 12) and all(ran)
    set_force_torch(model, True)
    pinned_max.second_run()
    out_t, _, grads_t = step(model, x, 5, lambda o: ce(o, labels), need_dz=False)
    print(f"whole model {style} {mode} logits: {parity_gate(out, out_t, REL, f'whole model {style} logits'):.3e}")
    check_stem_grads(grads, grads_t, MODEL_STRICT[mode])
    stem = ("gcn0.", "tcn0.")
    assert any(k.startswith(stem) for k in grads) and any(not k.startswith(stem) and v is not None for k, v in grads.items())
    compare_grads({k: v for k, v in grads.items() if not k.startswith(stem)},
                  {k: v for k, v in grads_t.items() if not k.startswith(stem)}, f"whole model {style} {mode}", MODEL_STRICT[mode])


def test_replicas_send_their_gradients_to_the_master(dev):
    from test_data_parallel import _replicas
    head = small_head(dev, "ST")                      # .eval(): no masks, so the halves can be compared one by one
    z = torch.randn(8, 128, 40, 22, device=dev)
    want = None
    for half in (z[:4], z[4:]):
        _, _, gh = step(head, half, 1, lambda o: o.sum())
        want = gh if want is None else {k: None if v is None else v + gh[k] for k, v in want.items()}
    for p in head.parameters():
        p.grad = None
    outs = parallel_apply(_replicas(head, 2), [(z[:4],), (z[4:],)], devices=[dev, dev])
    (outs[0].sum() + outs[1].sum()).backward()
    compare_grads(named_grads(head), want, "two replicas vs the sum of the halves")
    head.train()
    for p in head.parameters():
        p.grad = None
    dp = nn.DataParallel(head, device_ids=[dev.index or 0])
    dp(z).sum().backward()
    unused = ("Spatial_cls_token", "cls_token", "Spatial_norm.", "Temporal_norm.", "weighted_mean.", "fcn.")
    for k, p in head.named_parameters():
        assert (p.grad is not None) != k.startswith(unused), k
