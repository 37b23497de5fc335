"""GPU tests of the alignment contract (include/stgcn_hip.h, "Alignment"; DESIGN.md section 4 has the table of operands).

A tensor operand needs the alignment of its element only, so a contiguous view at any element offset - a batch slice, a
parameter that lives in a flat buffer, a cotangent that is a slice of a larger gradient, a caller's ``out`` - is served in
place.  Every case below runs an entry point once on operands from the allocator and again with one kind of operand moved
off that alignment (tests/_util.py::skewed: 256-byte boundary + k elements, a NaN-filled guard band either side):

* the input, at 4 (mod 8) and 8 (mod 16) bytes, and as a real slice ``x[1:]`` / ``logits[1:]`` at 8 and 12 (mod 16);
* every parameter and buffer of the module as a view into one flat buffer at 4 (mod 16), through ``p.data = view``;
* the cotangent, one element off;
* the fused stem's ``out``, fp32 and bf16 (2 (mod 4) bytes).

Where the path is deterministic every output and gradient equals the aligned run bit for bit; the two training families whose
reductions use atomics (unit_agcn, Unit2D) pass the fp64 reference and gate of their own tests instead, in every variant.  The
guards stay intact.  The operands that entry points list as exceptions, and the blobs, are refused by name before anything
is written; the modules and autograd functions hand those through ``functional.aligned`` and never surface a refusal.

The setups are tests/entry_points.py's, the rows the buffer and non-finite contracts use."""
import copy
import functools
import re

import pytest
import torch

import altformer_ref as ar
import altformer_train_ref as tr
import entry_points as ep
import st_attention_ref as R
import stvit_ref as sr
from _util import grad_gate, hostile_allocations, parity_gate, skewed
from entry_points import AGCN_SHAPES, STEM_KERNELS, TCN_KERNELS, TCN_SHAPES, _stem_kernel, _tcn_mode, hipF as _F, math_flag as _math

pytestmark = pytest.mark.gpu
SKEWS = (1, 2)            # fp32 elements past the boundary: 4 (mod 8) and 8 (mod 16) bytes


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def same_bits(got, want, what):
    assert set(got) == set(want), f"{what}: {sorted(got)} vs {sorted(want)}"
    for k, w in want.items():
        g = got[k]
        assert (g is None) == (w is None), f"{what}: {k}"
        if w is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} is {tuple(g.shape)} {g.dtype}"
            assert torch.equal(g, w), f"{what}: {k} differs from the aligned run ({int((g != w).sum())} of {w.numel()} elements)"


def checked(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        t.check()


def rebase_parameters(module, dev):
    """Every fp32 parameter and buffer of ``module`` becomes a view into ONE flat buffer, each starting 4 bytes past a 16-byte
    boundary, through ``p.data = view`` - what torch.nn.utils.vector_to_parameters does with a flat vector.  Returns the
    buffer (whose bytes between the tensors are NaN) and the number of tensors moved."""
    tensors = [t for t in list(module.parameters()) + list(module.buffers()) if t.dtype == torch.float32 and t.numel()]
    total = sum((t.numel() + 3) // 4 * 4 + 4 for t in tensors) + 8
    flat = torch.full((total,), float("nan"), device=dev)
    assert flat.data_ptr() % 16 == 0
    at = 1
    for t in tensors:
        view = flat[at:at + t.numel()].view(t.shape)
        view.copy_(t.detach())
        t.data = view
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        at += (t.numel() + 3) // 4 * 4 + 4
    return flat, len(tensors)


# ---- 1. the input of every inference setup --------------------------------------------------------------------------------------
# (id, make() -> Setup).  Every path here is deterministic (the buffer contract's ``bitwise`` flag of the same rows): bit-equal.
INPUT_ROWS = []
for _s in AGCN_SHAPES:
    INPUT_ROWS.append(("agcn_forward-" + "x".join(map(str, _s)), functools.partial(ep.agcn, *_s)))
for _s in TCN_SHAPES:
    INPUT_ROWS.append(("tcn-" + "x".join(map(str, _s[:7])) + f"-{_s[7]}" + ("-bf16out" if _s[8] else "") + ("-alongV" if _s[9] else ""),
                       functools.partial(ep.tcn, *_s)))
for _o in ("ST", "TS"):
    INPUT_ROWS.append((f"patch_embed-{_o}", functools.partial(ep.patch_embed, _o, "nctv")))
for _s in [(2, 131, 128, 12, 22), (5, 64, 128, 33, 25), (2, 256, 512, 3, 46)]:
    INPUT_ROWS.append(("st_attention_forward-" + "x".join(map(str, _s)), functools.partial(ep.st_attention, *_s)))
for _m, (_k, _n) in ((1, (32, 64)), (129, (96, 100)), (300, (256, 200)), (129, (512, 1536))):
    for _ma in ("f32", "bf16x3"):
        INPUT_ROWS.append((f"vit_linear-{_m}x{_k}x{_n}-{_ma}", functools.partial(ep.vit_linear, _m, _k, _n, _ma)))
for _form, _b, _l, _hd in [("resident", 9, 33, 32), ("resident", 9, 256, 64), ("stream", 3, 65, 64), ("stream", 3, 300, 32),
                           ("split", 2, 65, 32), ("split", 2, 256, 64)]:
    INPUT_ROWS.append((f"vit_attention-{_form}-{_b}x{_l}-hd{_hd}", functools.partial(ep.vit_attention, _form, _b, _l, _hd)))
for _s in [(7, 1, 256, 8, 512), (3, 65, 512, 8, 1024)]:
    for _mo in ("f32", "mixed"):
        INPUT_ROWS.append(("vit_block_forward-" + "x".join(map(str, _s)) + "-" + _mo, functools.partial(ep.vit_block, *_s, _mo)))


@pytest.mark.parametrize("make", [r[1] for r in INPUT_ROWS], ids=[r[0] for r in INPUT_ROWS])
def test_an_input_off_16_bytes_gives_the_aligned_bits(make, dev):
    s = make()
    run, xd = s.on(dev), s.x.to(dev)
    want = run(xd)
    for k in SKEWS:
        xs = skewed(xd, k)
        assert xs.data_ptr() % 16 == 4 * k
        got = run(xs)
        checked(xs)
        same_bits(got, want, f"x at {4 * k} (mod 16)")
    # a real slice: one clip (row) in front, the view behind it starts wherever the clip's size puts it
    big = torch.cat([xd[:1], xd])
    same_bits(run(big[1:]), want, f"x[1:], {big[1:].data_ptr() % 16} (mod 16)")


def test_the_conv_rows_reach_every_kernel():
    assert {_tcn_mode(ci, co, K, s, T, V, m, av)[1] for ci, co, K, s, T, V, N, m, ob, av in TCN_SHAPES} == TCN_KERNELS


def test_patch_embed_reads_a_channels_last_input_in_place_off_16_bytes(dev):
    F = _F()
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 128, 9, 25, generator=g).to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    W, b = (torch.randn(256, 128, generator=g) / 11).to(dev), torch.randn(256, generator=g).to(dev)
    pos = torch.randn(1, 25, 256, generator=g).to(dev)
    want = F.patch_embed(z, W, b, pos, order="ST")
    for k in SKEWS:
        zs = skewed(z, k)
        assert F._is_channels_last(zs) and zs.data_ptr() % 16 == 4 * k
        got = F.patch_embed(zs, W, b, pos, order="ST")
        checked(zs)
        assert torch.equal(got, want), f"channels-last z at {4 * k} (mod 16)"
    Ws, bs, ps = skewed(W, 1), skewed(b, 1), skewed(pos, 1)
    assert torch.equal(F.patch_embed(z, Ws, bs, ps, order="ST"), want), "weight, bias and pos at 4 (mod 16)"
    checked(Ws, bs, ps)


def test_step_stats_on_a_logits_slice_and_a_skewed_probe(dev):
    """``logits[1:]`` of an (N, 14) tensor starts at 56 = 8 (mod 16) bytes; the probed output fp32 and bf16 one element off."""
    from stgcn_amd import dist as sd
    n, classes = 300, 14
    g = torch.Generator().manual_seed(3)
    big = (torch.randn(n + 1, classes, generator=g) * 4).round().div(4).to(dev)
    logits = big[1:].clone()
    labels = torch.randint(0, classes, (n,), generator=g).to(dev)
    out = torch.randn(n, 4, 2, 3, generator=g).to(dev)
    assert big[1:].data_ptr() % 16 == 8 and logits.data_ptr() % 16 == 0
    for o in (out, out.bfloat16()):
        pred, pred_s = (torch.full((n,), -1, dtype=torch.int64, device=dev) for _ in range(2))
        want = sd.step_stats(o, n, logits, labels, pred)
        os_ = skewed(o, 1)
        got = sd.step_stats(os_, n, big[1:], labels, pred_s)
        checked(os_)
        assert torch.equal(got, want) and torch.equal(pred_s, pred) and bool((pred >= 0).all()), o.dtype


# ---- 2. the fused stem: input, the caller's result and workspace ---------------------------------------------------------------------
STEM_ROWS = [((3, 37, 22, 128), "f32"), ((3, 37, 22, 128), "bf16x3"), ((3, 37, 22, 128), "bf16"), ((3, 37, 22, 128), "f16mx"),
             ((2, 23, 7, 128), "f32"), ((2, 23, 7, 128), "bf16x3"), ((3, 40, 22, 256), "bf16x3"), ((2, 2, 52, 128), "bf16x3")]


def test_the_stem_rows_reach_every_kernel():
    assert {_stem_kernel(s, m) for s, m in STEM_ROWS} == STEM_KERNELS


@functools.lru_cache(maxsize=None)
def _stem(shape, dev):
    s = ep.stem(*shape)
    return s.on(dev), s.x.to(dev)


def _stem_call(staged, x, prep, mode, C, bf16=False, cl_out=False, out=None, ws=None):
    st, ts = staged.st, staged.ts
    return _F().stem_forward(x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], prep, ts["shift"], C, 9, mode, bf16, out=out,
                             ws=ws, channels_last_out=cl_out)


@pytest.mark.parametrize("shape,math", STEM_ROWS, ids=["x".join(map(str, s)) + "-" + m for s, m in STEM_ROWS])
def test_the_stem_serves_input_and_result_off_16_bytes(shape, math, dev):
    F = _F()
    N, T, V, C = shape
    staged, xd = _stem(shape, dev)
    mode = _math(math)
    prep = staged.prepare(mode)
    x_cl = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    for bf16 in (False, True):
        for cl_out in (False, True):
            what = f"{'bf16' if bf16 else 'f32'} {'ntvc' if cl_out else 'nctv'} result"
            out0, P0 = _stem_call(staged, xd, prep, mode, C, bf16, cl_out)
            out0, P0 = out0.clone(), P0.clone()
            # the input: contiguous and channels-last (read in place), 4 (mod 8) and 8 (mod 16)
            for k in SKEWS if not (bf16 or cl_out) else SKEWS[:1]:
                for x in (skewed(xd, k), skewed(x_cl, k)):
                    assert x.data_ptr() % 16 == 4 * k and F._is_channels_last(x) == (x.stride() == x_cl.stride())
                    out, P = _stem_call(staged, x, prep, mode, C, bf16, cl_out)
                    checked(x)
                    assert torch.equal(out, out0) and torch.equal(P, P0), f"{what}: x at {4 * k} (mod 16), strides {x.stride()}"
            # the caller's result, one element off: 4 (mod 16) bytes fp32, 2 (mod 4) bytes bf16
            target = skewed(torch.zeros((N, T, V, C) if cl_out else (N, C, T, V), device=dev, dtype=out0.dtype), 1)
            assert target.data_ptr() % 4 == (2 if bf16 else 0) and target.data_ptr() % 16 == target.element_size()
            out, P = _stem_call(staged, xd, prep, mode, C, bf16, cl_out, out=target)
            checked(target)
            assert out.data_ptr() == target.data_ptr(), "the result is not the caller's tensor"
            assert torch.equal(out, out0) and torch.equal(P, P0), f"{what} one element off"
    # the real slice: x[1:] of a batch with one more clip (8 (mod 16) at 37 x 22, 12 at 23 x 7, 0 at the others)
    big = torch.cat([xd[:1], xd])
    out, P = _stem_call(staged, big[1:], prep, mode, C)
    out0, P0 = _stem_call(staged, xd, prep, mode, C)
    assert torch.equal(out, out0) and torch.equal(P, P0), f"x[1:] at {big[1:].data_ptr() % 16} (mod 16)"


def test_the_stem_slices_sit_at_8_and_12_mod_16(dev):
    for shape, want in (((3, 37, 22, 128), 8), ((2, 23, 7, 128), 12)):
        _, xd = _stem(shape, dev)
        assert torch.cat([xd[:1], xd])[1:].data_ptr() % 16 == want


# ---- 3. training: input, cotangent and parameters ------------------------------------------------------------------------------------
def _step(m, x, dy, want_dx):
    for p in m.parameters():
        p.grad = None
    xg = x.detach().requires_grad_(want_dx)          # (a view at the same address)
    y = m(xg)
    y.backward(dy)
    assert all(p.grad is not None for p in m.parameters() if p.requires_grad), "a gradient did not arrive in p.grad"
    return y.detach(), xg.grad


def _variants(run, xd, dyd, dev):
    """{variant: outputs}: 'aligned', the input at 4 (mod 8) and 8 (mod 16), the cotangent one element off, the parameters and
    buffers in a flat buffer at 4 (mod 16).  ``run(x, dy, rebase)`` steps a fresh copy of the module."""
    outs = {"aligned": run(xd, dyd, False)}
    for k in SKEWS:
        xs = skewed(xd, k)
        outs[f"x at {4 * k} (mod 16)"] = run(xs, dyd, False)
        checked(xs)
    dys = skewed(dyd, 1)
    outs["dy at 4 (mod 16)"] = run(xd, dys, False)
    checked(dys)
    outs["parameters at 4 (mod 16)"] = run(xd, dyd, True)
    return outs


AGCN_TRAIN = [(3, 128, 3, 20, 22, False, False), (64, 64, 2, 12, 22, True, False), (64, 128, 2, 9, 25, True, True)]


@pytest.mark.parametrize("cin,cout,N,T,V,want_dx,frozen", AGCN_TRAIN, ids=["x".join(map(str, s[:5])) + ("-frozen" if s[6] else "") for s in AGCN_TRAIN])
def test_unit_agcn_trains_on_operands_off_16_bytes(cin, cout, N, T, V, want_dx, frozen, dev):
    """Not bit-reproducible (fp64 atomics in the batch sums, fp32 atomics in the moment form's dPA): every variant passes the
    fp64 oracle and the gate of test_unit_agcn_backward_vs_oracle / test_eval_mode_backward_unit_agcn_vs_oracle."""
    s = ep.agcn_train(cin, cout, N, T, V, want_dx, kink_free=True, frozen=frozen)
    want = s.reference(s.x)
    ref = {k: want["d" + k] for k in s.leaves}
    master = s.module.to(dev).train(not frozen)

    def run(x, dy, rebase):
        m = copy.deepcopy(master)
        m.A = master.A
        if rebase:
            flat, moved = rebase_parameters(m, dev)
            assert moved >= len(list(m.parameters()))
        y, dx = _step(m, x, dy, want_dx)
        return {"y": y, "dx": dx, **ep.agcn_module_grads(m)}

    for what, o in _variants(run, s.x.to(dev), s.cotangent[0].to(dev), dev).items():
        parity_gate(o["y"], want["y"], 1e-4, f"{what} forward")
        got = {k: o[k] for k in ref}
        if not frozen:
            ep.agcn_compare_grads(got, ref, 1e-4)
        else:                                   # behind frozen statistics the conv_d / down biases have real gradients
            for k in s.leaves:
                scale = ref[k].abs().max().item()
                if k.startswith("a_b"):
                    scale = max(scale, ref["a_w" + k[3:]].abs().max().item())
                err = (got[k].reshape(ref[k].shape).double().cpu() - ref[k]).abs().max().item()
                assert err <= 1e-4 * max(scale, 1e-30), f"{what} d{k}: err {err:.3e} vs 1e-4*{scale:.3e}"
        if want_dx:
            grad_gate(o["dx"], want["dx"], 1e-4, f"{what} dx")


TCN_TRAIN = [(128, 128, 9, 1, 3, 21, 22, True, "bf16x3"), (64, 128, 9, 2, 2, 21, 22, True, "bf16x3"), (128, 256, 9, 1, 3, 13, 17, True, "bf16x3"),
             (32, 64, 2, 1, 2, 7, 22, True, "f32_valu"), (128, 256, 9, 2, 2, 31, 25, False, "f32_valu")]


@pytest.mark.parametrize("cin,cout,K,stride,N,T,V,bias,math", TCN_TRAIN, ids=["x".join(map(str, s[:7])) + "-" + s[8] for s in TCN_TRAIN])
def test_unit2d_trains_on_operands_off_16_bytes(cin, cout, K, stride, N, T, V, bias, math, dev):
    """Not bit-reproducible (atomics in the channel sums, the VALU weight gradient and the statistics): every variant passes the
    fp64 oracle and the gate of test_unit2d_backward_vs_oracle."""
    s = ep.tcn_train(cin, cout, K, stride, N, T, V, math, bias=bias, kink_free=True)
    want = s.reference(s.x)
    master = s.module.to(dev).train()

    def run(x, dy, rebase):
        m = copy.deepcopy(master)
        if rebase:
            rebase_parameters(m, dev)
        y, dx = _step(m, x, dy, True)
        return {"y": y, "dx": dx, "dW": m.conv.weight.grad.reshape(cout, cin, K), "dgamma": m.bn.weight.grad, "dbeta": m.bn.bias.grad,
                "dbias": m.conv.bias.grad if bias else None}

    for what, o in _variants(run, s.x.to(dev), s.cotangent[0].to(dev), dev).items():
        parity_gate(o["y"], want["y"], 1e-4, f"{what} forward")
        for k in ("dW", "dgamma", "dbeta", "dx"):
            grad_gate(o[k], want[k], 1e-4, f"{what} {k}")
        if bias:       # analytically zero behind a batch-statistics BatchNorm: rounding noise
            assert o["dbias"].abs().max().item() <= 1e-3 * want["dbeta"].abs().max().item(), f"{what} dbias"


@pytest.mark.parametrize("N,cin,cout,T,V,frozen", [(3, 256, 256, 10, 46, False), (2, 131, 128, 12, 22, True)],
                         ids=["3x256x256x10x46-mask", "2x131x128x12x22-frozen"])
def test_gcn_unit_attention_trains_on_operands_off_16_bytes(N, cin, cout, T, V, frozen, dev):
    """Deterministic: bit-equal to the aligned step in every variant, the drop-connect mask from the same seed."""
    sd = R.make_state(cin, cout, V, 21 if frozen else 11)
    xd = R.make_input(N, cin, T, V, 22 if frozen else 12).to(dev)
    dyd = torch.randn(N, cout, T, V, generator=torch.Generator().manual_seed(23 if frozen else 13)).to(dev)

    def run(x, dy, rebase):
        m = ep.st_unit(cin, cout, V, sd).train(not frozen)
        if rebase:
            rebase_parameters(m, dev)
        torch.manual_seed(99)
        y, dx = _step(m, x, dy, True)
        return {"y": y, "dx": dx, **{"d" + k: p.grad for k, p in m.named_parameters()},
                **{k: b.clone() for k, b in m.named_buffers() if b.dtype == torch.float32}}

    outs = _variants(run, xd, dyd, dev)
    for what, o in outs.items():
        same_bits(o, outs["aligned"], what)


@pytest.mark.parametrize("mode", ["f32", "mixed"])
@pytest.mark.parametrize("name", ["st_spatial_L22_D256", "st_temporal_L180_D512"])
def test_a_block_trains_on_operands_off_16_bytes(name, mode, dev):
    """The functional pair (vit_block_forward_train / vit_block_backward) and the Block module behind autograd: bit-equal."""
    from stgcn_amd.altformer import Block, set_hip_min_tokens, set_train_math
    blk = ar.build_block(Block, name).to(dev)
    xd, dyd = ar.make_input(name).to(dev), tr.make_dy(name).to(dev)

    def pair(x, dy):
        y, g = ep.run_block(blk, x, dy, mode)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    want = pair(xd, dyd)
    xs, dys = skewed(xd, 1), skewed(dyd, 1)
    same_bits(pair(xs, dyd), want, "x at 4 (mod 16)")
    same_bits(pair(xd, dys), want, "dy at 4 (mod 16)")
    checked(xs, dys)

    def run(x, dy, rebase):
        m = copy.deepcopy(blk).train()
        set_hip_min_tokens(m, 0)
        set_train_math(m, mode)
        if rebase:
            rebase_parameters(m, dev)
        assert m.trains_on_hip(x.detach().requires_grad_())
        y, dx = _step(m, x, dy, True)
        return {"y": y, "dx": dx, **{"d" + k: p.grad for k, p in m.named_parameters()}}

    outs = _variants(run, xd, dyd, dev)
    for what, o in outs.items():
        same_bits(o, outs["aligned"], what)
    assert torch.equal(outs["aligned"]["y"], want["y"]) and torch.equal(outs["aligned"]["dx"], want["dx"])


# ---- 4. modules whose parameters live in a flat buffer -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 37, 22, 128), (2, 23, 7, 128)], ids=["3x37x22x128", "2x23x7x128"])
def test_the_stem_modules_in_a_flat_buffer_give_the_aligned_bits_in_eval(shape, dev):
    """unit_agcn and Unit2D in eval mode, two-stage and fused: the parameters and running statistics are staged (folded,
    packed) from wherever they live, and ``x[1:]`` of a larger batch is read in place."""
    import stgcn_amd
    s = ep.stem(*shape)
    x = torch.cat([s.x[:1], s.x]).to(dev)[1:]
    outs = []
    for rebase in (False, True):
        gcn, tcn = copy.deepcopy(s.gcn), copy.deepcopy(s.tcn)          # fresh modules: nothing staged yet
        gcn.A = s.gcn.A
        gcn, tcn = gcn.to(dev).eval(), tcn.to(dev).eval()
        if rebase:
            rebase_parameters(gcn, dev), rebase_parameters(tcn, dev)
        with torch.no_grad():
            two = tcn(gcn(x))
            stgcn_amd.enable_stem_fusion(gcn, tcn)
            outs.append({"two_stage": two, "fused": tcn(gcn(x))})
    same_bits(outs[1], outs[0], "unit_agcn + Unit2D, parameters at 4 (mod 16)")
    parity_gate(outs[1]["fused"], s.reference(s.x)["out"], 1e-4, "fused stem in a flat buffer vs the fp64 oracle")


def _vit(dev, depth=2):
    from stgcn_amd import set_hip_min_tokens
    from stgcn_amd.vit import ViT
    torch.manual_seed(sr.MODEL_SEED)
    model = sr.prepare(ViT(**dict(sr.CONFIG, depth=depth), dropout=0.1, emb_dropout=0.0)).to(dev)
    set_hip_min_tokens(model, 0)
    return model


@pytest.mark.parametrize("layout", ["nctv", "ntvc"])
def test_a_vit_in_a_flat_buffer_runs_on_hip_with_the_aligned_bits(layout, dev):
    """The patch embedding's weight and the classifier's weight are listed operands: the module copies them, and ``uses_hip``
    stays true.  The input one element off as well (z is listed too)."""
    model = _vit(dev).eval()
    z = sr.make_input().to(dev)
    if layout == "ntvc":
        z = z.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    with torch.no_grad():
        assert model.uses_hip(z)
        want = model(z)
        rebase_parameters(model, dev)
        assert model.to_patch_embedding[1].weight.data_ptr() % 16 == 4 and model.mlp_head[1].weight.data_ptr() % 16 == 4
        assert model.uses_hip(z) and model.embed_on_hip(z)
        assert torch.equal(model(z), want), "parameters at 4 (mod 16)"
        zs = skewed(z, 1)
        assert model.uses_hip(zs)
        assert torch.equal(model(zs), want), "parameters and z at 4 (mod 16)"
        checked(zs)


def test_a_vit_in_a_flat_buffer_trains_on_hip_with_the_aligned_bits(dev):
    """Both ends and every layer on the HIP training kernels, the layers' dropout masks drawn from the same seed (with them
    the cotangent of the block backward is a listed operand): logits, dz and every gradient equal the aligned model's."""
    from stgcn_amd import set_hip_train_min_tokens
    z0 = sr.make_input().to(dev)
    dlogits = torch.randn(sr.CLIPS + 1, sr.CONFIG["num_classes"], generator=torch.Generator().manual_seed(8)).to(dev)

    def run(rebase, z, dl):
        model = _vit(dev).train()
        set_hip_train_min_tokens(model, 0)
        if rebase:
            rebase_parameters(model, dev)
        zg = z.detach().requires_grad_(True)
        assert model.embed_trains_on_hip(zg) and model.trains_on_hip(zg)
        torch.manual_seed(77)
        x = model.embed(zg)
        assert model.head_trains_on_hip(x)
        logits = model.classify(model.transformer(x))
        logits.backward(dl)
        assert all(p.grad is not None for p in model.parameters())
        return {"logits": logits.detach(), "dz": zg.grad, **{"d" + k: p.grad for k, p in model.named_parameters()}}

    want = run(False, z0, dlogits[1:].clone())
    same_bits(run(True, z0, dlogits[1:].clone()), want, "parameters at 4 (mod 16)")
    zs = skewed(z0, 1)
    assert dlogits[1:].data_ptr() % 16 == 8
    same_bits(run(True, zs, dlogits[1:]), want, "parameters and z at 4 (mod 16), dlogits a slice at 8 (mod 16)")
    checked(zs)


def _head_input(dev):
    return torch.relu(torch.randn(3, 128, 40, 22, generator=torch.Generator().manual_seed(4))).to(dev)


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_an_altformer_head_in_a_flat_buffer_runs_whole_with_the_aligned_bits(cls_name, dev):
    """The one-call head: ``head.weight`` is its listed operand, the module copies it, ``runs_whole`` stays true."""
    import stgcn_amd
    head = ep.small_head(dev, cls_name)
    stgcn_amd.set_whole_head(head)
    z = _head_input(dev)
    with torch.no_grad():
        assert head.runs_whole(z)
        want = head(z)
        rebase_parameters(head, dev)
        assert head.mlp_head[1].weight.data_ptr() % 16 == 4 and head.runs_whole(z)
        assert torch.equal(head(z), want), "parameters at 4 (mod 16)"
        zs = skewed(z, 1)
        assert head.runs_whole(zs)
        assert torch.equal(head(zs), want), "parameters and z at 4 (mod 16)"
        checked(zs)


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_an_altformer_head_in_a_flat_buffer_runs_its_blocks_on_hip_with_the_aligned_bits(cls_name, dev):
    """The per-block forward.  Its HIP parts - the first embedding and every block - give the aligned bits: the first stage as
    a whole (nothing but HIP calls), and every block of the second stage on the input the aligned head gave it.  Between the
    stages the head runs torch's own linear, whose kernel choice may follow the weight's address, so the logits are held to
    the gate of test_two_runs_are_bit_identical_and_match_the_torch_path instead: the module's torch path, 1e-4."""
    from stgcn_amd.altformer import Block
    head = ep.small_head(dev, cls_name)
    z = _head_input(dev)
    order, lin1, pos1, blocks1, lin2, pos2, blocks2 = head._stages()
    seen = {}
    hooks = [b.register_forward_hook(lambda mod, args, out, i=i: seen.__setitem__(i, (mod.uses_hip(args[0]), args[0].clone(), out.clone())))
             for i, b in enumerate(blocks2)]
    with torch.no_grad():
        want1 = head._first_stage(z, lin1, pos1, blocks1, order)
        want = head(z)
        aligned = dict(seen)
        assert len(aligned) == len(blocks2) and all(v[0] for v in aligned.values())
        rebase_parameters(head, dev)
        assert all(b.uses_hip(want1) for b in blocks1)
        assert torch.equal(head._first_stage(z, lin1, pos1, blocks1, order), want1), "first stage, parameters at 4 (mod 16)"
        zs = skewed(z, 1)
        assert torch.equal(head._first_stage(zs, lin1, pos1, blocks1, order), want1), "first stage, parameters and z at 4 (mod 16)"
        checked(zs)
        for i, b in enumerate(blocks2):
            used, x, y = aligned[i]
            xs = skewed(x, 1)
            assert b.uses_hip(x) and torch.equal(b(x), y) and torch.equal(b(xs), y), f"second stage, block {i}"
            checked(xs)
        for h in hooks:
            h.remove()
        got = head(z)
        for m in head.modules():
            if isinstance(m, Block):
                m.force_torch = True
        torch_path = head(z)
    parity_gate(got, torch_path, 1e-4, f"{cls_name} in a flat buffer: HIP path vs the module's torch path")
    parity_gate(want, torch_path, 1e-4, f"{cls_name} aligned: HIP path vs the module's torch path")


@pytest.mark.parametrize("N,cin,cout,T,V", [(2, 131, 128, 12, 22), (2, 256, 512, 3, 46)])
def test_gcn_unit_attention_in_a_flat_buffer_gives_the_aligned_bits_in_eval(N, cin, cout, T, V, dev):
    m = ep.st_unit(cin, cout, V, R.make_state(cin, cout, V, 7)).eval()
    x = R.make_input(N, cin, T, V, 8).to(dev)
    with torch.no_grad():
        want = m(x)
        m2 = ep.st_unit(cin, cout, V, R.make_state(cin, cout, V, 7)).eval()
        rebase_parameters(m2, dev)
        assert torch.equal(m2(x), want)


def test_wx_product_takes_its_unaligned_weight_form_and_gives_the_aligned_bits(dev):
    """stgcn_wx_product picks W's staging form from W's address: with K % 4 == 0 the 16-byte form needs a 16-byte W, and a W
    in a flat buffer takes the element-wise form.  Same values staged, same summation order: same bits."""
    F = _F()
    g = torch.Generator().manual_seed(12)
    for M, K, TV in ((96, 64, 300), (33, 128, 77)):
        W, X = (torch.randn(M, K, generator=g) / K ** 0.5).to(dev), torch.randn(2, K, TV, generator=g).to(dev)
        bias, Rr = torch.randn(M, generator=g).to(dev), torch.randn(2, M, TV, generator=g).to(dev)
        for math in (F.MATH_F32, F.MATH_BF16X3):
            if not F.wx_product_supported(M, K, TV, math):
                continue
            want = F.wx_product(W, X, bias, Rr, math=math)
            parity_gate(want, torch.einsum("mk,nkt->nmt", W.double(), X.double()).cpu() + bias.double().cpu()[None, :, None] + Rr.double().cpu(),
                        1e-4, f"wx_product {M}x{K}x{TV}")
            ops = [skewed(t, 1) for t in (W, X, bias, Rr)]
            assert torch.equal(F.wx_product(*ops, math=math), want), f"{M}x{K}x{TV} math {math}: every operand at 4 (mod 16)"
            checked(*ops)


def test_the_bf16_operands_of_the_heads_are_served_one_element_off(dev):
    """bf16 storage at 2 (mod 4) bytes: x and y of ``vit_linear_bf16``, qkv of ``vit_attention_bf16`` - read and written at
    lane-dependent addresses, 8 and 16 bytes at a time."""
    from stgcn_amd import _capi
    F = _F()
    g = torch.Generator().manual_seed(31)
    M, K, Nout = 129, 256, 256
    assert _capi.lib().stgcn_vit_linear_bf16_supported(M, K, Nout, 0) and F.vit_attention_bf16_supported(65, 8, 32)
    x = torch.randn(M, K, generator=g).bfloat16().to(dev)
    W, b = (torch.randn(Nout, K, generator=g) / 16).to(dev), torch.randn(Nout, generator=g).to(dev)
    want = F.vit_linear_bf16(x, W, b, gelu=True, y_bf16=True)
    xs, ys, Ws, bs = skewed(x, 1), skewed(torch.zeros_like(want), 1), skewed(W, 1), skewed(b, 1)
    assert xs.data_ptr() % 4 == 2 and ys.data_ptr() % 4 == 2
    got = F.vit_linear_bf16(xs, Ws, bs, gelu=True, y=ys)
    checked(xs, ys, Ws, bs)
    assert got.data_ptr() == ys.data_ptr() and torch.equal(got, want)
    qkv = ep.peaked_qkv(3, 65, 8, 32, 7).bfloat16().to(dev)
    want = F.vit_attention_bf16(qkv, 8)
    qs = skewed(qkv, 1)
    assert qs.data_ptr() % 4 == 2
    got = F.vit_attention_bf16(qs, 8)
    checked(qs)
    assert torch.equal(got, want)


# ---- 5. the exceptions are refused by name, before anything is written ---------------------------------------------------------------
def _refused(call_skewed, call_aligned, name, dev):
    with hostile_allocations(0xFF) as h:
        with pytest.raises(ValueError, match=rf"^{re.escape(name)} must be \d+-byte aligned"):
            call_skewed()
        torch.cuda.synchronize()
        h.check()
        for i, (raw, nbytes, shape, dtype) in enumerate(h.records):
            assert bool((raw == h.fill).all()), f"allocation #{i} (shape {shape}, {dtype}) was written by a refused call"
    out = call_aligned()
    torch.cuda.synchronize()
    return out


def refuse_stem(operand, dev):
    from stgcn_amd import _capi
    staged, xd = _stem((3, 37, 22, 128), dev)
    F = _F()
    mode = F.MATH_BF16X3
    prep = staged.prepare(mode)
    need = _capi.lib().stgcn_stem_ws_bytes(3, 3, 128, 37, 22, 9, 3, F._flags(mode, False))
    ws = torch.empty((need + 3) // 4, device=dev)
    bad = {"ws": dict(ws=skewed(ws, 1)), "prep": {}}[operand]
    bad_prep = skewed(prep, 4) if operand == "prep" else prep
    return (lambda: _stem_call(staged, xd, bad_prep, mode, 128, **bad)), (lambda: _stem_call(staged, xd, prep, mode, 128, ws=ws))


def refuse_tcn_packed(operand, dev):
    F = _F()
    s = ep.tcn(32, 128, 9, 1, 23, 22, 2, "bf16x3", False, False)
    from stgcn_amd import Unit2D
    torch.manual_seed(3)
    st = Unit2D(32, 128, kernel_size=9).to(dev).eval()._staged(dev)
    Wp = F.tcn_pack(st["W"], st["scale"], F.MATH_BF16X3)
    xd, bad = s.x.to(dev), skewed(Wp, 16)          # (made here: the refused call runs under the hostile allocator)
    return (lambda: F.tcn_forward_packed(xd, bad, st["shift"], 128, 9, 1, F.MATH_BF16X3)), \
        (lambda: F.tcn_forward_packed(xd, Wp, st["shift"], 128, 9, 1, F.MATH_BF16X3))


def refuse_vit_patch_embed(operand, dev):
    F = _F()
    z, W, bias, cls, pos = (t.to(dev) for t in sr.embed_case("a_K256_rows18"))
    ops = {"z": z, "weight": W}
    ops[operand] = skewed(ops[operand], 1)
    return (lambda: F.vit_patch_embed(ops["z"], ops["weight"], bias, cls, pos, 4, 2)), (lambda: F.vit_patch_embed(z, W, bias, cls, pos, 4, 2))


def refuse_vit_patch_embed_backward(operand, dev):
    F = _F()
    z, W, bias, cls, pos = (t.to(dev) for t in sr.embed_case("a_K256_rows18"))
    dx = torch.randn(3, 7, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    ops = {"z": z, "weight": W, "dx": dx}
    ops[operand] = skewed(ops[operand], 1)
    return (lambda: F.vit_patch_embed_backward(ops["z"], ops["weight"], ops["dx"], 4, 2)), (lambda: F.vit_patch_embed_backward(z, W, dx, 4, 2))


def _classify_ops(dev):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 9, 128, generator=g).to(dev)
    return x, (1 + 0.2 * torch.randn(128, generator=g)).to(dev), torch.randn(128, generator=g).to(dev), \
        (torch.randn(14, 128, generator=g) / 11).to(dev), torch.randn(14, generator=g).to(dev), torch.randn(3, 14, generator=g).to(dev)


def refuse_vit_pool(operand, dev):
    F = _F()
    x = _classify_ops(dev)[0]
    bad = skewed(x, 1)
    return (lambda: F.vit_pool(bad, "mean")), (lambda: F.vit_pool(x, "mean"))


def refuse_vit_pool_classify(operand, dev):
    F = _F()
    x, lw, lb, W, b, _ = _classify_ops(dev)
    ops = {"x": x, "weight": W}
    ops[operand] = skewed(ops[operand], 1)
    return (lambda: F.vit_pool_classify(ops["x"], lw, lb, 1e-5, ops["weight"], b, mode="cls")), \
        (lambda: F.vit_pool_classify(x, lw, lb, 1e-5, W, b, mode="cls"))


def refuse_vit_pool_classify_backward(operand, dev):
    F = _F()
    x, lw, lb, W, b, dl = _classify_ops(dev)
    bad = skewed(x, 1)
    return (lambda: F.vit_pool_classify_backward(bad, lw, lb, 1e-5, W, dl, mode="cls")), \
        (lambda: F.vit_pool_classify_backward(x, lw, lb, 1e-5, W, dl, mode="cls"))


def refuse_block_backward_drop(operand, dev):
    F = _F()
    x, sd = ep.block_inputs(3, 22, 256, 512)
    xd, flat = x.to(dev), [t for pair in ep.block_params(sd, dev) for t in pair]
    g = torch.Generator().manual_seed(9)
    masks = {"m_proj": (torch.rand(3, 22, 256, generator=g) > 0.1).float().to(dev) / 0.9, "m_act": None,
             "m_fc2": (torch.rand(3, 22, 256, generator=g) > 0.1).float().to(dev) / 0.9}
    dy = torch.randn(3, 22, 256, generator=g).to(dev)
    args = (8, ar.EPS, 32 ** -0.5, F.MATH_F32)
    drop = tuple(masks.values())
    y, saved = F.vit_block_forward_train(xd, flat, *args, drop=drop)
    ops = dict(masks, dy=dy)
    ops[operand] = skewed(ops[operand], 1)
    bad_drop = (ops["m_proj"], None, ops["m_fc2"])
    return (lambda: F.vit_block_backward(xd, flat, saved, ops["dy"], *args, drop=bad_drop)), \
        (lambda: F.vit_block_backward(xd, flat, saved, dy, *args, drop=drop))


def refuse_head(operand, dev):
    head = ep.small_head(dev, "ST")
    import stgcn_amd
    stgcn_amd.set_whole_head(head)
    z = _head_input(dev)
    with torch.no_grad():
        plan = head._whole_plan(z)
    assert plan is not None
    w, b = plan["head_linear"]
    bad = dict(plan, head_linear=(skewed(w.detach(), 1), b))
    F = _F()

    def good():
        with torch.no_grad():
            return F.altformer_head_forward(z, **plan)

    def refused():
        with torch.no_grad():
            return F.altformer_head_forward(z, **bad)
    return refused, good


REFUSALS = [("stem_forward", "ws", refuse_stem), ("stem_forward", "prep", refuse_stem), ("tcn_forward_packed", "Wp", refuse_tcn_packed),
            ("vit_patch_embed", "z", refuse_vit_patch_embed), ("vit_patch_embed", "weight", refuse_vit_patch_embed),
            ("vit_patch_embed_backward", "z", refuse_vit_patch_embed_backward),
            ("vit_patch_embed_backward", "weight", refuse_vit_patch_embed_backward),
            ("vit_patch_embed_backward", "dx", refuse_vit_patch_embed_backward),
            ("vit_pool", "x", refuse_vit_pool), ("vit_pool_classify", "x", refuse_vit_pool_classify),
            ("vit_pool_classify", "weight", refuse_vit_pool_classify), ("vit_pool_classify_backward", "x", refuse_vit_pool_classify_backward),
            ("vit_block_backward", "m_proj", refuse_block_backward_drop), ("vit_block_backward", "m_fc2", refuse_block_backward_drop),
            ("vit_block_backward", "dy", refuse_block_backward_drop), ("altformer_head_forward", "head.weight", refuse_head)]


@pytest.mark.parametrize("entry,operand,make", REFUSALS, ids=[f"{e}-{o}" for e, o, _ in REFUSALS])
def test_a_listed_operand_off_its_demand_is_refused_by_name_and_the_next_call_succeeds(entry, operand, make, dev):
    bad, good = make(operand, dev)
    want = good()
    torch.cuda.synchronize()
    got = _refused(bad, good, operand, dev)
    flat = lambda o: list(o.values()) if isinstance(o, dict) else list(o) if isinstance(o, (tuple, list)) else [o]      # noqa: E731
    for a, b in zip(flat(got), flat(want)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"{entry}: the call after the refusal differs"
