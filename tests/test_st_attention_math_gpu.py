"""GPU tests of gcn_unit_attention's 'bf16x3' arithmetic (opt-in): the product kernel of csrc/wx_bf16.hip on its own through
stgcn_wx_product, and the whole unit through the module after set_st_attention_math(m, 'bf16x3').  The inputs, the three-term
emulation and the bounds are tests/st_attention_math_ref.py's; tests/test_st_attention_math_host.py asserts that the arithmetic
itself holds every gate used here with room, on these inputs.

Product: (1) |C - emu3| <= terms * 2^-24 * S elementwise (terms = 3K, plus one per epilogue addend, which also joins S: the
rounding of an fp32 sum of exact products, in whatever order); (2) rms(C - emu3) <= rms(C - exact64) / 4 - the flag is not
ignored; (3) the f32 call of the same entry point gives the reverse and other bits; parity_gate 1e-4 against the fp64 product;
two runs bit-identical.  Unit: y strict, gradients and dx under st_attention_train_gate (1e-4 of max|fp64|), running statistics
under parity_gate, a second identical step bit-identical.

Measured on the MI355X (fractions of max|fp64|; the emulation's own figures are in the host file's output):

    product          rms to emu3   rms to exact   of the elementwise bound
    ragged_k131      9.5e-08       3.7e-06        0.006
    ragged_m131_t    1.1e-07       3.7e-06        0.003
    skip             9.5e-08       3.7e-06        0.008
    wide_768x512     1.9e-07       3.6e-06        0.002
    tiny             2.3e-08       3.9e-06        0.116
    many_columns     1.3e-07       3.6e-06        0.004

    unit case          y        dx       worst parameter gradient
    ragged_k131_tv75   1.0e-05  7.7e-06  1.3e-05 attention_conv.qkv_conv.bias
    skip_tv110         4.1e-06  8.7e-06  9.1e-06 data_bn.weight
    k131_c256_tv264    8.5e-06  1.0e-05  1.1e-05 data_bn.weight
    c512_v46           9.8e-06  1.2e-05  1.2e-05 data_bn.bias
    skip512_tv92       3.6e-06  1.9e-05  1.4e-05 data_bn.bias
    eval_skip_c256     3.1e-06  (eval forward only)
    eval_k131_tv75     8.4e-06  (eval forward only)
    frozen_mask        7.8e-06  9.9e-06  1.3e-05 data_bn.weight
"""
import functools

import pytest
import torch

import st_attention_math_ref as MR
import st_attention_ref as R
from _util import ZERO_GRAD, HostileCase, hostile_allocations, parity_gate, run_under_both_fills, st_attention_train_gate
from entry_points import st_unit

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F32, BF16X3, BF16, F32_VALU = 0, 1, 2, 3
TRAIN = [c["name"] for c in MR.UNIT_CASES if c["mode"] == "train"]
EVAL = [c["name"] for c in MR.UNIT_CASES if c["mode"] == "eval"]


def _up(t):
    return None if t is None else t.to(DEV)


# ---- the product alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in MR.PRODUCT_CASES])
def test_product_holds_bound_separation_and_gate(name):
    from stgcn_amd import functional as F
    ref = MR.product_reference(name)
    c = ref["case"]
    args = (_up(ref["W"]), _up(ref["X"]), _up(ref["bias"]), _up(ref["R"]))
    C = F.wx_product(*args, w_transposed=c["wt"], math=BF16X3)
    again = F.wx_product(*args, w_transposed=c["wt"], math=BF16X3)
    C32 = F.wx_product(*args, w_transposed=c["wt"], math=F32)
    torch.cuda.synchronize()
    assert C.shape == (c["N"], c["M"], c["TV"])
    Cd, C32d = C.double().cpu(), C32.double().cpu()
    over = (Cd - ref["emu3"]).abs() - ref["bound"]
    near, far = MR.rms(Cd - ref["emu3"]), MR.rms(Cd - ref["exact64"])
    near32, far32 = MR.rms(C32d - ref["exact64"]), MR.rms(C32d - ref["emu3"])
    used = float(((Cd - ref["emu3"]).abs() / ref["bound"].clamp_min(1e-300)).max())
    print(f"FIGURES {name}: bf16x3 rms to emu3 {near:.2e}, to exact {far:.2e} ({far / max(near, 1e-300):.0f} x), "
          f"{used:.3f} of the elementwise bound; f32 rms to exact {near32:.2e}, to emu3 {far32:.2e}")
    assert torch.isfinite(C).all()
    assert float(over.max()) <= 0, f"{name}: {float(over.max()):.2e} over the elementwise bound ({used:.2f} of it)"
    assert near <= far / 4, f"{name}: bf16x3 is not the three-term arithmetic (rms {near:.2e} to emu3, {far:.2e} to exact)"
    assert near32 <= far32 / 4, f"{name}: the f32 call is not exact fp32 (rms {near32:.2e} to exact, {far32:.2e} to emu3)"
    assert not torch.equal(C, C32), f"{name}: the two arithmetics gave the same bits"
    assert torch.equal(C, again), f"{name}: two bf16x3 runs differ"
    parity_gate(C, ref["exact64"], rel=1e-4, what=f"{name} bf16x3 vs fp64")
    parity_gate(C32, ref["exact64"], rel=1e-4, what=f"{name} f32 vs fp64")


# ---- the whole unit ----------------------------------------------------------------------------------------------------------------------
def _module(c, sd, math="bf16x3"):
    from stgcn_amd import set_st_attention_math
    m = st_unit(c["cin"], c["cout"], c["V"], sd, drop_connect=c["drop"])
    m.train(c["mode"] != "eval")
    if c["mode"] == "frozen":
        m.data_bn.eval()
        m.bn.eval()
    set_st_attention_math(m, math)
    return m


def _step(m, sd, x, dyd, mask):
    """One forward and backward from the state ``sd`` with the recorded drop-connect mask."""
    m.load_state_dict(sd)
    for p in m.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    orig = torch.bernoulli
    if mask is not None:
        def bern(p, *a, **k):
            torch.bernoulli = orig
            assert p.numel() == mask.numel()
            return mask.to(p.device, p.dtype)
        torch.bernoulli = bern
    try:
        y = m(xd)
        assert torch.bernoulli is orig, "the drop-connect mask was not drawn"
    finally:
        torch.bernoulli = orig
    y.backward(dyd)
    return {"y": y.detach(), "dx": xd.grad, **{"d" + k: p.grad for k, p in m.named_parameters()}}


def _eval(m, x):
    with torch.no_grad():
        return m(x)


@pytest.mark.parametrize("name", TRAIN)
def test_training_step_vs_fp64(name):
    c, sd, x, dy, mask, (yr, new, g, dx) = MR.unit_reference(name)
    m = _module(c, sd)
    dyd = dy.to(DEV)
    o = _step(m, sd, x, dyd, mask)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    refs = {"y": yr, "dx": dx, **{"d" + k: v for k, v in g.items()}}
    fig = {k: float((o[k].double().cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-30) for k, r in refs.items()}
    worst = max((k for k in fig if k not in ("y", "dx") and k[1:] not in ZERO_GRAD), key=fig.get)
    print(f"FIGURES {name}: y {fig['y']:.2e} dx {fig['dx']:.2e} worst grad {fig[worst]:.2e} ({worst[1:]})")
    st_attention_train_gate(yr, g, dx, False)(o, name)
    for pre in ("data_bn.", "bn."):
        for k in ("running_mean", "running_var"):
            parity_gate(state[pre + k], new[pre + k], what=f"{name} {pre + k}")
        assert int(state[pre + "num_batches_tracked"]) == int(sd[pre + "num_batches_tracked"]) + 1
    o2 = _step(m, sd, x, dyd, mask)
    for k in o:
        assert torch.equal(o[k], o2[k]), f"{name}: {k} differs in a second identical step"


@pytest.mark.parametrize("name", EVAL)
def test_eval_forward_vs_fp64(name):
    c, sd, x, _, _, (yr, *_rest) = MR.unit_reference(name)
    m = _module(c, sd)
    xd = x.to(DEV)
    y = _eval(m, xd)
    r = parity_gate(y, yr, what=f"{name} eval y")
    print(f"FIGURES {name}: y {r:.2e} (eval forward)")
    assert torch.equal(_eval(m, xd), y), f"{name}: a second identical forward differs"


def test_frozen_statistics_with_drop_connect_under_bf16x3():
    """``frozen_mask`` of st_attention_ref.EDGE_CASES: STGCN_BN_FROZEN and the arithmetic bits in one flag word.  State, input
    and mask are the case's; the cotangent is its kink-free form (st_attention_math_ref.frozen_reference: with the plain one
    the fp64 emulation of the arithmetic is itself 5e-3 off, one ReLU flip)."""
    c, sd, x, dy, mask, (yr, _, g, dx) = MR.frozen_reference()
    m = _module(c, sd)
    assert m.attention_conv.training and not m.bn.training and not m.data_bn.training
    o = _step(m, sd, x, dy.to(DEV), mask)
    refs = {"y": yr, "dx": dx, **{"d" + k: v for k, v in g.items()}}
    fig = {k: float((o[k].double().cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-30) for k, r in refs.items()}
    print("FIGURES frozen_mask: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    st_attention_train_gate(yr, g, dx, True)(o, "frozen_mask")
    for k, v in m.state_dict().items():
        if "running" in k or "num_batches" in k:
            assert torch.equal(v.cpu(), sd[k]), f"{k} changed under frozen statistics"


def test_bf16x3_differs_from_f32_and_switching_back_restores_the_bits():
    from stgcn_amd import set_st_attention_math
    c, sd, x, dy, mask, _ = MR.unit_reference("skip_tv110")
    m = _module(c, sd, "f32")
    dyd = dy.to(DEV)
    f32 = _step(m, sd, x, dyd, mask)
    set_st_attention_math(m, "bf16x3")
    b3 = _step(m, sd, x, dyd, mask)
    assert not torch.equal(b3["y"], f32["y"]), "bf16x3 gave the f32 bits: the setting does not reach the kernels"
    assert not torch.equal(b3["dx"], f32["dx"])
    set_st_attention_math(m, "f32")
    back = _step(m, sd, x, dyd, mask)
    for k in f32:
        assert torch.equal(back[k], f32[k]), f"{k}: 'f32' after 'bf16x3' does not reproduce the f32 bits"
    m.eval()
    xd = x.to(DEV)
    e32 = _eval(m, xd)
    set_st_attention_math(m, "bf16x3")
    assert not torch.equal(_eval(m, xd), e32)
    set_st_attention_math(m, "f32")
    assert torch.equal(_eval(m, xd), e32)


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------------
def _make_eval(name, dev):
    c, sd, x, _, _, (yr, *_rest) = MR.unit_reference(name)
    m = _module(c, sd)
    xd = x.to(dev)
    return (lambda: {"y": _eval(m, xd)}), (lambda o, what: parity_gate(o["y"], yr, what=f"{what} y"))


def _make_train(name, dev):
    c, sd, x, dy, mask, (yr, _, g, dx) = MR.unit_reference(name)
    m = _module(c, sd)
    dyd = dy.to(dev)
    return (lambda: _step(m, sd, x, dyd, mask)), st_attention_train_gate(yr, g, dx, False)


def test_eval_forward_under_poisoned_guarded_buffers():
    """Outputs and workspaces pre-filled with NaN, then 3.4e38, between guard bands: a staged tail that was loaded instead of
    zeroed, or a store past a ragged tile, shows as a non-finite result or a trampled guard; the two runs agree bit for bit."""
    run_under_both_fills(HostileCase("st_attention_math_eval-eval_k131_tv75", functools.partial(_make_eval, "eval_k131_tv75"), True), DEV)


def test_training_step_under_poisoned_guarded_buffers():
    run_under_both_fills(HostileCase("st_attention_math_train-skip_tv110", functools.partial(_make_train, "skip_tv110"), False), DEV)


# ---- non-finite ------------------------------------------------------------------------------------------------------------------------------
def test_nan_in_the_last_element_stays_in_its_clip_and_reaches_its_outputs():
    name = "eval_k131_tv75"
    c, sd, x, *_ = MR.unit_reference(name)
    assert x.shape == (2, 131, 3, 25)
    m = _module(c, sd)
    clean = _eval(m, x.to(DEV))
    bad = x.clone()
    bad[1, 130, 2, 24] = float("nan")                 # last channel, last pixel of clip 1: the K tail and the column tail
    y = _eval(m, bad.to(DEV))
    assert torch.isfinite(clean).all()
    assert torch.equal(y[0], clean[0]), "a NaN in clip 1 changed clip 0"
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    ref, _ = R.forward64(sd64, bad.double(), False)
    want = torch.isnan(ref[1])
    assert bool(want.any()) and not bool(want.all())
    assert bool(torch.isnan(y[1].cpu())[want].all()), "an output the fp64 reference makes NaN is not NaN"
    assert torch.equal(y[1].cpu()[~want], clean[1].cpu()[~want]), "an output outside the NaN's reach changed"


def test_nan_behind_the_end_of_x_is_never_read():
    """x in a buffer whose bytes behind its end hold NaN (hostile fill 0xFF): clean input, clean and unchanged result."""
    name = "eval_k131_tv75"
    c, sd, x, _, _, (yr, *_rest) = MR.unit_reference(name)
    m = _module(c, sd)
    clean = _eval(m, x.to(DEV))
    with hostile_allocations(0xFF) as h:
        xd = torch.empty(x.shape, dtype=torch.float32, device=DEV)
        assert h.records
    xd.copy_(x)
    y = _eval(m, xd)
    torch.cuda.synchronize()
    h.check()
    assert torch.isfinite(y).all()
    assert torch.equal(y, clean)
    parity_gate(y, yr, what=f"{name} y behind a NaN guard")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math,word", [(BF16, "STGCN_MATH_BF16"), (F32_VALU, "STGCN_MATH_F32_VALU")])
def test_other_arithmetics_are_refused_by_name(math, word):
    from stgcn_amd import _capi, functional as F
    c, sd, x, dy, mask, _ = MR.unit_reference("skip_tv110")
    m = _module(c, sd, "f32")
    st = m._staged(DEV)
    xd, dbn, bn = x.to(DEV), m.data_bn, m.bn
    folded = m._folded(st)

    def refused(fn):
        with pytest.raises(_capi.StgcnError, match="STGCN_ERR_UNSUPPORTED") as e:
            fn()
        assert e.value.code == -2
        assert word in str(e.value) and word in _capi.lib().stgcn_last_error().decode()

    refused(lambda: F.st_attention_forward(xd, folded[0], folded[1], st["Wqkv"], st["bqkv"], st["Wout"], st["bout"], folded[2],
                                           folded[3], m._dk, m._heads, math=math))
    train = lambda mm: F.st_attention_forward_train(                                                      # noqa: E731
        xd, (dbn.weight.detach(), dbn.bias.detach(), dbn.running_mean.clone(), dbn.running_var.clone()), st["Wqkv"], st["bqkv"],
        st["Wout"], st["bout"], (bn.weight.detach(), bn.bias.detach(), bn.running_mean.clone(), bn.running_var.clone()),
        mask.to(DEV), m._dk, m._heads, 0.1, bn.eps, math=mm)
    refused(lambda: train(math))
    _, sv = train(F32)
    refused(lambda: F.st_attention_backward(xd, dbn.weight.detach(), dbn.bias.detach(), st["Wqkv"], st["Wout"], bn.weight.detach(),
                                            bn.bias.detach(), mask.to(DEV), sv, dy.to(DEV), m._dk, m._heads, math=math))
    refused(lambda: F.wx_product(st["Wout"], xd.reshape(2, 128, -1), math=math))
    assert not F.st_attention_math_supported(c["cin"], c["cout"], m._dk, c["V"], m._heads, math)
    assert F.st_attention_math_supported(c["cin"], c["cout"], m._dk, c["V"], m._heads, BF16X3)
