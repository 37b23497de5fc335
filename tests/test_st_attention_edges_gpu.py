"""GPU tests of the HIP gcn_unit_attention (ST-TR spatial attention) at the edges of what its kernels cover, against the fp64
restatement in tests/st_attention_ref.py.  The cases are st_attention_ref.EDGE_CASES; tests/test_st_attention_edges_host.py
asserts that they are well conditioned (plain fp32 within 2.5e-5 of fp64) and that each is the edge it is named for.

Gates: the project's own - parity_gate (1e-4 of max|fp64|, strict) for y and the running statistics, strict=False for
gradients, and the ZERO_GRAD rule for attn_out.bias behind a batch-statistics BatchNorm.

Measured on the MI355X: worst max|kernel - fp64| / max|fp64| per case (y, dx, worst parameter gradient), next to the worst figure
of the fp32 restatement on the CPU (test_st_attention_edges_host.py prints it):

    case          y        dx       worst parameter gradient             fp32 restatement (worst of all)
    v64_skip      3.1e-07  7.5e-07  6.7e-07 attn_out.weight              7.6e-07
    v1            2.9e-07  2.8e-07  6.4e-07 data_bn.bias                 6.8e-07
    v2_cin3       5.6e-07  4.9e-07  4.9e-07 data_bn.weight               6.1e-07
    v3_cin1       4.5e-07  3.1e-07  9.6e-07 data_bn.weight               1.1e-06
    n16           4.0e-07  4.7e-07  3.7e-07 data_bn.weight               6.4e-07
    n17           4.6e-07  4.3e-07  4.6e-07 qkv_conv.bias                5.5e-07
    n33           6.1e-07  5.5e-07  5.6e-07 qkv_conv.weight              6.9e-07
    chunks        4.5e-07  4.9e-07  1.4e-06 qkv_conv.bias                1.3e-06
    h4_c64        4.1e-07  4.7e-07  4.1e-07 bn.weight                    4.4e-07
    h16_c256      4.9e-07  5.3e-07  4.9e-07 data_bn.bias                 5.8e-07
    h1_c16        1.4e-07  3.5e-07  6.8e-07 qkv_conv.bias                5.4e-07
    h2_c128       3.7e-07  4.5e-07  4.8e-07 qkv_conv.bias                5.0e-07
    h16_c1024     1.0e-06  7.8e-07  9.8e-07 bn.weight                    1.0e-06
    h4_c128       3.1e-07  2.8e-07  5.0e-07 qkv_conv.bias                5.1e-07
    sharp         3.6e-06  1.0e-05  1.2e-05 qkv_conv.weight              8.2e-06
    sharp_mask    2.4e-06  8.0e-06  1.2e-05 qkv_conv.bias                8.8e-06
    frozen_mask   4.6e-07  6.8e-07  5.4e-07 data_bn.weight               6.6e-07
    eval_v1       5.0e-07  (eval forward only)                           9.1e-08 (y)
    eval_h1_v64   1.8e-07  (eval forward only)                           1.8e-07 (y)
    eval_v64      2.0e-07  (eval forward only)                           2.2e-07 (y)
    eval_tv3      5.0e-07  (eval forward only)                           5.7e-07 (y)

The sharp cases (603 of 2112 rows with a maximal logit above 88.8, logits -259 .. 297) sit at 1.2e-5, an eighth of the gate and
next to plain fp32's 8.8e-6: an fp32 logit of 300 carries an absolute rounding error of 3e-5, which the exponential turns into a
relative one.  No case needed the ReLU-kink treatment of its cotangent.
"""
import functools

import pytest
import torch

import st_attention_ref as R
from _util import parity_gate
from test_st_attention_gpu import ZERO_GRAD, _incidence, _mask_gen

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
BATCH = [c["name"] for c in R.EDGE_CASES if c["mode"] == "batch"]
EVAL = [c["name"] for c in R.EDGE_CASES if c["mode"] == "eval"]


def _module(cin, cout, V, nh, drop, sd=None, mode="batch"):
    from stgcn_amd import gcn_unit_attention
    m = gcn_unit_attention(cin, cout, _incidence(V), **dict(R.unit_kwargs(V, drop), Nh=nh))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.train(mode != "eval")
    if mode == "frozen":                            # model.train() then bn.eval() on both BatchNorms: frozen-BN fine-tuning
        m.data_bn.eval()
        m.bn.eval()
    return m


def _case_module(c, sd=None):
    return _module(c["cin"], c["cout"], c["V"], c["nh"], c["drop"], sd, c["mode"])


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Inputs and the fp64 result of a case, computed once and left unchanged."""
    c = R.edge_case(name)
    sd, x, dy, mask = R.edge_inputs(c)
    yr, new, g, dx = R.edge_grads(c)
    return c, sd, x, dy, mask, yr, new, g, dx


def _step(m, sd, xd, dyd, mask):
    """One forward and backward from the state ``sd`` with the recorded drop-connect mask; xd, dyd: device tensors (views
    allowed), xd.requires_grad decides whether dx is asked for."""
    m.load_state_dict(sd)
    for p in m.parameters():
        p.grad = None
    orig = torch.bernoulli
    if mask is not None:
        orig, torch.bernoulli = _mask_gen(mask)
    try:
        y = m(xd)
        assert mask is None or torch.bernoulli is orig, "the drop-connect mask was not drawn"
    finally:
        torch.bernoulli = orig
    y.backward(dyd)
    return {"y": y.detach(), "dx": xd.grad, **{"d" + k: p.grad for k, p in m.named_parameters()}}


def _fresh_x(x, need_dx=True):
    return x.to(DEV).requires_grad_(need_dx)


def _hold_to_fp64(name, o, m, frozen=False, dx_expected=True):
    """y, running statistics, num_batches_tracked, the eight parameter gradients and dx against grads64; prints the figures."""
    c, sd, x, dy, mask, yr, new, g, dx = _ref(name)
    fig = {"y": parity_gate(o["y"], yr, what=f"{name} y")}
    state = m.state_dict()
    for pre in ("data_bn.", "bn."):
        if frozen:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                assert torch.equal(state[pre + k].cpu(), sd[pre + k]), f"{name}: {pre + k} changed under frozen statistics"
        else:
            for k in ("running_mean", "running_var"):
                parity_gate(state[pre + k], new[pre + k], what=f"{name} {pre + k}")
            assert int(state[pre + "num_batches_tracked"]) == int(sd[pre + "num_batches_tracked"]) + 1
    assert len(g) == 8
    worst = ("", 0.0)
    for k in g:
        if k in ZERO_GRAD and not frozen:
            assert float(o["d" + k].abs().max()) <= 1e-4 * float(g["bn.bias"].abs().max()), f"{name} d{k}"
        else:
            r = parity_gate(o["d" + k], g[k], strict=False, what=f"{name} grad {k}")
            worst = max(worst, (k, r), key=lambda t: t[1])
    if dx_expected:
        fig["dx"] = parity_gate(o["dx"], dx, strict=False, what=f"{name} dx")
    print(f"FIGURES {name}: y {fig['y']:.2e} dx {fig.get('dx', float('nan')):.2e} worst grad {worst[1]:.2e} ({worst[0]})")
    return fig


# ---- batch statistics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BATCH)
def test_batch_statistics_step_vs_fp64(name):
    """One training step per edge:
    v64_skip: sta_fwd_kernel / sta_bwd_kernel with no idle lane (``lane < V``, ``if (j < V)`` at V = kVP = 64), skip connection.
    v1, v2_cin3, v3_cin1: almost all lanes idle, ``e / V`` and ``p % V`` at their extremes; (frame, head) blocks whose mask is all
      zero (``ss = 0``, ``rs = 1 / (0 + 1e-8)``, the backward's ``(dw - c) * rs * msk``); gemm_w_x / gemm_wgrad with K = Cin
      in {5, 3, 1} and T*V in {4, 10, 9}.
    n16, n17, n33: cv_splits(N) = 16 with per = ceil(N / 16) in cv_stats_kernel - exact, 7 empty splits, 5 empty splits (which
      must write zeros to ``parts``), in the statistics pass and the backward pass (``g != NULL``); n33 has T = 1.
    chunks: bn_chunks() = 2 in bn_batch_stats, bn_relu_bwd_stats, bn_relu_bwd_apply and bn_apply (9200 elements per channel,
      5 clips over 2 workgroups); run twice, the two runs within the fp32 gate of each other (its sums are fp64 atomics).
    h*: heads_supported's "any per-head split" at Nh in {1, 2, 4, 16}: grid.y, the head offsets ``h * DKH`` and
      ``2 * dk + h * DVH``, all three kernel instantiations.
    sharp, sharp_mask: the row maximum ``mx``, the saved (mx, l, ss) and ``__expf(a - mx)`` in the backward's recompute, at
      logits beyond fp32 exp's overflow."""
    c, sd, x, dy, mask, *_ = _ref(name)
    m = _case_module(c, sd)
    dyd = dy.to(DEV)
    o = _step(m, sd, _fresh_x(x), dyd, mask)
    _hold_to_fp64(name, o, m)
    if name == "chunks":
        o2 = _step(m, sd, _fresh_x(x), dyd, mask)
        for k in o:
            parity_gate(o2[k], o[k], strict=k == "y", what=f"chunks, second identical step: {k}")


# ---- frozen statistics with drop-connect ---------------------------------------------------------------------------------------------
def test_frozen_statistics_with_drop_connect():
    """``frozen`` with a mask: attention_conv.training draws the mask while both BatchNorms are in .eval() (STGCN_BN_FROZEN
    with ``mask != NULL`` in forward_train / backward); no buffer may change, num_batches_tracked included."""
    name = "frozen_mask"
    c, sd, x, dy, mask, *_ = _ref(name)
    m = _case_module(c, sd)
    assert m.attention_conv.training and not m.bn.training and not m.data_bn.training
    o = _step(m, sd, _fresh_x(x), dy.to(DEV), mask)
    _hold_to_fp64(name, o, m, frozen=True)


# ---- no input gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v64_skip", "n17"])
def test_parameter_gradients_without_an_input_gradient(name):
    """stgcn_st_attention_backward's ``dx == nullptr`` branch: parameter gradients against fp64 and bit-equal to the run that
    also asked for dx (same kernels in the same order; one BatchNorm chunk, so no atomics race)."""
    c, sd, x, dy, mask, *_ = _ref(name)
    m = _case_module(c, sd)
    dyd = dy.to(DEV)
    with_dx = _step(m, sd, _fresh_x(x), dyd, mask)
    xd = _fresh_x(x, need_dx=False)
    o = _step(m, sd, xd, dyd, mask)
    assert xd.grad is None and o["dx"] is None
    _hold_to_fp64(name, o, m, dx_expected=False)
    for k in o:
        if k != "dx":
            assert torch.equal(o[k], with_dx[k]), f"{name}: {k} differs from the run that also computed dx"


# ---- eval forward at the corners -------------------------------------------------------------------------------------------------------
def _eval_corner(name):
    c, sd, x, *_ = _ref(name)
    m = _case_module(c, sd)
    with torch.no_grad():
        y = m(x.to(DEV))
    ref, _ = R.forward64({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double(), False, nh=c["nh"])
    r = parity_gate(y, ref, what=f"{name} eval vs fp64")
    print(f"FIGURES {name}: y {r:.2e} (eval forward)")


@pytest.mark.parametrize("name", EVAL)
def test_eval_forward_at_the_corners(name):
    """stgcn_st_attention_forward at N*T = 1 with one joint (T*V = 1, K = 5), one head with a full wave (Nh = 1, V = 64, K = 1:
    ``grid.y`` = 1, no idle lane), V = 64 at the reference's widths, and gemm_w_x at T*V = 3 with K = 3."""
    _eval_corner(name)


# ---- views -------------------------------------------------------------------------------------------------------------------------------
def test_channels_last_input_and_strided_cotangent_give_the_same_bits():
    """forward's ``x.contiguous()`` and the backward's ``dy.contiguous()``: a channels-last view of x and a non-contiguous dy
    give the bits of the contiguous run."""
    c, sd, x, dy, mask, *_ = _ref("n17")
    m = _case_module(c, sd)
    plain = _step(m, sd, _fresh_x(x), dy.to(DEV), mask)
    xv = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    wide = torch.zeros(*dy.shape[:3], 2 * dy.shape[3], device=DEV)
    wide[..., ::2] = dy.to(DEV)
    dyv = wide[..., ::2]
    assert not xv.is_contiguous() and not dyv.is_contiguous()
    o = _step(m, sd, xv, dyv, mask)
    assert o["dx"].shape == x.shape
    for k in o:
        assert torch.equal(o[k], plain[k]), f"{k} differs between the views and the contiguous run"


# ---- N*T = 1 in training -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wants_dx", [False, True])
def test_one_value_per_channel_in_training_is_refused_like_the_reference(wants_dx):
    """Batch statistics of N*T = 1 value per channel: the reference's data_bn raises ValueError; bn_train_finalize_kernel would
    write running_var from a variance of 0.  Raised before the drop-connect draw, with every buffer unchanged."""
    c = R.edge_case("eval_v1")
    sd = R.make_state(c["cin"], c["cout"], c["V"], c["seed"])
    m = _module(c["cin"], c["cout"], c["V"], c["nh"], True, sd, "batch")
    x = R.make_input(1, c["cin"], 1, c["V"], c["seed"] + 1).to(DEV).requires_grad_(wants_dx)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    draws = []
    orig = torch.bernoulli
    torch.bernoulli = lambda *a, **k: draws.append(1) or orig(*a, **k)
    try:
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            m(x)
        with torch.no_grad(), pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            m(x)
    finally:
        torch.bernoulli = orig
    torch.cuda.synchronize()
    assert not draws, "torch.bernoulli was drawn before the refusal"
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed"
    assert int(m.bn.num_batches_tracked) == int(m.data_bn.num_batches_tracked) == 3
    _eval_corner("eval_v1")                         # eval with N*T = 1 keeps working


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
REFUSED = [("v65", 16, 128, 65, 8), ("widths_2_8", 16, 64, 9, 8), ("widths_6_24", 16, 192, 9, 8)]     # (cin, cout, V, Nh)
RUN_OFF_EIGHT = [(16, 128, 9, 4), (16, 64, 9, 4)]


@pytest.mark.parametrize("what,cin,cout,V,nh", REFUSED)
@pytest.mark.parametrize("mode", ["eval", "batch"])
def test_unsupported_shapes_are_refused_at_the_first_forward(what, cin, cout, V, nh, mode):
    """check_shape: V > kVP and per-head widths outside {(4,16), (8,32), (16,64)} raise StgcnError naming
    STGCN_ERR_UNSUPPORTED from every entry point, and stgcn_st_attention_supported says so; the next supported call on the
    device passes its gate."""
    from stgcn_amd import functional as F
    from stgcn_amd._capi import StgcnError
    assert not F.st_attention_supported(cin, cout, cout // 4, V, nh)
    m = _module(cin, cout, V, nh, True, R.make_state(cin, cout, V, 7), mode)
    x = R.make_input(2, cin, 3, V, 8).to(DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.set_grad_enabled(mode == "batch"), pytest.raises(StgcnError, match="STGCN_ERR_UNSUPPORTED") as e:
        m(x)
    assert e.value.code == -2
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed by a refused call"
    _eval_corner("eval_v64")


@pytest.mark.parametrize("cin,cout,V,nh", RUN_OFF_EIGHT)
def test_supported_widths_at_four_heads_run(cin, cout, V, nh):
    """(Cout 128, Nh 4) = (8,32) and (Cout 64, Nh 4) = (4,16) are served: eval forward against fp64."""
    from stgcn_amd import functional as F
    assert F.st_attention_supported(cin, cout, cout // 4, V, nh)
    sd = R.make_state(cin, cout, V, 9)
    x = R.make_input(2, cin, 3, V, 10)
    m = _module(cin, cout, V, nh, False, sd, "eval")
    with torch.no_grad():
        y = m(x.to(DEV))
    ref, _ = R.forward64({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double(), False, nh=nh)
    parity_gate(y, ref, what="eval vs fp64")


def test_supported_query_says_what_the_entry_points_do():
    """stgcn_st_attention_supported answers 1 exactly for the shapes that ran in this file and 0 for those refused."""
    from stgcn_amd import functional as F
    for c in R.EDGE_CASES:
        assert F.st_attention_supported(c["cin"], c["cout"], c["cout"] // 4, c["V"], c["nh"]), c["name"]
    for cin, cout, V, nh in RUN_OFF_EIGHT:
        assert F.st_attention_supported(cin, cout, cout // 4, V, nh)
    for _, cin, cout, V, nh in REFUSED:
        assert not F.st_attention_supported(cin, cout, cout // 4, V, nh)
    assert not F.st_attention_supported(16, 128, 32, 0, 8) and not F.st_attention_supported(0, 128, 32, 9, 8)


def test_mixed_batchnorm_modes_and_wrong_shapes_are_refused():
    """_bn_training (one BatchNorm in .train(), one in .eval()) raises NotImplementedError; a wrong C or V raises RuntimeError
    from the module, before any kernel sees the shape."""
    c, sd, x, *_ = _ref("n17")
    m = _case_module(c, sd)
    xd = x.to(DEV)
    for a, b in ((m.bn, m.data_bn), (m.data_bn, m.bn)):
        m.train()
        a.eval()
        with pytest.raises(NotImplementedError, match="different modes"):
            m(xd)
        assert b.training
    m.train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(RuntimeError, match="input channels"):
        m(torch.zeros(c["N"], c["cin"] + 1, c["T"], c["V"], device=DEV))
    with pytest.raises(RuntimeError, match="joints"):
        m(torch.zeros(c["N"], c["cin"], c["T"], c["V"] + 1, device=DEV))
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed by a refused call"


# ---- poisoned buffers ----------------------------------------------------------------------------------------------------------------------
def make_edge_train(name, dev):
    from _util import st_attention_train_gate
    c, sd, x, dy, mask, yr, _, g, dx = _ref(name)
    m = _case_module(c, sd)
    dyd = dy.to(dev)
    return (lambda: _step(m, sd, _fresh_x(x), dyd, mask)), st_attention_train_gate(yr, g, dx, False)


@pytest.mark.parametrize("name", ["v64_skip", "n17"])
def test_edge_steps_under_poisoned_guarded_buffers(name):
    """Every output and workspace pre-filled with NaN, then with 3.4e38, between guard bands: an empty split of
    cv_stats_kernel that left its ``parts`` unwritten, or a lane >= V that read or stored, shows as NaN or a trampled guard;
    the two runs agree bit for bit."""
    from _util import HostileCase as Case, run_under_both_fills
    run_under_both_fills(Case(f"st_attention_edge_train-{name}", functools.partial(make_edge_train, name), True), DEV)
