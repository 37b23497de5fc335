"""GPU tests of what the HIP entry points do to memory AROUND their results (tests/_util.py::hostile_allocations).

Every case below calls an entry point through its stgcn_amd.functional wrapper (or through the module the existing tests use)
twice, while ``torch.empty`` / ``torch.empty_like`` hand out buffers that are pre-filled with a poison byte and sit between two
1 MiB guard bands.  After each run: the guards are intact (nothing was written outside what the ``*_bytes`` queries size, nor
outside an output), every output is finite and passes the gate of the entry point's existing test (same reference, same
tolerance) - so nothing depends on what an output or a workspace held before - and, where the kernels promise run-to-run
identity, the two runs (NaN poison, huge-finite poison) agree bit for bit.  The second half makes every size query answer
eight bytes short and expects STGCN_ERR_WORKSPACE before anything is launched.

The patch is process-wide: no graph capture and no threads in this file."""
import functools
import itertools
from ctypes import c_int, c_size_t, c_uint, c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import altformer_ref as ar
import altformer_train_ref as tr
import entry_points as ep
import st_attention_ref as R
from _util import (FILLS, MATH_GATES, HostileCase as Case, grad_gate, hostile_allocations, parity_gate, run_under_both_fills,
                   st_attention_train_gate)
from entry_points import (AGCN_SHAPES, STEM_KERNELS, STEM_MATHS, STEM_SHAPES, TCN_KERNELS, TCN_SHAPES, TILE_FORMS, TRAIN_STRICT,
                          _stem_kernel, _tcn_mode, hipF as _F, math_flag as _math)

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
BF16_OUT_GATE = 4e-3          # test_large_tile_temporal_conv_kernel: half an ulp of the stored bf16 value, max-norm criterion


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


# ---- the table ------------------------------------------------------------------------------------------------------------------
# A case (tests/_util.py::HostileCase): ``make(dev)`` prepares inputs and references OUTSIDE the hostile block - where a family is
# shared with the non-finite contract, from its tests/entry_points.py setup - and returns ``(run, gate)``.
CASES = []


def add(id, bitwise, make, *args):
    CASES.append(Case(id, functools.partial(make, *args), bitwise))


# ---- inference: graph conv --------------------------------------------------------------------------------------------------------
def make_agcn(N, cin, cout, T, V, dev):
    s = ep.agcn(N, cin, cout, T, V)
    ref = s.reference(s.x)
    run, xd = s.on(dev), s.x.to(dev)

    def gate(o, what):
        parity_gate(o["y"], ref["y"], 1e-4, f"{what} y")
        parity_gate(o["P"], ref["P"], 1e-4, f"{what} P")
        parity_gate(o["P_attention"], ref["P_attention"], 1e-4, f"{what} P (agcn_attention)")
    return (lambda: run(xd)), gate


for _s in AGCN_SHAPES:
    add("agcn_forward-" + "x".join(map(str, _s)), True, make_agcn, *_s)


# ---- inference: temporal conv -----------------------------------------------------------------------------------------------------
def make_tcn(cin, cout, K, stride, T, V, N, math, out_bf16, along_v, dev):
    s = ep.tcn(cin, cout, K, stride, T, V, N, math, out_bf16, along_v)
    ref = s.reference(s.x)
    run, xd = s.on(dev, pack_every_run=True), s.x.to(dev)

    def gate(o, what):
        rel, strict = (BF16_OUT_GATE, False) if out_bf16 else MATH_GATES[math]
        for k, y in o.items():
            assert y.dtype == (torch.bfloat16 if out_bf16 else torch.float32) and y.is_contiguous()
            parity_gate(y.float(), ref[k], rel, f"{what} {k}", strict)
    return (lambda: run(xd)), gate


for _s in TCN_SHAPES:
    add("tcn-" + "x".join(map(str, _s[:7])) + f"-{_s[7]}" + ("-bf16out" if _s[8] else "") + ("-alongV" if _s[9] else ""), True, make_tcn, *_s)


def test_tcn_cases_reach_every_kernel():
    assert {_tcn_mode(ci, co, K, s, T, V, m, av)[1] for ci, co, K, s, T, V, N, m, ob, av in TCN_SHAPES} == TCN_KERNELS


# ---- inference: the fused stem ----------------------------------------------------------------------------------------------------
def _stem_cases():
    F = _F()
    return [(s, m) for s in STEM_SHAPES for m in STEM_MATHS if F.stem_supported(3, s[3], s[1], s[2], 9, 3, _math(m))]


@functools.lru_cache(maxsize=None)
def _stem_setup(N, T, V, C, dev):
    """The staged stem, the input on the device and the fp64 oracle's result of one stem shape: computed once, shared by the
    arithmetic modes."""
    s = ep.stem(N, T, V, C)
    return s.on(dev), s.x.to(dev), s.reference(s.x)


def _stem_one_call(F, x, st, prep, shift, C, K, fl, oshape, odt):
    """stgcn_stem_forward_prepared (attention + fused kernel in one C call), as test_stem_forward_prepared_entry_point calls it."""
    from stgcn_amd import _capi
    N, Cin, T, V = x.shape
    S, inter_c, _ = st["Wa"].shape
    need = _capi.lib().stgcn_stem_ws_bytes(N, Cin, C, T, V, K, S, fl)
    ws = torch.empty((need + 3) // 4, device=x.device, dtype=torch.float32)
    out = torch.empty(oshape, device=x.device, dtype=odt)
    p = lambda t: c_void_p(t.data_ptr())       # noqa: E731
    _capi.call("stgcn_stem_forward_prepared", p(x), p(st["A_eff"]), p(st["Wa"]), p(st["ba"]), p(st["Wb"]), p(st["bb"]), p(prep),
               p(shift), p(ws), c_size_t(ws.numel() * 4), p(out), c_int(N), c_int(Cin), c_int(C), c_int(T), c_int(V), c_int(inter_c),
               c_int(S), c_int(K), c_uint(fl), c_void_p(torch.cuda.current_stream().cuda_stream))
    return out, ws[:N * S * V * V].view(N, S, V, V)


def make_stem(shape, math, dev):
    from stgcn_amd import _capi
    F = _F()
    N, T, V, C = shape
    staged, xd, ref = _stem_setup(N, T, V, C, dev)
    ref, P_ref = ref["out"], ref["P"]
    mode = _math(math)
    variants = list(itertools.product((False, True), (False, True)))           # (channels-last output, bf16 output)

    def run():
        out = {}
        prep = staged.prepare(mode)
        for cl, b16 in variants:
            tag = f"[{'ntvc' if cl else 'nctv'},{'bf16' if b16 else 'f32'}]"
            out["out" + tag], out["P" + tag] = staged.forward(xd, prep, mode, "nctv", "ntvc" if cl else "nctv", b16)
            fl = F._flags(mode, b16) | (_capi.OUT_NTVC if cl else 0)
            o1, out["P_one_call" + tag] = _stem_one_call(F, xd, staged.st, prep, staged.ts["shift"], C, 9, fl,
                                                         (N, T, V, C) if cl else (N, C, T, V), torch.bfloat16 if b16 else torch.float32)
            out["out_one_call" + tag] = o1.permute(0, 3, 1, 2) if cl else o1
        return out

    def gate(o, what):
        rel, strict = MATH_GATES[math]
        for k, t in o.items():
            if k.startswith("P"):
                parity_gate(t, P_ref, 1e-4, f"{what} {k}")
            elif "bf16]" in k:                                              # the stored value is rounded to bf16 on top of the math's error
                parity_gate(t.float(), ref, max(rel, BF16_OUT_GATE), f"{what} {k}", False)
            else:
                parity_gate(t, ref, rel, f"{what} {k}", strict)
        for cl, b16 in variants:                                            # test_stem_forward_prepared_entry_point / layout fusion: same bits
            tag = f"[{'ntvc' if cl else 'nctv'},{'bf16' if b16 else 'f32'}]"
            assert torch.equal(o["out_one_call" + tag], o["out" + tag]), f"{what}: one-call entry differs {tag}"
            assert torch.equal(o["out" + tag], o[f"out[nctv,{'bf16' if b16 else 'f32'}]"]), f"{what}: layouts differ {tag}"
    return run, gate


def _add_stem_cases():
    try:
        cases = _stem_cases()
    except Exception:                          # the library is missing: the dev fixture reports it, test by test
        cases = [(s, m) for s in STEM_SHAPES for m in STEM_MATHS]
    for s, m in cases:
        add("stem-" + "x".join(map(str, s)) + "-" + m, True, make_stem, s, m)


_add_stem_cases()


def test_stem_cases_reach_every_kernel():
    assert {_stem_kernel(s, m) for s, m in _stem_cases()} == STEM_KERNELS


# ---- inference: patch embedding, step statistics ----------------------------------------------------------------------------------
def make_patch_embed(order, layout, dev):
    s = ep.patch_embed(order, layout)
    ref = s.reference(s.x)
    run, zd = s.on(dev), s.x.to(dev)

    def gate(o, what):                          # test_patch_embedding_vs_reference: the max-norm criterion at 1e-4
        parity_gate(o["e"], ref["e"], 1e-4, f"{what} e", strict=False)
        parity_gate(o["e_no_pos"], ref["e_no_pos"], 1e-4, f"{what} e without pos", strict=False)
    return (lambda: run(zd)), gate


for _o, _l in itertools.product(("ST", "TS"), ("nctv", "ntvc")):
    add(f"patch_embed-{_o}-{_l}", True, make_patch_embed, _o, _l)


def make_step_stats(n, classes, dev):
    """test_step_stats_argmax_is_numpy_argmax: ties, NaN rows and +-inf - the row maximum is where a stale NaN would be dropped
    and a stale huge value would win."""
    s = ep.step_stats(n, classes, special=True)
    want, labels = s.want, s.labels
    out = torch.randn(n, 4, 2, 3, generator=s.gen).to(dev)
    probe = out[:, :, 0, 0].double().cpu()
    staged, ld = s.on(dev, out), s.x.to(dev)

    def gate(o, what):
        count, correct = o["count_correct"].cpu()
        assert np.array_equal(o["pred"].cpu().numpy(), want), what
        assert float(correct) == float((torch.from_numpy(want) == labels).sum()) and float(count) == n, what
        assert torch.allclose(o["probe"].cpu().double(), torch.tensor([probe.sum().item(), probe.square().sum().item()], dtype=torch.float64),
                              rtol=1e-5, atol=1e-3), what
    return (lambda: staged(ld)), gate


for _n, _c in ((300, 28), (1, 2)):
    add(f"step_stats-{_n}x{_c}", True, make_step_stats, _n, _c)


# ---- inference: ST-TR spatial attention -------------------------------------------------------------------------------------------
def make_st_attention(N, cin, cout, T, V, dev):
    s = ep.st_attention(N, cin, cout, T, V)
    run, xd = s.on(dev), s.x.to(dev)
    ref = s.reference(s.x)["y"]

    def gate(o, what):
        parity_gate(o["y"], ref, what=f"{what} eval vs fp64")
    return (lambda: run(xd)), gate


for _s in [(2, 131, 128, 12, 22), (5, 64, 128, 33, 25), (2, 256, 512, 3, 46)]:
    add("st_attention_forward-" + "x".join(map(str, _s)), True, make_st_attention, *_s)


# ---- inference: the AltFormer heads -----------------------------------------------------------------------------------------------
LINEAR_M = (1, 129, 300)
LINEAR_KN = ((32, 64), (96, 100), (256, 200), (512, 1536))       # the first two are new: K below a k-step of the large tile, Nout off every tile


def make_vit_linear(M, K, Nout, math, dev):
    from stgcn_amd import _capi
    assert (_capi.VIT_TILE_64, _capi.VIT_TILE_32) == (TILE_FORMS[(64, 64)], TILE_FORMS[(32, 64)])
    assert _F().vit_linear_supported(M, K, Nout, _math(math))
    s = ep.vit_linear(M, K, Nout, math)
    want = s.reference(s.x)
    run, xd = s.on(dev), s.x.to(dev)

    def gate(o, what):
        for k, y in o.items():
            parity_gate(y, want[k], REL, f"{what} {k}")
            assert torch.equal(y, o[k.split("(")[0] + "(128, 128)"]), f"{what} {k}: a tile form changes the result"
    return (lambda: run(xd)), gate


for _m, (_k, _n), _ma in itertools.product(LINEAR_M, LINEAR_KN, ("f32", "bf16x3")):
    add(f"vit_linear-{_m}x{_k}x{_n}-{_ma}", True, make_vit_linear, _m, _k, _n, _ma)


def test_linear_cases_reach_every_tile_form():
    F = _F()
    seen = {F.vit_linear_tile(M, K, Nout, _math(ma) | fl) for M in LINEAR_M for K, Nout in LINEAR_KN for ma in ("f32", "bf16x3")
            for fl in TILE_FORMS.values()}
    assert seen == set(TILE_FORMS)


def make_vit_attention(L, hd, dev):
    s = ep.vit_attention("resident", 9, L, hd)
    want = s.reference(s.x)["out"]
    run, qd = s.on(dev), s.x.to(dev)

    def gate(o, what):
        parity_gate(o["out"], want, REL, what)
    return (lambda: run(qd)), gate


for _L, _hd in itertools.product((1, 33, 65, 256), (32, 64)):
    add(f"vit_attention-L{_L}-hd{_hd}", True, make_vit_attention, _L, _hd)


def make_vit_block(B, L, D, heads, hidden, mode, dev):
    from stgcn_amd import _capi
    assert _F().vit_block_supported(L, D, heads, hidden)
    s = ep.vit_block(B, L, D, heads, hidden, mode)
    run, xd = s.on(dev), s.x.to(dev)
    want = s.reference(xd if B * L > 4096 else s.x)["y"]      # the fp64 restatement on the device: the CPU would take tens of seconds

    def gate(o, what):
        parity_gate(o["y"], want, REL, f"{what} y")
        assert torch.equal(o["y_auto_tiles"], o["y"]), f"{what}: VIT_TILE_AUTO changes the result"
    return (lambda: {"y": run(xd)["y"], "y_auto_tiles": run(xd, _capi.VIT_TILE_AUTO)["y"]}), gate


# the third: 33,000 tokens = two slabs of the block entry point, 1489 and 11 sequences - the last slab is short
for _s, _mo in itertools.product([(7, 1, 256, 8, 512), (3, 65, 512, 8, 1024), (1500, 22, 256, 8, 512)], ("f32", "mixed")):
    add("vit_block_forward-" + "x".join(map(str, _s)) + "-" + _mo, True, make_vit_block, *_s, _mo)


# ---- training: graph conv ---------------------------------------------------------------------------------------------------------
def make_agcn_train(cin, cout, N, T, V, want_dx, frozen, dev):
    """Through the module (autograd.Function -> agcn_forward_train -> agcn_backward_train), as test_unit_agcn_backward_vs_oracle,
    test_unit_agcn_generic_backward_vs_oracle and test_eval_mode_backward_unit_agcn_vs_oracle do."""
    s = ep.agcn_train(cin, cout, N, T, V, want_dx, kink_free=True, frozen=frozen)
    want = s.reference(s.x)
    ref = {k: want["d" + k] for k in s.leaves}
    run = s.on(dev, fresh=False)

    def gate(o, what):
        parity_gate(o["y"], want["y"], 1e-4, f"{what} forward")
        got = {k[1:]: v for k, v in o.items() if k[1:] in ref}
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
    return (lambda: run(s.x)), gate


# not bitwise: the BatchNorm batch sums are fp64 atomicAdd (train_bn.hip: sums[c], sums[C + c]) and the moment form adds its
# attention-gradient partials with float atomicAdd (agcn_backward.hip: dPs)
add("agcn_train-moment_form-3x128-3x20x22", False, make_agcn_train, 3, 128, 3, 20, 22, False, False)
add("agcn_train-generic-64x64-2x12x22-dx", False, make_agcn_train, 64, 64, 2, 12, 22, True, False)
add("agcn_train-generic-64x128-2x9x25-frozen", False, make_agcn_train, 64, 128, 2, 9, 25, True, True)


# ---- training: temporal conv ------------------------------------------------------------------------------------------------------
TCN_TRAIN_SHAPES = [(128, 128, 9, 1, 3, 21, 22, True), (64, 128, 9, 2, 2, 21, 22, True), (32, 64, 2, 1, 2, 7, 22, True),
                    (128, 256, 9, 1, 3, 13, 17, True), (64, 128, 9, 1, 1, 1, 22, True), (128, 256, 9, 2, 2, 31, 25, False)]


def make_tcn_train(cin, cout, K, stride, N, T, V, bias, math, dev):
    """test_unit2d_backward_vs_oracle, through the module (tcn_forward_train -> tcn_backward_train)."""
    s = ep.tcn_train(cin, cout, K, stride, N, T, V, math, bias=bias, kink_free=True)
    want = s.reference(s.x)
    run = s.on(dev, fresh=False)

    def gate(o, what):
        parity_gate(o["y"], want["y"], 1e-4, f"{what} forward")
        grad_gate(o["dW"], want["dW"], 1e-4, f"{what} dW")
        grad_gate(o["dgamma"], want["dgamma"], 1e-4, f"{what} dgamma")
        grad_gate(o["dbeta"], want["dbeta"], 1e-4, f"{what} dbeta")
        grad_gate(o["dx"], want["dx"], 1e-4, f"{what} dx")
        if bias:       # analytically zero behind a batch-statistics BatchNorm: rounding noise
            assert o["dbias"].abs().max().item() <= 1e-3 * want["dbeta"].abs().max().item(), f"{what} dbias"
    return (lambda: run(s.x)), gate


# not bitwise: float atomicAdd in the channel sums and the VALU weight gradient (tcn_backward.hip: sums, bsum, dW), fp64 atomicAdd
# in the in-conv statistics (tcn_bf16_v6.hip: sstat, stats) and in the BatchNorm batch sums (train_bn.hip: sums)
for _s, _ma in itertools.product(TCN_TRAIN_SHAPES, ("bf16x3", "f32_valu")):
    add("tcn_train-" + "x".join(map(str, _s[:7])) + ("" if _s[7] else "-nobias") + "-" + _ma, False, make_tcn_train, *_s, _ma)


# ---- training: ST-TR spatial attention --------------------------------------------------------------------------------------------
def make_st_attention_train(N, cin, cout, T, V, frozen, dev):
    """test_gradients_vs_fp64_autograd_and_rng_state (drop-connect mask from the seeded generator) and
    test_without_drop_connect_and_frozen_batchnorm_under_autograd, through the module."""
    sd = R.make_state(cin, cout, V, 21 if frozen else 11)
    x = R.make_input(N, cin, T, V, 22 if frozen else 12)
    m = ep.st_unit(cin, cout, V, sd).train(not frozen)
    mask = None
    if not frozen:
        torch.manual_seed(99)
        mask = torch.bernoulli(0.5 * torch.ones(N * T * 8 * V, device=dev)).cpu()
    dy = torch.randn(N, cout, T, V, generator=torch.Generator().manual_seed(23 if frozen else 13))
    yr, _, g, dx = R.grads64(sd, x, dy, training=not frozen, mask=mask)
    dyd = dy.to(dev)

    def run():
        m.load_state_dict(sd)                   # the running statistics of the previous run
        for p in m.parameters():
            p.grad = None
        xg = x.to(dev).requires_grad_(True)
        torch.manual_seed(99)
        y = m(xg)
        y.backward(dyd)
        return {"y": y.detach(), "dx": xg.grad, **{"d" + k: p.grad for k, p in m.named_parameters()}}

    return run, st_attention_train_gate(yr, g, dx, frozen)


add("st_attention_train-3x256x256x10x46-mask", True, make_st_attention_train, 3, 256, 256, 10, 46, False)
add("st_attention_train-2x131x128x12x22-frozen", True, make_st_attention_train, 2, 131, 128, 12, 22, True)


# ---- training: the AltFormer heads' backward entry points -------------------------------------------------------------------------
def make_vit_linear_backward(M, K, Nout, math, dev):
    """test_linear_backward_vs_fp64; (33, 32, 4) is new: K of one k-step, Nout below every tile, M off every row tile."""
    F = _F()
    mode = _math(math)
    assert F.vit_linear_backward_supported(M, K, Nout, mode)
    g = torch.Generator(device=dev).manual_seed(M + K + Nout)
    dy = torch.randn(M, Nout, generator=g, device=dev) * (0.25 + 3.75 * torch.rand(M, 1, generator=g, device=dev))
    a = torch.randn(M, K, generator=g, device=dev) + 0.5
    W = (torch.rand(Nout, K, generator=g, device=dev) * 2 - 1) / K ** 0.5
    h = torch.randn(M, K, generator=g, device=dev) * 1.5
    old = torch.randn(M, K, generator=g, device=dev)
    base = dy.double() @ W.double()
    h64 = h.double().requires_grad_(True)
    TF.gelu(h64).sum().backward()
    want = {"dW": dy.double().T @ a.double(), "db": dy.double().sum(0)}
    for dgelu, accum in itertools.product((False, True), repeat=2):
        want[f"dx[gelu'={dgelu},accumulate={accum}]"] = (base * h64.grad if dgelu else base) + (old.double() if accum else 0)
    olds = [old.clone() for _ in range(2 * len(FILLS))]      # the pre-filled dx of the accumulate form is the caller's own tensor

    def run():
        out = {}
        for dgelu, accum in itertools.product((False, True), repeat=2):
            out[f"dx[gelu'={dgelu},accumulate={accum}]"], _, _ = F.vit_linear_backward(
                dy, a, W, h_pre=h if dgelu else None, dx_accumulate=olds.pop() if accum else None, need_dw=False, math=mode)
        _, out["dW"], out["db"] = F.vit_linear_backward(dy, a, W, need_dx=False, math=mode)
        _, out["dW_without_db"], none = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=False, math=mode)
        assert none is None
        return out

    def gate(o, what):
        for k, v in o.items():
            parity_gate(v, want["dW" if k == "dW_without_db" else k].cpu(), REL, f"{what} {k}")
        assert torch.equal(o["dW"], o["dW_without_db"])
    return run, gate


for _s, _ma in itertools.product([(1, 256, 256), (129, 512, 512), (300, 256, 200), (33, 32, 4)], ("f32", "bf16x3")):
    add("vit_linear_backward-" + "x".join(map(str, _s)) + "-" + _ma, True, make_vit_linear_backward, *_s, _ma)


def make_vit_attention_backward(L, hd, dev):
    s = ep.vit_attention_backward(9, L, hd)
    want = s.reference(s.x)["dqkv"]
    run, dd = s.on(dev), s.x.to(dev)

    def gate(o, what):
        parity_gate(o["dqkv"], want, REL, what)
    return (lambda: run(dd)), gate


for _L, _hd in itertools.product((1, 65, 256), (32, 64)):
    add(f"vit_attention_backward-L{_L}-hd{_hd}", True, make_vit_attention_backward, _L, _hd)


def make_vit_layernorm_backward(M, D, dev):
    """test_layernorm_backward_vs_fp64 at widths that are no multiple of the 256 floats a wave covers per pass (4, 260), one that
    is (256) and one of many passes (4096); autograd of ar.layer_norm64 is the reference."""
    s = ep.vit_layernorm_backward(M, D)
    want = s.reference(s.x)
    run, dnd = s.on(dev), s.x.to(dev)

    def gate(o, what):
        for res in (False, True):
            for k in ("dx", "dweight", "dbias"):
                parity_gate(o[f"{k}[dres={res}]"], want[f"{k}[dres={res}]"], REL, f"{what} {k} dres={res}")
    return (lambda: run(dnd)), gate


for _m, _d in [(5, 4), (7, 260), (3001, 256), (2, 4096)]:
    add(f"vit_layernorm_backward-{_m}x{_d}", True, make_vit_layernorm_backward, _m, _d)


# ---- training: one block ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block_train_reference(name, B, dev):
    """Block, input, cotangent, stochastic-depth factors and the fp64 gradients: once per case, shared by the arithmetic modes.
    ``B``: None for the fixture case's own batch (no factors, as test_forward_train_is_bit_equal_to_the_eval_forward runs it), else
    that many sequences with tr.make_scales' factors, the restatement differentiated on the device."""
    from stgcn_amd.altformer import Block
    _, L, D, _, _, seed = ar.BLOCK_CASES[name]
    blk = ar.build_block(Block, name)
    if B is None:
        x, dy, s1, s2 = ar.make_input(name), tr.make_dy(name), None, None
        want_y, want = tr.grads64(x, blk.state_dict(), dy, scale=blk.attn.scale)
    else:
        g = torch.Generator().manual_seed(seed + 5)
        x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
        dy = torch.randn(B, L, D, generator=g)
        s1, s2 = tr.make_scales(B, seed)
        want_y, want = tr.grads64(x.to(dev), {k: v.to(dev) for k, v in blk.state_dict().items()}, dy.to(dev), scale=blk.attn.scale,
                                  s1=s1.to(dev), s2=s2.to(dev))
        want_y, want = want_y.cpu(), {k: v.cpu() for k, v in want.items()}
    on = lambda t: None if t is None else t.to(dev)       # noqa: E731
    return blk.to(dev), on(x), on(dy), on(s1), on(s2), want_y, want


def make_vit_block_train(name, B, mode, dev):
    F = _F()
    blk, xd, dyd, s1, s2, want_y, want = _block_train_reference(name, B, dev)
    _, L, D, _, _, _ = ar.BLOCK_CASES[name]
    assert F.vit_block_train_supported(L, D, ar.HEADS, 2 * D)

    def run():
        y, g = ep.run_block(blk, xd, dyd, mode, s1, s2)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def gate(o, what):
        parity_gate(o["y"], want_y, REL, f"{what} y", TRAIN_STRICT[mode])
        for k, v in want.items():
            parity_gate(o["d" + k], v, REL, f"{what} d{k}", TRAIN_STRICT[mode])
    return run, gate


# 1500 x 22 x 256: two slabs of 1489 and 11 sequences - the short last slab of the forward, the saved buffer and the backward
for (_n, _b), _mo in itertools.product([("st_spatial_L22_D256", None), ("st_temporal_L180_D512", None), ("st_spatial_L22_D256", 1500)],
                                       ("f32", "mixed")):
    add(f"vit_block_train-{_n}" + (f"-B{_b}-stochastic_depth" if _b else "") + "-" + _mo, True, make_vit_block_train, _n, _b, _mo)


# ---- 3. the test over the table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_entry_point_under_poisoned_guard_banded_buffers(case, dev):
    run_under_both_fills(case, dev)


def test_every_case_without_the_bitwise_flag_is_a_training_case_with_atomics():
    """The unflagged cases are exactly the two families whose reductions use atomicAdd (named at their ``add`` calls)."""
    assert {c.id.split("-")[0] for c in CASES if not c.bitwise} == {"agcn_train", "tcn_train"}
    assert len({c.id for c in CASES}) == len(CASES)


# ---- 4. eight bytes short is refused ------------------------------------------------------------------------------------------------
# Every entry point that takes a caller-supplied size, called through its wrapper while the matching size query answers eight
# bytes less (some wrappers round their allocation up to eight bytes: eight is the smallest shortfall that always reaches the C
# check).  ``make(dev)`` prepares everything the call needs with the real queries and returns the call.
def _stem_args(dev, N=2, T=9, V=22):
    F = _F()
    staged, xd, _ = _stem_setup(3, 37, 22, 128, dev)
    return F, staged.st, staged.ts, xd, staged.prepare(F.MATH_BF16X3)


def short_tcn_forward(dev):
    from stgcn_amd import Unit2D
    F = _F()
    torch.manual_seed(3)
    st = Unit2D(32, 64, kernel_size=9).to(dev).eval()._staged(dev)
    x = torch.randn(2, 32, 12, 22, device=dev)
    return lambda: F.tcn_forward(x, st["W"], st["scale"], st["shift"], 1, F.MATH_BF16X3)


def short_stem_forward(dev):
    F, st, ts, xd, prep = _stem_args(dev)
    return lambda: F.stem_forward(xd, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], prep, ts["shift"], 128, 9, F.MATH_BF16X3)


def _agcn_train_args(dev, cin, cout):
    gcn, _, _, _, gen = ep.random_stem(22, None, 77, dev, cin=cin, c=cout)
    st = gcn.train()._staged(dev)
    bn, d = gcn.bn, gcn.down[1]
    x = torch.randn(2, cin, 12, 22, generator=gen).to(dev)
    fwd = (x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"], st["bdown"],
           (bn.weight.detach(), bn.bias.detach(), bn.running_mean.clone(), bn.running_var.clone()),
           (d.weight.detach(), d.bias.detach(), d.running_mean.clone(), d.running_var.clone()), 0.1, 1e-5)
    return gcn, st, x, fwd


def short_agcn_forward_train(dev):
    F = _F()
    _, _, _, fwd = _agcn_train_args(dev, 3, 128)
    return lambda: F.agcn_forward_train(*fwd, save=True)


def short_agcn_backward_train(dev):
    F = _F()
    gcn, st, x, fwd = _agcn_train_args(dev, 3, 128)
    bn, d = gcn.bn, gcn.down[1]
    y, P, zm, zd, stats = F.agcn_forward_train(*fwd, save=True)
    dy = torch.randn_like(y)
    return lambda: F.agcn_backward_train(*fwd[:10], P, None, None, bn.weight.detach(), bn.bias.detach(), d.weight.detach(),
                                         d.bias.detach(), stats, dy, y=None)      # the GEMM chain: the path the wrapper's query sizes


def _tcn_train_args(dev):
    torch.manual_seed(4)
    W = torch.randn(128, 64, 9, device=dev) * 0.05
    b = torch.randn(128, device=dev) * 0.1
    bn = (torch.rand(128, device=dev) + 0.5, torch.randn(128, device=dev) * 0.2, torch.zeros(128, device=dev), torch.ones(128, device=dev))
    return torch.randn(2, 64, 21, 22, device=dev), W, b, bn


def short_tcn_forward_train(dev):
    F = _F()
    x, W, b, bn = _tcn_train_args(dev)
    return lambda: F.tcn_forward_train(x, W, b, bn, 1, F.MATH_BF16X3, save=True)


def short_tcn_backward_train(dev):
    F = _F()
    x, W, b, bn = _tcn_train_args(dev)
    y, z, mean, invstd = F.tcn_forward_train(x, W, b, bn, 1, F.MATH_BF16X3, save=True)
    dy = torch.randn_like(y)
    return lambda: F.tcn_backward_train(x, W, z, bn[0], bn[1], mean, invstd, dy, 1, F.MATH_BF16X3)


def _st_args(dev):
    N, cin, cout, T, V = 2, 131, 128, 12, 22
    m = ep.st_unit(cin, cout, V, R.make_state(cin, cout, V, 21)).train()
    st = m._staged(dev)
    x = R.make_input(N, cin, T, V, 22).to(dev)
    tup = lambda b: (b.weight.detach(), b.bias.detach(), b.running_mean.clone(), b.running_var.clone())      # noqa: E731
    return m, st, x, tup


def short_st_attention_forward(dev):
    F = _F()
    m, st, x, _ = _st_args(dev)
    ds, dsh, bs, bsh = m._folded(st)
    return lambda: F.st_attention_forward(x, ds, dsh, st["Wqkv"], st["bqkv"], st["Wout"], st["bout"], bs, bsh, m._dk, m._heads)


def short_st_attention_forward_train(dev):
    F = _F()
    m, st, x, tup = _st_args(dev)
    return lambda: F.st_attention_forward_train(x, tup(m.data_bn), st["Wqkv"], st["bqkv"], st["Wout"], st["bout"], tup(m.bn), None,
                                                m._dk, m._heads)


def short_st_attention_backward(dev):
    F = _F()
    m, st, x, tup = _st_args(dev)
    y, sv = F.st_attention_forward_train(x, tup(m.data_bn), st["Wqkv"], st["bqkv"], st["Wout"], st["bout"], tup(m.bn), None, m._dk, m._heads)
    dy = torch.randn_like(y)
    return lambda: F.st_attention_backward(x, m.data_bn.weight.detach(), m.data_bn.bias.detach(), st["Wqkv"], st["Wout"],
                                           m.bn.weight.detach(), m.bn.bias.detach(), None, sv, dy, m._dk, m._heads)


def short_vit_block_forward(dev):
    F = _F()
    x, sd = ep.block_inputs(3, 22, 256, 512)
    xd, params = x.to(dev), ep.block_params(sd, dev)
    return lambda: F.vit_block_forward(xd, *params, 8, ar.EPS, 32 ** -0.5, F.MATH_F32)


def short_vit_linear_backward(dev):
    F = _F()
    dy, a, W = torch.randn(33, 64, device=dev), torch.randn(33, 32, device=dev), torch.randn(64, 32, device=dev)
    return lambda: F.vit_linear_backward(dy, a, W)


def short_vit_layernorm_backward(dev):
    F = _F()
    x, dn, w = torch.randn(7, 260, device=dev), torch.randn(7, 260, device=dev), torch.randn(260, device=dev)
    return lambda: F.vit_layernorm_backward(x, dn, w, ar.EPS)


def _block_train_args(dev):
    x, sd = ep.block_inputs(3, 22, 256, 512)
    return x.to(dev), [t for pair in ep.block_params(sd, dev) for t in pair]


def short_vit_block_forward_train(dev):
    F = _F()
    xd, flat = _block_train_args(dev)
    return lambda: F.vit_block_forward_train(xd, flat, 8, ar.EPS, 32 ** -0.5, F.MATH_F32)


def short_vit_block_backward(dev):
    F = _F()
    xd, flat = _block_train_args(dev)
    y, saved = F.vit_block_forward_train(xd, flat, 8, ar.EPS, 32 ** -0.5, F.MATH_F32)
    dy = torch.randn_like(y)
    return lambda: F.vit_block_backward(xd, flat, saved, dy, 8, ar.EPS, 32 ** -0.5, F.MATH_F32)


SHORT = [("tcn_forward", "stgcn_tcn_packed_bytes", short_tcn_forward),
         ("stem_forward", "stgcn_stem_ws_bytes", short_stem_forward),
         ("agcn_forward_train", "stgcn_agcn_train_ws_bytes", short_agcn_forward_train),
         ("agcn_backward_train", "stgcn_agcn_backward_ws_bytes", short_agcn_backward_train),
         ("tcn_forward_train", "stgcn_tcn_train_ws_bytes", short_tcn_forward_train),
         ("tcn_backward_train", "stgcn_tcn_backward_ws_bytes", short_tcn_backward_train),
         ("st_attention_forward", "stgcn_st_attention_ws_bytes", short_st_attention_forward),
         ("st_attention_forward_train", "stgcn_st_attention_ws_bytes", short_st_attention_forward_train),
         ("st_attention_backward", "stgcn_st_attention_ws_bytes", short_st_attention_backward),
         ("vit_block_forward", "stgcn_vit_block_ws_bytes", short_vit_block_forward),
         ("vit_linear_backward", "stgcn_vit_linear_backward_ws_bytes", short_vit_linear_backward),
         ("vit_layernorm_backward", "stgcn_vit_layernorm_backward_ws_bytes", short_vit_layernorm_backward),
         ("vit_block_forward_train-saved", "stgcn_vit_block_saved_bytes", short_vit_block_forward_train),
         ("vit_block_backward-saved", "stgcn_vit_block_saved_bytes", short_vit_block_backward),
         ("vit_block_backward-ws", "stgcn_vit_block_backward_ws_bytes", short_vit_block_backward)]


@pytest.mark.parametrize("name,query,make", SHORT, ids=[s[0] for s in SHORT])
def test_eight_bytes_short_is_refused_before_anything_is_launched(name, query, make, dev, monkeypatch):
    from stgcn_amd import StgcnError, _capi
    call = make(dev)
    torch.cuda.synchronize()
    lib = _capi.lib()
    real = getattr(lib, query)
    asked = []

    def eight_short(*args):
        asked.append(real(*args))
        assert asked[-1] >= 8, f"{query}{args} = {asked[-1]}: nothing to take eight bytes from"
        return asked[-1] - 8

    monkeypatch.setattr(lib, query, eight_short)
    with hostile_allocations(0xFF) as h:
        with pytest.raises(StgcnError) as e:
            call()
        torch.cuda.synchronize()
        assert asked, f"{name} never asked {query}"
        assert e.value.code == -3, f"{name}: {e.value}"
        h.check()
        assert h.records
        for i, (raw, nbytes, shape, dtype) in enumerate(h.records):      # outputs and workspaces alike: still nothing but the fill
            assert bool((raw == h.fill).all()), f"{name}: allocation #{i} (shape {shape}, {dtype}) was written by a refused call"
