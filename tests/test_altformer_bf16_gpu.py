"""GPU tests of the heads' bf16 block mode (``VIT_BF16``; include/stgcn_hip.h, DESIGN section 14 "bf16"): the bf16 linear and
attention entry points against fp64 on the rounded operands, one block against the reference's fixture and against the fp64
emulation of the mode's contract (tests/altformer_bf16_ref.py), the entry points under poisoned guard-banded buffers, the
modules' switch (``set_head_math(m, 'bf16')``) and the whole model against the reference's logits."""
import functools
import itertools

import numpy as np
import pytest
import torch

import altformer_bf16_ref as br
import altformer_ref as ar
from _util import MATH_GATES, gather_flat, hostile_allocations, load_golden, parity_gate
from test_altformer_gpu import peaked_qkv, whole_model

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]                  # the bf16 x bf16 products are exact in fp32: only the accumulation differs
BF16_REL, BF16_STRICT = MATH_GATES["bf16"]  # the project's bf16 gate: 1e-2 of max|ref|, max-norm only
assert (REL, MATH_GATES["f32"][1]) == (1e-4, True) and (BF16_REL, BF16_STRICT) == (1e-2, False)
FLIP_CAP = 1e-3                             # share of the elements that may sit one bf16 ulp off, at a rounding boundary
TILES = (0, 0x10000, 0x20000, 0x30000)      # 128 x 128, auto, 64 x 64, 32 x 64
# max|logit error| / max|logit| of the mode's fp64 emulation through a whole head of the fixture model, against the fixture's
# logits: computed on the CPU by `python tests/altformer_bf16_ref.py`.  The GPU gate is twice this.
WHOLE_MODEL_EMULATION = {"ST": 7.357e-3, "TS": 2.582e-3}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref():
    return load_golden("altformer_reference")


def gate_on_device(out, want, rel, what):
    """parity_gate's two criteria where the tensors are."""
    out = out.double()
    assert out.shape == want.shape and torch.isfinite(out).all(), what
    scale = want.abs().max().item()
    err = (out - want).abs().max().item()
    assert err <= rel * scale, f"{what}: max abs err {err:.3e} > {rel:g} * max|ref| ({scale:.3e})"
    assert torch.allclose(out, want, rtol=rel, atol=rel * 0.1 * scale), f"{what}: allclose(rtol={rel}) failed"
    return err / scale


def bf16_ulp(t):
    """Spacing of bf16 at |t| (fp64 tensor): 2^(exponent - 7), from the exponent bits (no pow: exact)."""
    p = (t.abs().clamp_min(2.0 ** -120).contiguous().view(torch.int64) & 0x7FF0000000000000).view(torch.float64)
    return p * 2.0 ** -7


def rounded_equal(got_bf16, want64, what, noise_rel=REL):
    """``got_bf16`` against the fp64 value rounded to bf16.  An element may differ from that only as the bf16 rounding of a
    value within fp32 noise of the fp64 one: |got - want| <= ulp / 2 + noise, noise = the fp32 gate's elementwise allowance
    noise_rel * (|want| + 0.1 max|want|).  Where the noise is below the spacing (everywhere but in the tail of a GELU, whose
    1e-6 outputs sit next to a max of 3) that is: one bf16 ulp off, and the fp64 value within noise of the rounding boundary.
    Returns how many elements differ; the caller caps their share."""
    got, rw = got_bf16.double(), br.r(want64)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    off = got != rw
    n = int(off.sum())
    if n:
        g, v = got[off], want64[off]
        noise = noise_rel * (v.abs() + 0.1 * want64.abs().max())
        assert ((g - v).abs() <= 0.5 * bf16_ulp(g) + noise).all(), f"{what}: off by more than a rounding at a boundary within fp32 noise"
    return n


# ---- 1. the linear ------------------------------------------------------------------------------------------------------------
LIN_M, LIN_K, LIN_N = (1, 33, 129, 200), (32, 64, 256), (14, 64, 96, 768)


@pytest.mark.parametrize("K", LIN_K)
@pytest.mark.parametrize("M", LIN_M)
def test_linear_bf16_vs_fp64_on_rounded_operands(M, K, dev):
    """Every accepted combination of LayerNorm, bias, GELU, residual and the storage kind of x and y, in the three tile forms,
    against fp64 products of the rounded operands: the project's fp32 gate, both criteria.  The rounded operands are r(W),
    r(x) (or the bf16 x as stored), and with LayerNorm what the kernel itself rounded - read back through an identity weight
    (a product with one non-zero term is exact) and held to r(LN(x)) in fp64 by the boundary rule of ``rounded_equal``.
    A bf16 y is compared after rounding the fp64 result, by the same rule; the flips are capped at 0.1 % of the elements."""
    from stgcn_amd import functional as F
    flips = total = 0
    eye = torch.eye(K, device=dev)
    for Nout in LIN_N:
        g = torch.Generator().manual_seed(1000 * M + 10 * K + Nout)
        x = torch.randn(M, K, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
        W = (torch.rand(Nout, K, generator=g) * 2 - 1) / K ** 0.5
        b = torch.randn(Nout, generator=g) * 0.5
        R = torch.randn(M, Nout, generator=g)
        lw, lb = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        xd, Wd, bd, Rd, lwd, lbd = (t.to(dev) for t in (x, W, b, R, lw, lb))
        xb = xd.bfloat16()
        ln = (lwd, lbd, ar.EPS)
        a_ln = F.vit_linear_bf16(xd, eye, ln=ln)                       # the kernel's rounded LayerNorm operand, exactly
        ln64 = ar.layer_norm64(xd.double(), lwd.double(), lbd.double(), ar.EPS)
        nf = rounded_equal(a_ln.bfloat16(), ln64, f"LN operand {M}x{K}", noise_rel=1e-5)
        assert torch.equal(a_ln.bfloat16().float(), a_ln), "the identity product returns bf16 values"
        assert nf <= max(1, FLIP_CAP * M * K), f"LN operand {M}x{K}: {nf} of {M * K} elements flipped"
        Wr = br.r(Wd)
        base = {("f32", False): br.r(xd) @ Wr.T, ("f32", True): a_ln.double() @ Wr.T, ("bf16", False): xb.double() @ Wr.T}
        for xkind, use_ln, bias, gelu, res in itertools.product(("f32", "bf16"), (False, True), (False, True), (False, True),
                                                                (False, True)):
            what = f"linear {M}x{K}x{Nout} x={xkind} ln={use_ln} bias={bias} gelu={gelu} residual={res}"
            kw = dict(bias=bd if bias else None, ln=ln if use_ln else None, residual=Rd if res else None, gelu=gelu)
            xin = xd if xkind == "f32" else xb
            if xkind == "bf16" and use_ln:
                with pytest.raises(F._capi.StgcnError) as e:
                    F.vit_linear_bf16(xin, Wd, **kw)
                assert e.value.code == -2, what                           # STGCN_ERR_UNSUPPORTED
                continue
            want = base[(xkind, use_ln)] + (bd.double() if bias else 0)
            if gelu:
                want = torch.nn.functional.gelu(want)
            if res:
                want = want + Rd.double()
            for y_bf16 in (False, True):
                ys = [F.vit_linear_bf16(xin, Wd, y_bf16=y_bf16, tile=t, **kw) for t in TILES]
                for t, y in zip(TILES[1:], ys[1:]):
                    assert torch.equal(y, ys[0]), f"{what} y_bf16={y_bf16}: tile form {t:#x} changes the result"
                if y_bf16:
                    assert ys[0].dtype == torch.bfloat16
                    flips += rounded_equal(ys[0], want, what + " (bf16 y)")
                    total += want.numel()
                else:
                    gate_on_device(ys[0], want, REL, what)
    print(f"linear M={M} K={K}: {flips} of {total} bf16 outputs one ulp off at a rounding boundary")
    assert flips <= FLIP_CAP * total, f"{flips} of {total} bf16 outputs flipped"


def test_linear_bf16_forms_are_all_reached():
    from stgcn_amd import functional as F
    seen = {F.vit_linear_tile(M, K, N, t) for M in LIN_M for K in LIN_K for N in LIN_N for t in TILES}
    assert seen == {(128, 128), (64, 64), (32, 64)}


# ---- 2. the attention -----------------------------------------------------------------------------------------------------------
def attention_gate(out, qkv, heads, scale, what):
    """|out - attention64| <= 2^-8 max|v| of the (sequence, head) pair + one bf16 ulp of the value: each p carries at most 2^-9
    relative error (the row sum adds the unrounded p, so the bound is 2^-9 max|v|; the gate is the issue's 2^-8), and the
    stored result is rounded once."""
    B, L, D3 = qkv.shape
    hd = D3 // 3 // heads
    want = ar.attention64(qkv, heads, scale)
    assert out.dtype == torch.bfloat16 and out.shape == want.shape
    got = out.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    vmax = qkv.double().reshape(B, L, 3, heads, hd)[:, :, 2].abs().amax(dim=(1, 3))              # (B, heads)
    bound = (2.0 ** -8 * vmax)[:, None, :, None] + bf16_ulp(want).reshape(B, L, heads, hd)
    err = (got - want).abs().reshape(B, L, heads, hd)
    worst = (err / bound).max().item()
    assert worst <= 1.0, f"{what}: error {worst:.3f} of the bound 2^-8 max|v| + ulp"
    return err.max().item() / want.abs().max().item()


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 22, 31, 32, 33, 46, 64, 65, 150, 180, 255, 256])
def test_attention_bf16_vs_fp64(L, hd, dev):
    """3 and 5 (sequence, head) pairs: neither fills the workgroups of the short lengths (4 pairs at L <= 32, 2 at L <= 64)."""
    from stgcn_amd import functional as F
    assert F.vit_attention_bf16_supported(L, 8, hd)
    for (B, heads), scale in itertools.product(((3, 1), (1, 5)), (None, 0.37)):
        qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd + heads).bfloat16()
        qd = qkv.to(dev)
        out = F.vit_attention_bf16(qd, heads, scale)
        rel = attention_gate(out, qkv, heads, hd ** -0.5 if scale is None else scale, f"attention L={L} hd={hd} pairs={B * heads}")
        assert torch.equal(out, F.vit_attention_bf16(qd, heads, scale)), "two runs differ"
        print(f"attention bf16 L={L} hd={hd} pairs={B * heads} scale={scale}: {rel:.3e} of max|out|")


@functools.lru_cache(maxsize=None)
def planted_qkv(case, L, hd):
    """test_vit_long_gpu.py's planted scores at a resident length: q = 8 u + noise, k_j = profile[j] / (8 scale) u + noise."""
    B, heads, scale = 2, 3, hd ** -0.5
    g = torch.Generator().manual_seed(4242 + L + hd)
    u = torch.randn(heads, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    j = torch.arange(L, dtype=torch.float32)
    if case == "rising":
        prof = -60 + 120 * j / (L - 1)
    else:
        prof = torch.full((L,), -100.0)
        prof[L - 1 if case == "spike_last" else 0] = 100.0
    qkv = torch.empty(B, L, 3, heads, hd)
    qkv[:, :, 0] = 8.0 * u + 0.01 * torch.randn(B, L, heads, hd, generator=g)
    qkv[:, :, 1] = (prof / (8.0 * scale))[None, :, None, None] * u + 0.01 * torch.randn(B, L, heads, hd, generator=g)
    qkv[:, :, 2] = torch.randn(B, L, heads, hd, generator=g)
    qkv = qkv.bfloat16()
    s = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0].double(), qkv[:, :, 1].double()) * scale
    return qkv.reshape(B, L, 3 * heads * hd), s


@pytest.mark.parametrize("L,hd", [(180, 64), (256, 32)])
@pytest.mark.parametrize("case", ["rising", "spike_first", "spike_last"])
def test_attention_bf16_on_planted_scores(case, L, hd, dev):
    from stgcn_amd import functional as F
    qkv, s = planted_qkv(case, L, hd)
    lo, hi = s.min(dim=-1).values, s.max(dim=-1).values
    if case == "rising":                                # rises by 120 over the sequence: exp(range) overflows fp32
        assert (hi - lo).min().item() > 100 and (s[..., -1] - s[..., 0]).min().item() > 100
    else:                                               # one key 200 above the rest
        at = s.argmax(dim=-1)
        assert bool((at == (L - 1 if case == "spike_last" else 0)).all())
        assert (hi - s.median(dim=-1).values).min().item() > 150
    out = F.vit_attention_bf16(qkv.to(dev), 3)
    print(f"planted {case} L={L}: {attention_gate(out, qkv, 3, hd ** -0.5, f'planted {case} L={L} hd={hd}'):.3e}")


# ---- 3. one block ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(name):
    """(x, module on the CPU, fp64 reference y, emulated y) of a fixture case, computed once."""
    from stgcn_amd.altformer import Block
    x = ar.make_input(name)
    blk = ar.build_block(Block, name)
    sd = blk.state_dict()
    y64, _ = ar.block64(x, sd, scale=blk.attn.scale)
    emu, _ = br.block_bf16_64(x, sd, scale=blk.attn.scale)
    return x, blk, y64, emu


def block_params(blk):
    a, m = blk.attn, blk.mlp
    return ((blk.norm1.weight, blk.norm1.bias), (a.qkv.weight, a.qkv.bias), (a.proj.weight, a.proj.bias),
            (blk.norm2.weight, blk.norm2.bias), (m.fc1.weight, m.fc1.bias), (m.fc2.weight, m.fc2.bias))


@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_bf16_vs_reference_case_and_emulation(name, ref, dev):
    """y against the reference's fixture under the project's bf16 gate, and against the fp64 emulation of the contract:
    max|kernel - emulation| <= 1/4 max|emulation - fp64 reference|.  A missing or an extra rounding point moves the result by
    about the whole distance.  Measured ratios (MI355X): 0.11 - 0.23, DESIGN section 14 "bf16"."""
    import copy
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import set_head_math
    x, blk_cpu, y64, emu = block_case(name)
    pre = f"case.{name}."
    assert torch.equal(gather_flat(x, ref[pre + "x_idx"].astype(np.int64)), torch.from_numpy(ref[pre + "x_val"]))
    blk = copy.deepcopy(blk_cpu).to(dev)
    set_head_math(blk, "bf16")
    blk.hip_min_tokens = 0
    xd = x.to(dev)
    with torch.no_grad():
        assert blk.uses_hip(xd)
        y = blk(xd)
        assert torch.equal(y, blk(xd)), "two runs differ"
        for t in TILES[1:]:
            yt = F.vit_block_forward(xd, *block_params(blk), blk.attn.num_heads, ar.EPS, blk.attn.scale, F.VIT_BF16 | t)
            assert torch.equal(yt, y), f"tile field {t:#x} changes the result"
        set_head_math(blk, None)
        assert not torch.equal(blk(xd), y), "the bf16 mode gave the default arithmetic's bits"
    got = gather_flat(y.cpu(), ref[pre + "y_idx"].astype(np.int64))
    rel = parity_gate(got, ref[pre + "y_val"], BF16_REL, f"{name} bf16 y", BF16_STRICT)
    dist = (emu - y64).abs().max().item()
    off = (y.cpu().double() - emu).abs().max().item()
    print(f"{name}: y vs fixture {rel:.3e}; emulation vs fp64 {dist / y64.abs().max().item():.3e}; kernel vs emulation / that = {off / dist:.3f}")
    assert off <= 0.25 * dist, f"{name}: max|kernel - emulation| = {off:.3e} > 1/4 of max|emulation - fp64| = {dist:.3e}"


def test_block_bf16_more_than_one_slab(dev):
    """33,000 tokens = two slabs of the entry point, 1489 and 11 sequences (the last one short): the bf16 gate against the
    fp64 restatement on the device, and the last slab's sequences equal a call of their own bit for bit."""
    from stgcn_amd import functional as F
    B, L, D, heads, hidden = 1500, 22, 256, 8, 512
    sd = {k: v.to(dev) for k, v in ar.random_block_state(D, hidden, True, seed=B + L + D).items()}
    g = torch.Generator().manual_seed(L)
    x = (torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)).to(dev)
    pair = lambda n: (sd[n + ".weight"], sd[n + ".bias"])       # noqa: E731
    params = (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))
    y = F.vit_block_forward(x, *params, heads, ar.EPS, (D // heads) ** -0.5, F.VIT_BF16)
    assert B * L > 32768 and 32768 // L == 1489
    want = ar.block64(x, sd, heads=heads)[0]
    rel = parity_gate(y, want.cpu(), BF16_REL, "two slabs, bf16", BF16_STRICT)
    print(f"two slabs bf16: {rel:.3e}")
    assert torch.equal(y, F.vit_block_forward(x, *params, heads, ar.EPS, (D // heads) ** -0.5, F.VIT_BF16 | TILES[1]))
    tail = F.vit_block_forward(x[1489:].contiguous(), *params, heads, ar.EPS, (D // heads) ** -0.5, F.VIT_BF16)
    assert torch.equal(y[1489:], tail), "the short last slab differs from a call of its own"


def test_block_bf16_refuses_the_streaming_length(dev):
    from stgcn_amd import functional as F
    B, L, D, heads, hidden = 2, 257, 256, 8, 512
    sd = {k: v.to(dev) for k, v in ar.random_block_state(D, hidden, True, seed=1).items()}
    pair = lambda n: (sd[n + ".weight"], sd[n + ".bias"])       # noqa: E731
    params = (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))
    x = torch.randn(B, L, D, device=dev)
    assert F.vit_block_forward_supported(L, D, heads, hidden) and not F.vit_block_forward_bf16_supported(L, D, heads, hidden)
    with pytest.raises(F._capi.StgcnError) as e:
        F.vit_block_forward(x, *params, heads, ar.EPS, 32 ** -0.5, F.VIT_BF16)
    assert e.value.code == -2 and "STGCN_VIT_BF16" in str(e.value)
    with pytest.raises(F._capi.StgcnError) as e:
        F.vit_block_forward(x[:, :22].contiguous(), *params, heads, ar.EPS, 32 ** -0.5, F.VIT_BF16 | F._capi.VIT_QKV_F32)
    assert e.value.code == -1
    F.vit_block_forward(x, *params, heads, ar.EPS, 32 ** -0.5, F.MATH_F32)          # the fp32 block still runs the length


# ---- 4. poisoned, guard-banded buffers ----------------------------------------------------------------------------------------------
FILLS = (0xFF, 0x7F)


def under_both_fills(run, gate, what):
    outs = []
    for fill in FILLS:
        with hostile_allocations(fill) as h:
            out = run(h)
            torch.cuda.synchronize()
            h.check()
        assert h.records, f"{what}: no allocation went through torch.empty"
        for k, t in out.items():
            assert torch.isfinite(t.float()).all(), f"{what} fill={fill:#x}: {k} is not finite"
        gate(out, f"{what} fill={fill:#x}")
        outs.append(out)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), f"{what}: {k} differs between the NaN-filled and the huge-filled run"


@pytest.mark.parametrize("L", [22, 180])
def test_linear_bf16_under_poisoned_buffers(L, dev):
    from stgcn_amd import functional as F
    M, K, Nout = 3 * L, 256, 768
    g = torch.Generator().manual_seed(M)
    x, W, b = torch.randn(M, K, generator=g), (torch.rand(Nout, K, generator=g) * 2 - 1) / 16, torch.randn(Nout, generator=g)
    R = torch.randn(M, Nout, generator=g)
    lw, lb = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    xd, Wd, bd, Rd, lwd, lbd = (t.to(dev) for t in (x, W, b, R, lw, lb))
    xb = xd.bfloat16()
    want = {"f32": br.r(xd) @ br.r(Wd).T + bd.double() + Rd.double(), "bf16": xb.double() @ br.r(Wd).T + bd.double() + Rd.double()}
    clean = F.vit_linear_bf16(xd, Wd, bd, ln=(lwd, lbd, ar.EPS), gelu=True, y_bf16=True)

    def run(h):
        out = {}
        for t in TILES:
            out[f"f32->f32 {t:#x}"] = F.vit_linear_bf16(xd, Wd, bd, residual=Rd, tile=t)
            out[f"bf16->f32 {t:#x}"] = F.vit_linear_bf16(xb, Wd, bd, residual=Rd, tile=t)
            out[f"f32->bf16 {t:#x}"] = F.vit_linear_bf16(xd, Wd, bd, residual=Rd, y_bf16=True, tile=t)
            out[f"bf16->bf16 {t:#x}"] = F.vit_linear_bf16(xb, Wd, bd, residual=Rd, y_bf16=True, tile=t)
            out[f"ln gelu {t:#x}"] = F.vit_linear_bf16(xd, Wd, bd, ln=(lwd, lbd, ar.EPS), gelu=True, y_bf16=True, tile=t)
        return out

    def gate(o, what):
        flips = total = 0
        for k, y in o.items():
            if k.startswith("ln gelu"):
                assert torch.equal(y, clean), f"{what} {k}: differs from the call on ordinary buffers"
            elif y.dtype == torch.bfloat16:
                flips += rounded_equal(y, want[k.split("->")[0]], f"{what} {k}")
                total += y.numel()
            else:
                gate_on_device(y, want[k.split("->")[0]], REL, f"{what} {k}")
        assert flips <= FLIP_CAP * total
    under_both_fills(run, gate, f"vit_linear_bf16 L={L}")


@pytest.mark.parametrize("L", [22, 180])
def test_attention_bf16_under_poisoned_buffers(L, dev):
    from stgcn_amd import functional as F
    cases = {hd: peaked_qkv(3, L, 8, hd, 100 * L + hd).bfloat16() for hd in (32, 64)}
    on_dev = {hd: q.to(dev) for hd, q in cases.items()}

    def run(h):
        return {f"hd{hd}": F.vit_attention_bf16(q, 8) for hd, q in on_dev.items()}

    def gate(o, what):
        for hd, q in cases.items():
            attention_gate(o[f"hd{hd}"], q, 8, hd ** -0.5, f"{what} hd={hd}")
    under_both_fills(run, gate, f"vit_attention_bf16 L={L}")


def bf16_plan_bytes(B, L, D, hidden):
    """What the bf16 block carves from its workspace: qkv, the attention output and the fc1 hidden as bf16, x1 as fp32, for one
    slab of whole sequences (32768 tokens at the most), each piece padded to 256 bytes."""
    rows = min(B, max(1, 32768 // L)) * L
    up = lambda n: (n + 255) // 256 * 256                       # noqa: E731
    return up(rows * 3 * D * 2) + up(rows * D * 2) + up(rows * D * 4) + up(rows * hidden * 2)


@pytest.mark.parametrize("L", [22, 180])
def test_block_bf16_under_poisoned_buffers(L, dev):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    B, D, heads, hidden = 5, 256, 8, 512
    sd = ar.random_block_state(D, hidden, True, seed=B + L + D)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    want = ar.block64(x, sd, heads=heads)[0]
    sdd = {k: v.to(dev) for k, v in sd.items()}
    pair = lambda n: (sdd[n + ".weight"], sdd[n + ".bias"])       # noqa: E731
    params = (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))
    xd = x.to(dev)
    sized = _capi.lib().stgcn_vit_block_ws_bytes(B, L, D, hidden)
    plan = bf16_plan_bytes(B, L, D, hidden)
    assert plan < sized, "the bf16 plan needs less than the workspace query sizes"

    def run(h):
        out = {"y": F.vit_block_forward(xd, *params, heads, ar.EPS, (D // heads) ** -0.5, F.VIT_BF16),
               "y_auto_tiles": F.vit_block_forward(xd, *params, heads, ar.EPS, (D // heads) ** -0.5, F.VIT_BF16 | TILES[1])}
        torch.cuda.synchronize()
        spaces = [(raw, n) for raw, n, shape, dtype in h.records if dtype == torch.float64]
        assert len(spaces) == 2 and all(n >= sized for _, n in spaces), "the two workspaces"
        for raw, n in spaces:
            assert bool((raw[h.guard + plan:h.guard + n] == h.fill).all()), "the workspace was written past the bf16 plan"
            assert not bool((raw[h.guard:h.guard + plan] == h.fill).all()), "the workspace was not used"
        return out

    def gate(o, what):
        parity_gate(o["y"], want, BF16_REL, f"{what} y", BF16_STRICT)
        assert torch.equal(o["y_auto_tiles"], o["y"])
    under_both_fills(run, gate, f"vit_block_forward bf16 L={L}")


# ---- 5. the modules -------------------------------------------------------------------------------------------------------------
SHAPES = {"12x7": (12, 7), "shrec": (180, 22)}          # (frames, joints); two clips


def make_module(kind, T, V, dev):
    """A ``Block`` as the ST head's spatial stage sees it, or a two-block-deep ``ST`` / ``TS`` head; returns (module, input)."""
    from stgcn_amd import altformer
    from stgcn_amd.altformer import set_hip_min_tokens
    torch.manual_seed(11 + T)
    if kind == "Block":
        mod = altformer.Block(256, 8, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer())
        x = torch.randn(2 * T, V, 256)
    else:
        mod = getattr(altformer, kind)(14, num_frame=T, num_joints=V, in_chans=128, embed_dim_ratio=256, depth=2, num_heads=8,
                                       mlp_ratio=2., qkv_bias=True, drop_path_rate=0.1)
        with torch.no_grad():
            for n, p in mod.named_parameters():
                if n.endswith("pos_embed"):
                    p.copy_(0.05 * torch.randn(p.shape))
        x = torch.randn(2, 128, T, V)
    set_hip_min_tokens(mod, 0)
    return mod.to(dev).eval(), x.to(dev)


def blocks_of(mod):
    from stgcn_amd.altformer import Block
    return [m for m in mod.modules() if isinstance(m, Block)]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["Block", "ST", "TS"])
def test_module_takes_the_bf16_block(kind, shape, dev):
    from stgcn_amd.altformer import set_head_math
    mod, x = make_module(kind, *SHAPES[shape], dev)
    seen = []
    hooks = [b.register_forward_pre_hook(lambda m, a: seen.append(m.uses_hip(a[0]))) for b in blocks_of(mod)]
    with torch.no_grad():
        mixed = mod(x)
        set_head_math(mod, "bf16")
        y = mod(x)
        assert torch.equal(y, mod(x)), "two runs differ"
        for h in hooks:
            h.remove()
        assert seen and all(seen), "every block call on the HIP path"
        for b in blocks_of(mod):
            b.force_torch = True
        torch_path = mod(x)
    assert not torch.equal(y, mixed), "the bf16 mode gave the default arithmetic's bits"
    rel = parity_gate(y, torch_path, BF16_REL, f"{kind} {shape} bf16 vs the torch path", BF16_STRICT)
    print(f"{kind} {shape}: bf16 vs torch path {rel:.3e}")


def test_block_of_300_tokens_runs_the_default_arithmetic(dev):
    from stgcn_amd.altformer import Block, set_head_math
    torch.manual_seed(5)
    blk = Block(256, 8, mlp_ratio=2., qkv_bias=True, norm_layer=ar.norm_layer()).to(dev).eval()
    blk.hip_min_tokens = 0
    x = torch.randn(4, 300, 256, device=dev)
    with torch.no_grad():
        want = blk(x)
        set_head_math(blk, "bf16")
        assert blk.uses_hip(x), "a 300-token call of a bf16 block stays on the HIP path"
        assert torch.equal(blk(x), want), "L = 300 under 'bf16' is the default arithmetic's result, bit for bit"
        blk.small_tiles = True
        assert torch.equal(blk(x), want)
        short = x[:, :256].contiguous()
        got = blk(short)
        set_head_math(blk, None)
        assert not torch.equal(got, blk(short)), "L = 256 under 'bf16' runs the bf16 block"


@pytest.mark.parametrize("kind", ["Block", "ST"])
def test_training_under_the_bf16_mode_is_the_default_training_arithmetic(kind, dev):
    """``loss.backward()`` with ``math_mode = 'bf16'``: the HIP training path in ``_default_train_math()``, gradients equal to
    those of a module without the mode, bit for bit.  The bit never reaches a training entry point (which would refuse it)."""
    from stgcn_amd.altformer import set_head_math
    mod, x = make_module(kind, 12, 7, dev)
    x = x.clone().requires_grad_()

    def grads():
        for p in mod.parameters():
            p.grad = None
        x.grad = None
        assert all(b.trains_on_hip(torch.zeros(4, 7, b.norm1.normalized_shape[0], device=dev, requires_grad=True)) for b in blocks_of(mod))
        out = mod(x)
        out.square().sum().backward()
        return out.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}
    y0, dx0, g0 = grads()
    set_head_math(mod, "bf16")
    y1, dx1, g1 = grads()
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and set(g0) == set(g1) and len(g0) >= 12
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_low_latency_capture_replays_the_bf16_forward(dev):
    import stgcn_amd
    from stgcn_amd.altformer import set_head_math
    mod, x = make_module("ST", 12, 7, dev)
    stgcn_amd.set_low_latency(mod, min_tokens=0)
    set_head_math(mod, "bf16")
    assert all(b.small_tiles and b.hip_min_tokens == 0 for b in blocks_of(mod))
    clips = [torch.randn(1, 128, 12, 7, device=dev) for _ in range(3)]
    with torch.no_grad():
        eager = [mod(c).clone() for c in clips]
        for b in blocks_of(mod):
            b.small_tiles = False
        assert torch.equal(mod(clips[0]), eager[0]), "the tile forms change the bf16 result"
        for b in blocks_of(mod):
            b.small_tiles = True
        static_in = clips[0].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = mod(static_in)
        for i in (1, 2):
            static_in.copy_(clips[i])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, eager[i]), f"replay with clip {i} differs from the eager result"
    assert not torch.equal(eager[1], eager[2])


# ---- 6. the whole model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["ST", "TS"])
def test_whole_model_bf16_logits_and_argmax(style, dev):
    """Skeleton clips -> logits with every block in the bf16 mode, against the reference model's logits.  Allowed: twice what
    the fp64 emulation of the mode loses on the same clips (WHOLE_MODEL_EMULATION).  The arg max must be the fixture's on every
    clip whose top-two margin exceeds twice the allowed logit error; at least half of the clips are such clips."""
    from stgcn_amd.altformer import Block, set_head_math
    model, g = whole_model(style, dev)
    set_head_math(model, "bf16")
    calls = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: calls.append(mod.uses_hip(args[0])))
             for m in model.modules() if isinstance(m, Block)]
    with torch.no_grad():
        logits = model(torch.from_numpy(g["skeleton"]).to(dev)).cpu()
    for h in hooks:
        h.remove()
    assert len(calls) == 12 and all(calls)
    want = g[f"logits_{style}"]
    allowed_rel = 2 * WHOLE_MODEL_EMULATION[style]
    rel = parity_gate(logits, want, allowed_rel, f"whole model {style} bf16", strict=False)
    print(f"whole model {style} bf16: max|err|/max|logit| = {rel:.3e} (emulation {WHOLE_MODEL_EMULATION[style]:.3e})")
    allowed = allowed_rel * float(np.abs(want).max())
    sure = g[f"margin_{style}"] > 2 * allowed
    assert sure.sum() * 2 >= len(sure), f"only {int(sure.sum())} of {len(sure)} clips have a margin above {2 * allowed:.3e}"
    assert np.array_equal(logits.argmax(1).numpy()[sure], g[f"argmax_{style}"][sure])
