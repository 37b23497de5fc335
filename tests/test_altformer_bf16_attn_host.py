"""The training attention on bf16 matrix operands (``STGCN_VIT_TRAIN_ATTN_BF16``), host side (no GPU): the fp64 emulation of its
contract (tests/altformer_bf16_attn_ref.py) held to fp64 autograd and to the figures the GPU bounds are taken from, the additive
C ABI (one flag bit, two entry points, two queries, ABI 11 unchanged), the plan's answers, the argument errors reached before
any launch, and the Python switch (``set_train_attention_math`` / ``Block.train_attention_mode`` / env
``STGCN_VIT_TRAIN_ATTENTION``).

Where the GPU bounds come from (every figure is printed before it is asserted; ``python tests/altformer_bf16_attn_ref.py``
reprints them all): at the attention level an fp32 torch run of the emulation stays within 0.039 of it in the L2 ratio
``||candidate - emulation|| / ||emulation - fp64||`` and a single missing rounding point moves the most affected tensor by 0.225
or more, so ``ATTN_L2_BOUND`` = 0.1, their geometric mean, tells the two apart.  At the block level the fp32 run alone reaches
0.39, so ``BLOCK_L2_BOUND`` = 0.8 only catches gross errors."""
import ctypes
import math
import os
import re

import pytest
import torch

import altformer_bf16_attn_ref as at
import altformer_bf16_train_ref as br
import altformer_ref as ar
import altformer_train_ref as tr
from _util import MATH_GATES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT = 0x800000
NEW_NAMES = ["stgcn_vit_attention_train_bf16_supported", "stgcn_vit_attention_train_bf16", "stgcn_vit_attention_backward_bf16",
             "stgcn_vit_block_train_attn_bf16_supported"]
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
GATE = MATH_GATES["bf16"][0]


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


# ---- the emulation, one block ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block_rows():
    """Per block case (with factors): fp64 autograd, the contract, and the two variants the contract was chosen against."""
    rows = {}
    for name in sorted(ar.BLOCK_CASES):
        x, sd, dy, scale, s1, s2 = br.case_inputs(name, True)
        kw = dict(scale=scale, s1=s1, s2=s2)
        rows[name] = dict(kw=(x, sd, dy, kw), ref=tr.grads64(x, sd, dy, **kw), contract=at.block_grads(x, sd, dy, **kw),
                          plain=at.block_grads(x, sd, dy, scores="bf16", delta="rowsum", **kw),
                          rowsum=at.block_grads(x, sd, dy, delta="rowsum", **kw))
    return rows


def test_the_contract_holds_the_gate_on_the_six_cases(block_rows):
    for name, row in block_rows.items():
        (y64, g64), (y, g) = row["ref"], row["contract"]
        worst = at.worst(g, g64)
        print(f"{name}: contract worst tensor {worst:.2e}, y {br.max_rel(y, y64):.2e}")
        assert set(g) == set(g64) and worst <= GATE and br.max_rel(y, y64) <= GATE
        assert worst <= 7e-3 and br.max_rel(y, y64) <= 5e-4, "measured 4.8e-3 - 6.4e-3 and 3.1e-4 - 3.7e-4"


def test_plain_bf16_scores_exceed_the_gate(block_rows):
    """Why the score product takes three terms: q and k rounded once put a gradient tensor over 1e-2 of max|.|."""
    worst = {name: at.worst(row["plain"][1], row["ref"][1]) for name, row in block_rows.items()}
    print("scores plain bf16, delta = rowsum(dO out):", " ".join(f"{v:.2e}" for v in worst.values()))
    assert sum(v > GATE for v in worst.values()) >= 1
    assert all(v > at.worst(block_rows[n]["contract"][1], block_rows[n]["ref"][1]) for n, v in worst.items())


def test_delta_of_the_kernels_own_products_is_not_worse_than_rowsum(block_rows):
    for name, row in block_rows.items():
        pdp, rowsum = at.worst(row["contract"][1], row["ref"][1]), at.worst(row["rowsum"][1], row["ref"][1])
        print(f"{name}: delta = sum P dP {pdp:.2e}, delta = rowsum(dO out) {rowsum:.2e}")
        assert pdp <= rowsum


def test_block_level_bound_catches_gross_errors_only(block_rows):
    """The fp32 run of the emulation against ``BLOCK_FP32_RUN_L2`` on two cases (the largest and the smallest measured), and
    plain-bf16 scores as the gross error the bound is there for."""
    assert at.BLOCK_L2_BOUND == 2 * at.BLOCK_FP32_RUN_L2
    for name in ("st_temporal_L180_D512", "ts_spatial_L46_D512"):
        row = block_rows[name]
        x, sd, dy, kw = row["kw"]
        (_, g64), (_, ge) = row["ref"], row["contract"]
        _, gf = at.block_grads(x, sd, dy, dtype=torch.float32, **kw)
        keys = [k for k in ge if k not in br.EXACT_IN_EMULATION]
        noise = max(br.l2_ratio(gf[k], ge[k], g64[k]) for k in keys)
        gross = max(br.l2_ratio(row["plain"][1][k], ge[k], g64[k]) for k in keys)
        print(f"{name}: fp32 run of the block emulation, worst L2 ratio {noise:.3f}; plain-bf16 scores {gross:.2f}")
        assert noise <= at.BLOCK_FP32_RUN_L2 and gross > at.BLOCK_L2_BOUND


# ---- the emulation, attention alone ---------------------------------------------------------------------------------------------
def test_attention_level_ratios_bracket_the_gpu_bound():
    rows = at.attention_table()
    for row in rows:
        print(f"{row['case']}: fp32 run L2 {row['fp32_l2']:.3f} (max norm {row['fp32_max']:.3f}); without "
              + " ".join(f"{p} {row[p]:.3f}" for p in at.POINTS) + f"; plain-bf16 scores {row['scores_bf16']:.2f}")
    noise = max(row["fp32_l2"] for row in rows)
    weakest = min(row[p] for row in rows for p in at.POINTS)
    assert noise <= at.FP32_RUN_L2 and weakest >= at.LEAVE_ONE_OUT_L2
    assert at.FP32_RUN_L2 < at.ATTN_L2_BOUND < at.LEAVE_ONE_OUT_L2
    assert at.ATTN_L2_BOUND == round(math.sqrt(noise * weakest), 1), "the geometric mean of the two measured ends"
    assert all(row["p_fwd"] == min(row[p] for p in at.POINTS) for row in rows), "p_fwd is the weak point"
    assert all(row[p] >= 0.45 for row in rows for p in at.POINTS if p != "p_fwd")
    assert all(row["scores_bf16"] >= 2.0 for row in rows), "plain-bf16 scores move every tensor by more than the mode's own error"
    assert max(row["fp32_max"] for row in rows) > at.LEAVE_ONE_OUT_L2, "the max norm does not separate the two"


def test_emulation_distance_over_the_gpu_tests_inputs():
    """``EMULATION_DISTANCE``: how far the contract is from the fp64 attention, per tensor, on every input of the GPU test."""
    worst = dict.fromkeys(at.TENSORS, 0.0)
    for kind, L, hd in at.ATTN_CASES:
        qkv, dout, heads, scale = at.attention_case(kind, L, hd)
        g64, ge = at.attention_grads64(qkv, dout, heads, scale), at.attention_grads(qkv, dout, heads, scale)
        for t in at.TENSORS:
            assert torch.isfinite(ge[t]).all()
            if g64[t].norm() > 0:
                worst[t] = max(worst[t], at.l2_rel(ge[t], g64[t]))
    print("largest ||emulation - fp64|| / ||fp64||:", " ".join(f"{t} {v:.2e}" for t, v in worst.items()))
    for t in at.TENSORS:
        assert 0.5 * at.EMULATION_DISTANCE[t] <= worst[t] <= at.EMULATION_DISTANCE[t], t


def test_emulation_variants_and_fp32_run():
    qkv, dout, heads, scale = at.random_qkv(2, 9, 2, 32, 1)
    g64 = at.attention_grads64(qkv, dout, heads, scale)
    exact = at.attention_grads(qkv, dout, heads, scale, scores="exact", skip="all")
    for t in at.TENSORS:
        assert torch.allclose(exact[t], g64[t], rtol=1e-12, atol=1e-14), "nothing rounded: the fp64 attention"
    f32 = at.attention_grads(qkv, dout, heads, scale, dtype=torch.float32)
    assert all(v.dtype == torch.float64 for v in f32.values()) and not torch.equal(f32["out"], exact["out"])
    with pytest.raises(KeyError):
        at.attention_grads(qkv, dout, heads, scale, scores="fp8")
    with pytest.raises(KeyError):
        at.attention_grads(qkv, dout, heads, scale, delta="none")
    with at.in_block(scores="bf16"):
        assert br.attention is not None and br.attention.__name__ == "<lambda>"
    assert br.attention.__name__ == "attention", "in_block restores altformer_bf16_train_ref.attention"


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_flag_value_prototypes_and_no_collision(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(STGCN_\w+)\s+0x([0-9A-Fa-f]+)u\b", hdr)}
    m = re.search(r"#define\s+STGCN_VIT_TRAIN_ATTN_BF16\s+\(STGCN_VIT_TRAIN_BF16\s*<<\s*(\d+)\)", hdr)
    assert m and defs["STGCN_VIT_TRAIN_BF16"] << int(m.group(1)) == BIT == _capi.VIT_TRAIN_ATTN_BF16 == F.VIT_TRAIN_ATTN_BF16
    assert len(defs) >= 19 and all(BIT & v == 0 for v in defs.values()), "collides with a flag of the header"
    assert all(BIT & v == 0 for k, v in vars(_capi).items() if k.isupper() and isinstance(v, int) and k not in
               ("VIT_TRAIN_ATTN_BF16", "ABI_VERSION"))
    handle = ctypes.CDLL(build())
    for n in NEW_NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
        assert n in open(os.path.join(ROOT, "INTEGRATION.md")).read(), n
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _capi.PROTOTYPES["stgcn_vit_attention_train_bf16"] == (I, [P] * 2 + [I] * 4 + [Fl, P])
    assert _capi.PROTOTYPES["stgcn_vit_attention_backward_bf16"] == (I, [P] * 4 + [I] * 4 + [Fl, P])
    assert _capi.PROTOTYPES["stgcn_vit_attention_train_bf16_supported"] == (I, [I] * 3)
    assert _capi.PROTOTYPES["stgcn_vit_block_train_attn_bf16_supported"] == (I, [I] * 4)
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11


def test_queries_answer_for_the_plan(lib):
    """1 exactly where a block call with the flag runs the bf16 attention: a covered shape of at most 256 tokens."""
    from stgcn_amd import functional as F
    ones = 0
    for L in (0, 1, 22, 46, 180, 255, 256, 257, 300, 4096, 4097):
        for D, heads, hidden in ((256, 8, 512), (512, 8, 1024), (384, 8, 768), (256, 8, 500), (256, 4, 512), (256, 3, 512),
                                 (128, 8, 256), (8192, 128, 64)):
            got = lib.stgcn_vit_block_train_attn_bf16_supported(L, D, heads, hidden)
            want = int(lib.stgcn_vit_block_train_long_supported(L, D, heads, hidden) == 1 and L <= 256)
            assert got == want == lib.stgcn_vit_block_train_supported(L, D, heads, hidden), (L, D, heads, hidden)
            assert F.vit_block_train_attn_bf16_supported(L, D, heads, hidden) is bool(got)
            ones += got
    assert ones == 6 * 3, "six lengths of 1 .. 256 x the three covered (D, heads, hidden) of the grid"
    for L in (0, 1, 256, 257):
        for heads in (0, 1, 8):
            for hd in (16, 32, 48, 64, 128):
                got = lib.stgcn_vit_attention_train_bf16_supported(L, heads, hd)
                assert got == lib.stgcn_vit_attention_backward_supported(L, heads, hd) == int(1 <= L <= 256 and heads >= 1 and hd in (32, 64))
                assert F.vit_attention_train_bf16_supported(L, heads, hd) is bool(got)


def test_buffers_are_sized_the_same_with_and_without_the_flag(lib):
    """The *_bytes queries take no flags; what the entry points ask of ``saved`` and the workspace is their answer with the
    flag as without it.  Host buffers that are never touched: one byte short of the need is refused before any launch."""
    from stgcn_amd._capi import MATH_BF16X3, VIT_QKV_F32, VIT_TRAIN_BF16
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast(ctypes.byref(buf, 8), ctypes.c_void_p)
    for B, L, D, hidden in ((32, 22, 256, 512), (4000, 22, 256, 512), (3, 256, 512, 1024), (3, 300, 256, 512)):
        saved = lib.stgcn_vit_block_train_long_saved_bytes(B, L, D, hidden)
        ws = lib.stgcn_vit_block_train_long_ws_bytes(B, L, D, 8, hidden)
        assert saved > 0 and ws > 0
        for fl in (0, BIT, VIT_TRAIN_BF16 | MATH_BF16X3 | VIT_QKV_F32, VIT_TRAIN_BF16 | MATH_BF16X3 | VIT_QKV_F32 | BIT):
            rc = lib.stgcn_vit_block_forward_train(*([p] * 15), 1e-6, 0.1, p, saved - 1, q, B, L, D, 8, hidden, fl, None)
            assert rc == ERR_WORKSPACE and f"< {saved} bytes".encode() in lib.stgcn_last_error(), (fl, lib.stgcn_last_error())
            rc = lib.stgcn_vit_block_backward(*([p] * 11), p, saved, p, q, *([p] * 12), 1e-6, 0.1, p, ws - 1, B, L, D, 8, hidden, fl, None)
            assert rc == ERR_WORKSPACE and f"< {ws} bytes".encode() in lib.stgcn_last_error(), (fl, lib.stgcn_last_error())


def test_argument_errors_are_reached_before_any_launch(lib):
    """Null buffers everywhere: a call that got as far as a launch would fault; these return a status and a message."""
    from stgcn_amd._capi import MATH_BF16, MATH_BF16X3, VIT_BF16, VIT_QKV_F32, VIT_TILE_64, VIT_TRAIN_BF16

    def fwd_train(fl):
        return lib.stgcn_vit_block_forward_train(*([None] * 15), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, fl, None)

    def bwd(fl):
        return lib.stgcn_vit_block_backward(*([None] * 12), 0, *([None] * 14), 1e-6, 0.1, None, 0, 2, 22, 256, 8, 512, fl, None)
    for call, name in ((fwd_train, b"forward_train"), (bwd, b"block_backward")):
        for legal in (0, MATH_BF16X3, MATH_BF16X3 | VIT_QKV_F32, VIT_TRAIN_BF16, VIT_TRAIN_BF16 | MATH_BF16X3 | VIT_QKV_F32):
            assert call(BIT | legal) == ERR_ARG and b"null" in lib.stgcn_last_error().lower(), "the bit itself is accepted"
        assert call(BIT | VIT_BF16) == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error() and name in lib.stgcn_last_error()
        assert call(BIT | VIT_TILE_64) == ERR_ARG and b"STGCN_VIT_TILE" in lib.stgcn_last_error()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.stgcn_vit_block_forward_train(*([p] * 15), 1e-6, 0.1, p, 0, ctypes.cast(ctypes.byref(buf, 8), ctypes.c_void_p),
                                           2, 22, 256, 8, 512, BIT | MATH_BF16, None)
    assert rc == ERR_UNSUPPORTED and b"math" in lib.stgcn_last_error(), "bad low bits: refused as ever, after the pointers"
    # the three entry points that refuse the bit, by name, before they look at a pointer
    rc = lib.stgcn_vit_block_forward(*([None] * 13), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, BIT | MATH_BF16X3, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TRAIN_ATTN_BF16" in lib.stgcn_last_error() and b"stgcn_vit_block_forward:" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_linear(*([None] * 5), 1e-6, None, None, 4, 256, 256, BIT, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TRAIN_ATTN_BF16" in lib.stgcn_last_error() and b"stgcn_vit_linear:" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_linear_backward(*([None] * 8), 0, 44, 256, 512, BIT, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TRAIN_ATTN_BF16" in lib.stgcn_last_error() and b"stgcn_vit_linear_backward:" in lib.stgcn_last_error()
    # older refusals answer first
    rc = lib.stgcn_vit_block_forward(*([None] * 13), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, BIT | VIT_TRAIN_BF16, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TRAIN_BF16 " in lib.stgcn_last_error()
    rc = lib.stgcn_vit_linear(*([None] * 5), 1e-6, None, None, 4, 256, 256, BIT | VIT_TRAIN_BF16, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TRAIN_BF16 " in lib.stgcn_last_error()
    rc = lib.stgcn_vit_linear_backward(*([None] * 8), 0, 44, 256, 512, BIT | VIT_TILE_64, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TILE" in lib.stgcn_last_error()
    # the two kernels alone
    assert lib.stgcn_vit_attention_train_bf16(None, None, 2, 22, 8, 32, 0.1, None) == ERR_ARG
    assert lib.stgcn_vit_attention_backward_bf16(None, None, None, None, 2, 22, 8, 32, 0.1, None) == ERR_ARG
    assert lib.stgcn_vit_attention_train_bf16(p, p, 2, 257, 8, 32, 0.1, None) == ERR_UNSUPPORTED and b"256" in lib.stgcn_last_error()
    assert lib.stgcn_vit_attention_backward_bf16(p, p, p, p, 2, 22, 8, 48, 0.1, None) == ERR_UNSUPPORTED
    assert lib.stgcn_vit_attention_backward_bf16(p, p, p, p, 0, 22, 8, 32, 0.1, None) == ERR_ARG


# ---- the switch -------------------------------------------------------------------------------------------------------------------
def test_switch_env_precedence_and_flag_words(monkeypatch):
    import stgcn_amd
    from stgcn_amd import _capi, altformer
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH, HEAD_TRAIN_MATH, Block, set_head_math, set_low_latency, set_train_attention_math, \
        set_train_math
    assert stgcn_amd.set_train_attention_math is set_train_attention_math and "set_train_attention_math" in stgcn_amd.__all__
    assert "attn" not in " ".join(HEAD_TRAIN_MATH) and all(v & BIT == 0 for v in HEAD_TRAIN_MATH.values()), "set_train_math is not touched"
    m = BIT | _capi.VIT_TRAIN_BF16 | _capi.MATH_BF16X3 | _capi.VIT_QKV_F32
    assert F._vit_train_flags(m) == m and F._vit_flags(m) == m & ~(BIT | _capi.VIT_TRAIN_BF16)
    assert F._vit_train_flags(m | 0x1000000) == m, "unknown bits are still dropped"
    monkeypatch.delenv("STGCN_VIT_TRAIN_ATTENTION", raising=False)
    monkeypatch.delenv("STGCN_VIT_TRAIN_MATH", raising=False)
    monkeypatch.delenv("STGCN_VIT_MATH", raising=False)

    torch.manual_seed(0)
    holder = torch.nn.Sequential(Block(64, 2), Block(64, 2))
    assert all(b.train_attention_mode is None for b in holder)
    set_train_attention_math(holder, "bf16")
    assert all(b.train_attention_mode == "bf16" and b.train_math_mode is None and b.math_mode is None for b in holder)
    set_train_attention_math(holder, None)
    assert all(b.train_attention_mode is None for b in holder)
    for bad in ("fp8", "BF16", 1):
        with pytest.raises(KeyError):
            set_train_attention_math(holder, bad)

    blk, x = holder[0], torch.zeros(1, 3, 64)
    words = []

    def word():
        words.append(blk._hip_flags(x, train=True))
        return words[-1]
    MODE = HEAD_TRAIN_MATH["bf16"]
    assert word() == _capi.MATH_F32, "unset: the flag word of today"
    monkeypatch.setenv("STGCN_VIT_TRAIN_ATTENTION", "bf16")
    assert word() == _capi.MATH_F32 | BIT, "the environment"
    set_train_attention_math(blk, "f32")
    assert word() == _capi.MATH_F32, "the attribute wins over the environment"
    monkeypatch.setenv("STGCN_VIT_TRAIN_ATTENTION", "BF16")
    set_train_attention_math(blk, None)
    assert word() == _capi.MATH_F32 | BIT, "None restores; the value is case-insensitive"
    monkeypatch.setenv("STGCN_VIT_TRAIN_ATTENTION", "fp8")
    with pytest.raises(KeyError):
        word()
    monkeypatch.delenv("STGCN_VIT_TRAIN_ATTENTION")
    set_train_attention_math(blk, "bf16")
    set_train_math(blk, "bf16")
    assert word() == MODE | BIT, "the intended use: both switches"
    set_train_math(blk, "bf16x3")
    assert word() == _capi.MATH_BF16X3 | BIT
    set_train_math(blk, None)
    set_head_math(blk, "mixed")
    assert word() == HEAD_MATH["mixed"] | BIT
    set_head_math(blk, "bf16")
    assert word() == _capi.MATH_F32 | BIT, "the inference mode: training in its path's default, plus the bit"
    # inference flags never carry the bit
    for mode in (None, "f32", "mixed", "bf16"):
        set_head_math(blk, mode)
        for low_latency in (False, True):
            set_low_latency(blk, low_latency)
            assert blk._hip_flags(x, train=False) & BIT == 0
    set_low_latency(blk, False)
    set_head_math(blk, None)

    # what reaches the training entry point, and that the second block (switch unset) sends today's word
    seen = []
    monkeypatch.setattr(Block, "uses_hip", lambda self, x: False)
    monkeypatch.setattr(Block, "trains_on_hip", lambda self, x: True)

    class Spy:
        @staticmethod
        def apply(x, s1, s2, heads, eps, scale, math, *params):
            seen.append(math)
            return x
    monkeypatch.setattr(altformer, "_BlockTrain", Spy)
    set_train_math(holder, "bf16")
    holder(x)
    set_train_attention_math(holder, "bf16")
    holder(x)
    set_train_attention_math(holder, None)
    set_train_math(holder, None)
    holder(x)
    assert seen == [MODE | BIT, MODE, MODE | BIT, MODE | BIT, _capi.MATH_F32, _capi.MATH_F32]
