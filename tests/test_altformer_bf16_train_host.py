"""The heads' bf16 TRAINING mode (``STGCN_VIT_TRAIN_BF16``), host side (no GPU): the additive C ABI (one flag bit, two queries,
ABI 11 unchanged), the unchanged answers of every older query with and without the bit, the argument errors reached before any
launch, the Python switch (``set_train_math`` / ``Block.train_math_mode`` / env ``STGCN_VIT_TRAIN_MATH``), and the fp64
emulation the GPU tests compare against (tests/altformer_bf16_train_ref.py) held to fp64 autograd."""
import ctypes
import importlib.util
import json
import os
import re

import pytest
import torch

import altformer_bf16_train_ref as br
import altformer_ref as ar
import altformer_train_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["stgcn_vit_block_train_bf16_supported", "stgcn_vit_linear_backward_bf16_supported"]
BIT = 0x200000
ERR_ARG, ERR_UNSUPPORTED = -1, -2
STAGES = ((22, 256, 512), (150, 512, 1024), (180, 512, 1024), (180, 256, 512), (46, 512, 1024), (22, 512, 1024))


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


def test_flag_value_prototypes_and_no_collision(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(STGCN_\w+)\s+0x([0-9A-Fa-f]+)u\b", hdr)}
    assert defs["STGCN_VIT_TRAIN_BF16"] == BIT == _capi.VIT_TRAIN_BF16 == F.VIT_TRAIN_BF16
    old = {k: v for k, v in defs.items() if k != "STGCN_VIT_TRAIN_BF16"}
    assert len(old) >= 18, "the header's flag definitions were not found"
    for k, v in old.items():
        assert BIT & v == 0, f"STGCN_VIT_TRAIN_BF16 collides with {k}"
    assert BIT == 2 * max(v for k, v in old.items() if k.startswith("STGCN_VIT_")), "the next free bit"
    assert all(BIT & v == 0 for k, v in vars(_capi).items() if k.isupper() and isinstance(v, int) and k not in
               ("VIT_TRAIN_BF16", "ABI_VERSION"))
    handle = ctypes.CDLL(build())
    for n in NEW_NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
    assert _capi.PROTOTYPES["stgcn_vit_block_train_bf16_supported"] == (ctypes.c_int, [ctypes.c_int] * 4)
    assert _capi.PROTOTYPES["stgcn_vit_linear_backward_bf16_supported"] == (ctypes.c_int, [ctypes.c_int] * 3)
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11


def test_the_two_new_queries(lib):
    from stgcn_amd import functional as F
    for L, D, hidden in STAGES:
        assert lib.stgcn_vit_block_train_bf16_supported(L, D, 8, hidden) == 1 and F.vit_block_train_bf16_supported(L, D, 8, hidden)
    for L in (1, 256, 257, 300, 4096, 4097, 0):       # the streaming lengths are covered: the coverage of the training plan
        for D, heads, hidden in ((256, 8, 512), (512, 8, 1024), (384, 8, 768), (256, 8, 500), (256, 4, 512), (256, 3, 512)):
            assert lib.stgcn_vit_block_train_bf16_supported(L, D, heads, hidden) == \
                lib.stgcn_vit_block_train_long_supported(L, D, heads, hidden), (L, D, heads, hidden)
    assert lib.stgcn_vit_block_train_bf16_supported(300, 256, 8, 512) == 1 and lib.stgcn_vit_block_train_supported(300, 256, 8, 512) == 0
    assert lib.stgcn_vit_block_train_bf16_supported(4097, 256, 8, 512) == 0
    for M in (0, 1, 33, 126720):
        for K in (0, 32, 48, 256, 1024):
            for Nout in (0, 2, 4, 200, 768):
                got = lib.stgcn_vit_linear_backward_bf16_supported(M, K, Nout)
                assert got == lib.stgcn_vit_linear_backward_supported(M, K, Nout, 0) == int(M >= 1 and K >= 32 and K % 32 == 0
                                                                                            and Nout >= 4 and Nout % 4 == 0)
                assert F.vit_linear_backward_bf16_supported(M, K, Nout) is bool(got)


def test_every_old_query_answers_the_same_with_and_without_the_bit(lib):
    """The fixture recorded before the inference bf16 mode still holds; and the queries that take ``flags`` answer with the bit
    set what they answer without it (they read the low math bits and the tile field only)."""
    spec = importlib.util.spec_from_file_location("make_golden_vit_queries",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_vit_queries.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    from stgcn_amd.build import build
    handle = ctypes.CDLL(build())
    with open(os.path.join(ROOT, "tests", "golden", "vit_queries_abi11.json")) as f:
        want = json.load(f)
    assert mk.answers(handle) == want
    for M, K, Nout in ((1, 256, 768), (200, 256, 768), (126720, 512, 256), (33, 32, 4), (5, 48, 4), (5, 64, 6)):
        for low in (0, 1, 2, 3):
            for extra in (0, 0x10000, 0x20000, 0x30000):
                fl = low | extra
                for q in ("stgcn_vit_linear_supported", "stgcn_vit_linear_tile", "stgcn_vit_linear_backward_supported",
                          "stgcn_vit_linear_bf16_supported"):
                    assert getattr(lib, q)(M, K, Nout, fl | BIT) == getattr(lib, q)(M, K, Nout, fl), (q, M, K, Nout, fl)
    for B, L, D, hidden in ((32, 22, 256, 512), (3, 300, 256, 512), (4000, 22, 256, 512)):   # sizes do not depend on the mode
        assert lib.stgcn_vit_block_train_long_saved_bytes(B, L, D, hidden) > 0
        assert lib.stgcn_vit_block_train_long_ws_bytes(B, L, D, 8, hidden) > 0


def test_argument_errors_are_reached_before_any_launch(lib):
    """Null buffers everywhere: a call that got as far as a launch would fault; these return a status and a message."""
    from stgcn_amd._capi import MATH_BF16, MATH_BF16X3, MATH_F32_VALU, VIT_BF16, VIT_TILE_64, VIT_TILE_AUTO

    def fwd_train(fl):
        return lib.stgcn_vit_block_forward_train(*([None] * 15), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, fl, None)

    def bwd(fl):
        return lib.stgcn_vit_block_backward(*([None] * 12), 0, *([None] * 14), 1e-6, 0.1, None, 0, 2, 22, 256, 8, 512, fl, None)

    def lin_bwd(fl):
        return lib.stgcn_vit_linear_backward(*([None] * 8), 0, 44, 256, 512, fl, None)
    for call, name in ((fwd_train, b"forward_train"), (bwd, b"block_backward"), (lin_bwd, b"linear_backward")):
        assert call(BIT | VIT_BF16) == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error() and name in lib.stgcn_last_error()
        for tile in (VIT_TILE_AUTO, VIT_TILE_64):
            assert call(BIT | tile) == ERR_ARG and b"STGCN_VIT_TILE" in lib.stgcn_last_error()
        assert call(BIT | MATH_BF16X3) == ERR_ARG and b"null" in lib.stgcn_last_error().lower(), "the bit itself is accepted"
    # bad low bits: refused as ever (after the pointer checks, so with buffers that are never touched)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for low in (MATH_BF16, MATH_F32_VALU):
        rc = lib.stgcn_vit_block_forward_train(*([p] * 15), 1e-6, 0.1, p, 0, ctypes.cast(ctypes.byref(buf, 8), ctypes.c_void_p),
                                               2, 22, 256, 8, 512, BIT | low, None)
        assert rc == ERR_UNSUPPORTED and b"math" in lib.stgcn_last_error()
        rc = lib.stgcn_vit_linear_backward(p, p, p, None, None, p, None, p, 0, 44, 256, 512, BIT | low, None)
        assert rc == ERR_UNSUPPORTED and b"math" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_block_forward(*([None] * 13), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, BIT | MATH_BF16X3, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TRAIN_BF16" in lib.stgcn_last_error() and b"stgcn_vit_block_forward:" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_linear(*([None] * 5), 1e-6, None, None, 4, 256, 256, BIT, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TRAIN_BF16" in lib.stgcn_last_error() and b"stgcn_vit_linear:" in lib.stgcn_last_error()


def test_train_math_switch_and_precedence(monkeypatch):
    import stgcn_amd
    from stgcn_amd import _capi, altformer
    from stgcn_amd.altformer import (DEFAULT_TRAIN_MATH, HEAD_MATH, HEAD_TRAIN_MATH, Block, _default_train_math, set_head_math,
                                     set_train_math)
    assert stgcn_amd.set_train_math is set_train_math and "set_train_math" in stgcn_amd.__all__
    assert HEAD_TRAIN_MATH == {"f32": _capi.MATH_F32, "bf16x3": _capi.MATH_BF16X3, "mixed": _capi.MATH_BF16X3 | _capi.VIT_QKV_F32,
                               "bf16": _capi.VIT_TRAIN_BF16 | _capi.MATH_BF16X3 | _capi.VIT_QKV_F32}
    MODE = HEAD_TRAIN_MATH["bf16"]
    assert MODE == HEAD_MATH["mixed"] | BIT, "the bit on top of 'mixed': the qkv forward in f32 (DESIGN section 15, bf16)"
    assert all(HEAD_TRAIN_MATH[k] == HEAD_MATH[k] for k in ("f32", "bf16x3", "mixed")) and DEFAULT_TRAIN_MATH == "f32"
    monkeypatch.delenv("STGCN_VIT_TRAIN_MATH", raising=False)
    assert _default_train_math() == _capi.MATH_F32
    for value in ("bf16", "BF16"):
        monkeypatch.setenv("STGCN_VIT_TRAIN_MATH", value)
        assert _default_train_math() == MODE
    monkeypatch.delenv("STGCN_VIT_TRAIN_MATH")

    torch.manual_seed(0)
    holder = torch.nn.Sequential(Block(64, 2), Block(64, 2))
    assert all(b.train_math_mode is None for b in holder)
    set_head_math(holder, "bf16")
    assert all(b.train_math_mode is None and b.math_mode == _capi.VIT_BF16 for b in holder), "set_head_math leaves it alone"
    set_train_math(holder, "bf16")
    assert all(b.train_math_mode == MODE and b.math_mode == _capi.VIT_BF16 for b in holder)
    set_train_math(holder, _capi.MATH_F32 | BIT)
    assert holder[1].train_math_mode == BIT
    set_train_math(holder, None)
    set_head_math(holder, None)
    assert all(b.train_math_mode is None and b.math_mode is None for b in holder)
    with pytest.raises(KeyError):
        set_train_math(holder, "fp8")

    # what reaches the training entry point: the attribute, else math_mode, else the environment, else the default
    blk = holder[0]
    seen = []
    monkeypatch.setattr(Block, "uses_hip", lambda self, x: False)
    monkeypatch.setattr(Block, "trains_on_hip", lambda self, x: True)

    class Spy:
        @staticmethod
        def apply(x, s1, s2, heads, eps, scale, math, *params):
            seen.append(math)
            return x
    monkeypatch.setattr(altformer, "_BlockTrain", Spy)
    x = torch.zeros(1, 3, 64)
    blk(x)
    monkeypatch.setenv("STGCN_VIT_TRAIN_MATH", "bf16")
    blk(x)
    set_head_math(blk, "mixed")
    blk(x)
    set_head_math(blk, "bf16")          # the inference mode: training falls back to the default of its path
    blk(x)
    set_train_math(blk, "bf16x3")
    blk(x)
    monkeypatch.delenv("STGCN_VIT_TRAIN_MATH")
    set_train_math(blk, "bf16")
    blk(x)
    set_train_math(blk, None)
    blk(x)
    assert seen == [_capi.MATH_F32, MODE, HEAD_MATH["mixed"], MODE, _capi.MATH_BF16X3, MODE, _capi.MATH_F32]


def test_functional_passes_the_bit_to_the_training_entry_points_only():
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    m = BIT | _capi.MATH_BF16X3 | _capi.VIT_QKV_F32
    assert F._vit_train_flags(m) == m and F._vit_flags(m) == m & ~BIT
    assert F._vit_train_flags(m | 0x400000) == m, "unknown bits are still dropped"


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spatial_case():
    x, sd, dy, scale, s1, s2 = br.case_inputs("st_spatial_L22_D256", True)
    kw = dict(scale=scale, s1=s1, s2=s2)
    return x, sd, dy, kw, tr.grads64(x, sd, dy, **kw), br.grads_bf16(x, sd, dy, **kw)


def test_emulation_stays_within_half_the_gate_of_fp64(spatial_case):
    _, _, _, _, (y64, g64), (ye, ge) = spatial_case
    assert br.max_rel(ye, y64) <= 5e-3
    assert set(ge) == set(g64) and len(ge) == 13
    for k in g64:
        rel = br.max_rel(ge[k], g64[k])
        print(f"st_spatial_L22_D256 with factors d{k}: emulation vs fp64 {rel:.3e}")
        assert rel <= 5e-3, k
    assert br.max_rel(ge["mlp.fc2.bias"], g64["mlp.fc2.bias"]) <= 1e-12, "the bias gradient sums unrounded values"
    assert max(br.max_rel(ge[k], g64[k]) for k in g64) >= 1e-3, "the emulation does round"


@pytest.mark.parametrize("point", ["wgrad_dy", "wgrad_a"])
def test_leaving_out_a_wgrad_rounding_point_is_visible_in_the_l2_ratio(point, spatial_case):
    x, sd, dy, kw, (_, g64), (_, ge) = spatial_case
    _, gs = br.grads_bf16(x, sd, dy, skip=point, **kw)
    k = "attn.proj.weight"
    ratio = br.l2_ratio(gs[k], ge[k], g64[k])
    print(f"without {point}: L2 ratio on d{k} {ratio:.3f}")
    assert ratio > 0.6


def test_emulation_places_the_row_factor_where_the_kernels_do():
    """dgrad: s (r(g) r(W)); wgrad: r(s g)^T r(a); bias: the unrounded s g.  On one linear, against the formulas."""
    g = torch.Generator().manual_seed(3)
    a, W, b = torch.randn(4, 5, 32, generator=g).double(), torch.randn(8, 32, generator=g).double(), torch.randn(8, generator=g).double()
    s = torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 0.0]).double().reshape(4, 1, 1)
    up = torch.randn(4, 5, 8, generator=g).double()
    a_, W_, b_ = (t.clone().requires_grad_(True) for t in (a, W, b))
    br._Linear.apply(a_, W_, b_, s, False, None).backward(up)
    assert torch.equal(a_.grad, (br.r(up) @ br.r(W)) * s)
    assert torch.equal(W_.grad, br.r(up * s).reshape(-1, 8).T @ br.r(a).reshape(-1, 32))
    assert torch.equal(b_.grad, (up * s).reshape(-1, 8).sum(0))
    y = br._Linear.apply(a, W, b, s, False, None)
    assert torch.equal(y, (br.r(a) @ br.r(W).T + b) * s)
    assert torch.equal(br._Linear.apply(a, W, None, None, True, None), a @ W.T), "the qkv forward is unrounded"
