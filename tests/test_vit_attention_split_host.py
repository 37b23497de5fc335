"""The heads' attention split over key tiles (``STGCN_VIT_ATTN_SPLIT``, ``stgcn_vit_attention_split``), host side (no GPU): the
additive C ABI (one flag bit, two entry points, two queries, ABI 11 unchanged), the plan's answers through
``stgcn_vit_block_attention_form``, the argument errors reached before any launch, and the Python switch
(``set_low_latency(split_attention=True)`` / ``Block.split_attention``)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT = 0x2000000
NEW_NAMES = ["stgcn_vit_attention_split_supported", "stgcn_vit_attention_split", "stgcn_vit_block_attention_form"]
ERR_ARG, ERR_UNSUPPORTED = -1, -2
NONE, RESIDENT, STREAM, RESIDENT_BF16, RESIDENT_SPLIT = 0, 1, 2, 3, 4
D, HEADS, HIDDEN = 512, 8, 1024


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


def test_header_binding_and_library_agree(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    # the value is written in parentheses: tests/test_altformer_bf16_train_host.py takes every bare `0x..u` definition of a
    # STGCN_VIT_* name for a flag older than STGCN_VIT_TRAIN_BF16
    assert re.search(r"#define\s+STGCN_VIT_ATTN_SPLIT\s+\(0x2000000u\)", hdr)
    defs = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(STGCN_\w+)\s+\(?0x([0-9A-Fa-f]+)u\b", hdr)}
    assert defs["STGCN_VIT_ATTN_SPLIT"] == BIT == _capi.VIT_ATTN_SPLIT and len(defs) >= 20
    assert all(BIT & v == 0 for k, v in defs.items() if k != "STGCN_VIT_ATTN_SPLIT"), "collides with a flag of the header"
    assert all(BIT & v == 0 for k, v in vars(_capi).items() if k.isupper() and isinstance(v, int) and k not in
               ("VIT_ATTN_SPLIT", "ABI_VERSION"))
    assert BIT & (0x400000 | 0x1000000) == 0, "the two bits that host tests use as unknown ones stay unassigned"
    handle = ctypes.CDLL(build())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW_NAMES:
        assert re.search(rf"\bint\s+{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
        assert n in integration, n
    P, I, Fl, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint
    assert _capi.PROTOTYPES["stgcn_vit_attention_split_supported"] == (I, [I] * 3)
    assert _capi.PROTOTYPES["stgcn_vit_attention_split"] == (I, [P] * 2 + [I] * 4 + [Fl, P]) == _capi.PROTOTYPES["stgcn_vit_attention"]
    assert _capi.PROTOTYPES["stgcn_vit_block_attention_form"] == (I, [I] * 5 + [U])
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11
    assert callable(F.vit_attention_split) and callable(F.vit_attention_split_supported) and callable(F.vit_block_attention_form)


def test_supported_is_the_resident_coverage(lib):
    from stgcn_amd import functional as F
    for hd in (32, 64):
        for L in (1, 32, 33, 256):
            assert lib.stgcn_vit_attention_split_supported(L, 8, hd) == 1 and F.vit_attention_split_supported(L, 8, hd) is True
        for L in (0, 257):
            assert lib.stgcn_vit_attention_split_supported(L, 8, hd) == 0 and F.vit_attention_split_supported(L, 8, hd) is False
    for hd in (16, 48, 128):
        for L in (1, 32, 33, 256):
            assert lib.stgcn_vit_attention_split_supported(L, 8, hd) == 0
    for L in (0, 1, 180, 256, 257):
        for heads in (0, 1, 8):
            for hd in (16, 32, 48, 64, 128):
                assert lib.stgcn_vit_attention_split_supported(L, heads, hd) == lib.stgcn_vit_attention_supported(L, heads, hd)


def test_entry_point_errors_before_any_launch(lib):
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.stgcn_vit_attention_split(None, None, 2, 180, 8, 64, 0.1, None) == ERR_ARG
    assert b"stgcn_vit_attention_split" in lib.stgcn_last_error()
    assert lib.stgcn_vit_attention_split(p, None, 2, 180, 8, 64, 0.1, None) == ERR_ARG
    assert lib.stgcn_vit_attention_split(None, p, 2, 180, 8, 64, 0.1, None) == ERR_ARG
    assert lib.stgcn_vit_attention_split(p, p, 0, 180, 8, 64, 0.1, None) == lib.stgcn_vit_attention(p, p, 0, 180, 8, 64, 0.1, None) == ERR_ARG
    assert lib.stgcn_vit_attention_split(p, p, 2, 257, 8, 64, 0.1, None) == ERR_UNSUPPORTED and b"256" in lib.stgcn_last_error()
    assert lib.stgcn_vit_attention_split(p, p, 2, 180, 8, 48, 0.1, None) == ERR_UNSUPPORTED


def test_block_attention_form(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F

    def form(B, L, flags, heads=HEADS):
        return lib.stgcn_vit_block_attention_form(B, L, D, heads, HIDDEN, flags)
    for low in (_capi.MATH_F32, _capi.MATH_BF16X3, _capi.MATH_BF16X3 | _capi.VIT_QKV_F32, _capi.VIT_TILE_AUTO | _capi.MATH_BF16X3):
        assert form(1, 180, low) == RESIDENT, "without the flag"
        assert form(1, 180, low | BIT) == RESIDENT_SPLIT and form(2, 180, low | BIT) == RESIDENT_SPLIT
        assert form(1, 22, low | BIT) == RESIDENT and form(1, 32, low | BIT) == RESIDENT, "one key tile: nothing to split"
        assert form(1, 33, low | BIT) == RESIDENT_SPLIT
        assert form(1, 256, low | BIT) == RESIDENT_SPLIT
        assert form(1, 300, low | BIT) == STREAM == form(1, 300, low) and form(1, 257, low | BIT) == STREAM
    # the edge of the constant, read through the query: the largest B that still splits, 1 <= B < 256 / heads
    edge = max(B for B in range(1, 64) if form(B, 180, BIT) == RESIDENT_SPLIT)
    assert all(form(B, 180, BIT) == RESIDENT_SPLIT for B in range(1, edge + 1)), "one threshold, no gaps"
    assert all(form(B, 180, BIT) == RESIDENT for B in (edge + 1, edge + 2, 32, 64, 1000)), "from the constant on: resident"
    assert (edge + 1) * HEADS <= 256, "the constant is at most the CU count"
    assert form(32, 180, BIT) == RESIDENT, "256 pairs"
    # 31 sequences (248 pairs) split with the constant at the CU count and do not once a measurement has lowered it
    assert form(31, 180, BIT) == (RESIDENT_SPLIT if edge >= 31 else RESIDENT)
    assert form(edge, 180, BIT, heads=16) == RESIDENT, "the rule counts pairs, not sequences"
    assert form(1, 180, _capi.VIT_BF16 | BIT) == RESIDENT_BF16 == form(1, 180, _capi.VIT_BF16), "legal with bf16, no effect"
    assert form(1, 180, BIT, heads=7) == NONE and form(1, 180, 0, heads=7) == NONE, "heads that do not divide D"
    assert form(1, 180, BIT, heads=0) == NONE and form(0, 180, BIT) == NONE and form(1, 0, BIT) == NONE
    assert form(1, 180, BIT | _capi.VIT_TRAIN_BF16) == NONE, "refused flags"
    assert form(1, 180, BIT | _capi.MATH_BF16) == NONE, "uncovered low bits"
    assert F.vit_block_attention_form(1, 180, D, HEADS, HIDDEN, BIT) == "resident_split"
    assert F.vit_block_attention_form(1, 180, D, HEADS, HIDDEN) == "resident"
    assert F.vit_block_attention_form(1, 300, D, HEADS, HIDDEN, BIT) == "stream"
    assert F.vit_block_attention_form(1, 180, D, 7, HIDDEN, BIT) is None
    # workspace sizes do not depend on flags at all: the query takes none
    assert lib.stgcn_vit_block_ws_bytes(1, 180, D, HIDDEN) > 0


def test_refusals_by_name_before_the_pointers(lib):
    from stgcn_amd._capi import MATH_BF16X3, VIT_BF16, VIT_QKV_F32, VIT_TILE_64, VIT_TILE_AUTO, VIT_TRAIN_ATTN_BF16, VIT_TRAIN_BF16

    def fwd_train(fl):
        return lib.stgcn_vit_block_forward_train(*([None] * 15), 1e-6, 0.1, None, 0, None, 1, 180, D, HEADS, HIDDEN, fl, None)

    def bwd(fl):
        return lib.stgcn_vit_block_backward(*([None] * 12), 0, *([None] * 14), 1e-6, 0.1, None, 0, 1, 180, D, HEADS, HIDDEN, fl, None)

    def lin_bwd(fl):
        return lib.stgcn_vit_linear_backward(*([None] * 8), 0, 44, 256, 512, fl, None)

    def lin(fl):
        return lib.stgcn_vit_linear(*([None] * 5), 1e-6, None, None, 4, 256, 256, fl, None)
    for call, name in ((fwd_train, b"stgcn_vit_block_forward_train:"), (bwd, b"stgcn_vit_block_backward:"),
                       (lin_bwd, b"stgcn_vit_linear_backward:"), (lin, b"stgcn_vit_linear:")):
        for legal in (0, MATH_BF16X3, MATH_BF16X3 | VIT_QKV_F32):
            assert call(BIT | legal) == ERR_ARG, name
            err = lib.stgcn_last_error()
            assert b"STGCN_VIT_ATTN_SPLIT" in err and name in err, err
        assert call(0) == ERR_ARG and b"STGCN_VIT_ATTN_SPLIT" not in lib.stgcn_last_error(), "without the bit: the pointers"
    # older refusals still answer first
    for call in (fwd_train, bwd, lin_bwd):
        assert call(BIT | VIT_BF16) == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error()
        assert call(BIT | VIT_TILE_64) == ERR_ARG and b"STGCN_VIT_TILE" in lib.stgcn_last_error()
        assert b"STGCN_VIT_ATTN_SPLIT" not in lib.stgcn_last_error()
    assert lin_bwd(BIT | VIT_TRAIN_ATTN_BF16) == ERR_ARG and b"STGCN_VIT_TRAIN_ATTN_BF16" in lib.stgcn_last_error()
    assert lin(BIT | VIT_TRAIN_BF16) == ERR_ARG and b"STGCN_VIT_TRAIN_BF16 " in lib.stgcn_last_error()
    assert lin(BIT | VIT_TRAIN_ATTN_BF16) == ERR_ARG and b"STGCN_VIT_TRAIN_ATTN_BF16" in lib.stgcn_last_error()
    # training flags that are legal for the two block entries do not make the bit legal
    for call in (fwd_train, bwd):
        assert call(BIT | VIT_TRAIN_BF16 | VIT_TRAIN_ATTN_BF16) == ERR_ARG and b"STGCN_VIT_ATTN_SPLIT" in lib.stgcn_last_error()

    # stgcn_vit_block_forward accepts the bit: with NULL pointers the answer is the NULL-pointer error
    def fwd(fl, L=180):
        return lib.stgcn_vit_block_forward(*([None] * 13), 1e-6, 0.1, None, 0, None, 1, L, D, HEADS, HIDDEN, fl, None)
    for legal in (0, MATH_BF16X3, MATH_BF16X3 | VIT_QKV_F32, VIT_TILE_AUTO, VIT_BF16):
        for L in (22, 180, 300):
            assert fwd(BIT | legal, L) == ERR_ARG and b"null pointer" in lib.stgcn_last_error(), lib.stgcn_last_error()
    assert fwd(BIT | VIT_TRAIN_BF16) == ERR_ARG and b"STGCN_VIT_TRAIN_BF16 " in lib.stgcn_last_error()
    assert fwd(BIT | VIT_BF16 | VIT_QKV_F32) == ERR_ARG and b"exclude" in lib.stgcn_last_error()


def test_python_switch_and_flag_words(monkeypatch):
    import inspect

    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import Block, set_head_math, set_low_latency
    monkeypatch.delenv("STGCN_VIT_TRAIN_ATTENTION", raising=False)
    monkeypatch.delenv("STGCN_VIT_TRAIN_MATH", raising=False)
    monkeypatch.delenv("STGCN_VIT_MATH", raising=False)
    sig = inspect.signature(set_low_latency)
    assert list(sig.parameters) == ["module", "enabled", "min_tokens", "split_attention"]
    assert sig.parameters["split_attention"].default is False
    m = BIT | _capi.MATH_BF16X3 | _capi.VIT_QKV_F32 | _capi.VIT_TILE_AUTO
    assert F._vit_flags(m) == m and F._vit_flags(m | 0x400000 | 0x1000000) == m, "the bit goes through, unknown ones do not"

    torch.manual_seed(0)
    model = torch.nn.Sequential(Block(64, 2), Block(64, 2))
    x = torch.zeros(1, 40, 64)
    assert all(b.split_attention is False for b in model)
    modes = (None, "f32", "bf16x3", "mixed", "bf16")

    def words(train):
        out = []
        for mode in modes:
            set_head_math(model, mode)
            out += [b._hip_flags(x, train=train) for b in model]
        set_head_math(model, None)
        return out
    set_low_latency(model)
    before, before_train = words(False), words(True)
    assert all(b.split_attention is False and b.small_tiles for b in model)
    assert all(w & BIT == 0 for w in before + before_train)
    set_low_latency(model, min_tokens=0)
    assert words(False) == before and all(b.split_attention is False for b in model), "the keyword defaults to off"

    set_low_latency(model, min_tokens=0, split_attention=True)
    assert all(b.split_attention is True and b.small_tiles and b.hip_min_tokens == 0 for b in model)
    assert words(False) == [w | BIT for w in before], "the inference word carries the bit and is otherwise what it was"
    assert words(True) == before_train, "the training word never does"
    for b in model:                               # not even from a math_mode that names it
        b.math_mode = _capi.MATH_BF16X3 | BIT
        assert b._hip_flags(x, train=True) & BIT == 0
        b.train_math_mode = _capi.MATH_F32 | BIT
        assert b._hip_flags(x, train=True) & BIT == 0
        b.math_mode = b.train_math_mode = None

    set_low_latency(model, enabled=False, split_attention=True)
    assert all(b.split_attention is False and not b.small_tiles for b in model), "enabled=False clears it"
    assert all(w & BIT == 0 for w in words(False))
    set_low_latency(model, split_attention=True)
    set_low_latency(model)
    assert all(b.split_attention is False for b in model), "a later call without the keyword switches it off again"
