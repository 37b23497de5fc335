"""The heads' bf16 block mode, host side (no GPU): the additive C ABI (new symbols, one new flag bit, ABI 11 unchanged), the
coverage query, the unchanged answers of every query that existed before the mode, the argument errors that are reached
before any launch, and the Python switch (``HEAD_MATH['bf16']``, env ``STGCN_VIT_MATH``)."""
import ctypes
import importlib.util
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["stgcn_vit_block_forward_bf16_supported", "stgcn_vit_linear_bf16_supported", "stgcn_vit_linear_bf16",
             "stgcn_vit_attention_bf16_supported", "stgcn_vit_attention_bf16"]
ERR_ARG, ERR_UNSUPPORTED = -1, -2
# (L, D, hidden) of a block at the six stages of the two heads (heads = 8)
STAGES = ((22, 256, 512), (150, 512, 1024), (180, 512, 1024), (180, 256, 512), (46, 512, 1024), (22, 512, 1024))


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


def test_new_symbols_declared_bound_and_exported(lib):
    from stgcn_amd import _capi
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    handle = ctypes.CDLL(build())
    for n in NEW_NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr)
    assert _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11


def test_flag_bit_value_and_no_collision():
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(STGCN_\w+)\s+0x([0-9A-Fa-f]+)u\b", hdr)}
    assert defs["STGCN_VIT_BF16"] == 0x40000 == _capi.VIT_BF16 == F.VIT_BF16
    assert defs["STGCN_VIT_X_BF16"] == _capi.VIT_X_BF16 and defs["STGCN_VIT_Y_BF16"] == _capi.VIT_Y_BF16
    new = ("STGCN_VIT_BF16", "STGCN_VIT_X_BF16", "STGCN_VIT_Y_BF16")
    old = {k: v for k, v in defs.items() if k not in new and k != "STGCN_VIT_MAX_STREAM_L"}
    assert len(old) >= 15, "the header's flag definitions were not found"
    for n in new:
        assert bin(defs[n]).count("1") == 1, n
        for k, v in old.items():
            assert defs[n] & v == 0, f"{n} collides with {k}"
        assert all(defs[n] != defs[m] for m in new if m != n)


def test_bf16_coverage_query(lib):
    from stgcn_amd import functional as F
    for L, D, hidden in STAGES:
        assert lib.stgcn_vit_block_forward_bf16_supported(L, D, 8, hidden) == 1, (L, D, hidden)
        assert F.vit_block_forward_bf16_supported(L, D, 8, hidden) is True
    assert lib.stgcn_vit_block_forward_bf16_supported(256, 256, 8, 512) == 1
    assert lib.stgcn_vit_block_forward_bf16_supported(257, 256, 8, 512) == 0       # the streaming form is not covered
    assert lib.stgcn_vit_block_forward_supported(257, 256, 8, 512) == 1            # (the fp32 block runs it)
    assert lib.stgcn_vit_block_forward_bf16_supported(22, 384, 8, 768) == 0        # head_dim 48
    assert lib.stgcn_vit_block_forward_bf16_supported(22, 256, 8, 500) == 0        # hidden not a multiple of 64
    assert lib.stgcn_vit_block_forward_bf16_supported(0, 256, 8, 512) == 0
    assert lib.stgcn_vit_attention_bf16_supported(256, 8, 64) == 1 and lib.stgcn_vit_attention_bf16_supported(1, 8, 32) == 1
    assert lib.stgcn_vit_attention_bf16_supported(257, 8, 64) == 0 and lib.stgcn_vit_attention_bf16_supported(22, 8, 48) == 0
    assert lib.stgcn_vit_linear_bf16_supported(1, 256, 768, 0) == 1 and lib.stgcn_vit_linear_bf16_supported(1, 250, 768, 0) == 0


def test_existing_queries_answer_what_they_answered_before_the_mode(lib):
    """tests/golden/vit_queries_abi11.json was recorded from the library of the commit before the mode (make_golden_vit_queries.py),
    over a grid that includes STGCN_MATH_BF16 in the low bits: adding the mode changed none of these answers."""
    spec = importlib.util.spec_from_file_location("make_golden_vit_queries",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_vit_queries.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    from stgcn_amd.build import build
    with open(os.path.join(ROOT, "tests", "golden", "vit_queries_abi11.json")) as f:
        want = json.load(f)
    got = mk.answers(ctypes.CDLL(build()))
    assert set(got) == set(want) and len(want) == 17
    calls = {}
    for q, args in mk.grid():
        calls.setdefault(q, []).append(args)
    for q in want:
        assert len(got[q]) == len(want[q]) == len(calls[q]), q
        for a, g, w in zip(calls[q], got[q], want[q]):
            assert g == w, f"{q}{a}: {g}, before the mode {w}"
    assert any(want["stgcn_vit_linear_supported"]) and any(want["stgcn_vit_block_ws_bytes"]), "the fixture holds covered shapes"
    assert lib.stgcn_vit_linear_supported(1, 256, 768, 2) == 0 and lib.stgcn_vit_linear_tile(200, 256, 768, 2) == 0
    assert lib.stgcn_vit_linear_backward_supported(200, 256, 768, 2) == 0


def test_argument_errors_are_reached_before_any_launch(lib):
    """Null buffers everywhere: a call that got as far as a launch would fault, these return STGCN_ERR_ARG with a message."""
    from stgcn_amd._capi import VIT_BF16, VIT_QKV_F32
    rc = lib.stgcn_vit_block_forward(*([None] * 13), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, VIT_BF16 | VIT_QKV_F32, None)
    assert rc == ERR_ARG and b"STGCN_VIT_QKV_F32" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_block_forward(*([None] * 13), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, VIT_BF16, None)
    assert rc == ERR_ARG and b"null" in lib.stgcn_last_error().lower()
    rc = lib.stgcn_vit_block_forward_train(*([None] * 15), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, VIT_BF16, None)
    assert rc == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error() and b"forward_train" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_block_backward(*([None] * 12), 0, *([None] * 14), 1e-6, 0.1, None, 0, 2, 22, 256, 8, 512, VIT_BF16, None)
    assert rc == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error() and b"block_backward" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_linear_backward(*([None] * 8), 0, 44, 256, 512, VIT_BF16, None)
    assert rc == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error() and b"linear_backward" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_linear_bf16(*([None] * 5), 1e-6, None, None, 4, 256, 256, 0, None)
    assert rc == ERR_ARG and b"null" in lib.stgcn_last_error().lower()
    rc = lib.stgcn_vit_attention_bf16(None, None, 1, 22, 8, 32, 0.1, None)
    assert rc == ERR_ARG


def test_head_math_has_bf16_and_the_env_var_parses(monkeypatch):
    from stgcn_amd import _capi
    from stgcn_amd.altformer import DEFAULT_HEAD_MATH, HEAD_MATH, Block, _default_head_math, set_head_math
    assert HEAD_MATH["bf16"] == _capi.VIT_BF16 and DEFAULT_HEAD_MATH == "mixed"
    assert HEAD_MATH["mixed"] == _capi.MATH_BF16X3 | _capi.VIT_QKV_F32, "the default arithmetic is untouched"
    blk = Block(64, 2)
    set_head_math(blk, "bf16")
    assert blk.math_mode == _capi.VIT_BF16
    set_head_math(blk, None)
    assert blk.math_mode is None
    for value in ("bf16", "BF16"):
        monkeypatch.setenv("STGCN_VIT_MATH", value)
        assert _default_head_math() == HEAD_MATH["bf16"] == 0x40000
    monkeypatch.delenv("STGCN_VIT_MATH")
    assert _default_head_math() == HEAD_MATH["mixed"]


def test_cpu_block_in_bf16_mode_takes_the_torch_path():
    from stgcn_amd.altformer import Block, set_head_math
    torch.manual_seed(0)
    blk = Block(64, 2).eval()
    x = torch.randn(2, 5, 64)
    with torch.no_grad():
        want = blk(x)
        set_head_math(blk, "bf16")
        assert not blk.uses_hip(x) and torch.equal(blk(x), want)
