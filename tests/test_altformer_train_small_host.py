"""Host tests (no GPU) of the small training calls of the heads' blocks: the flag ``STGCN_VIT_WGRAD_SMALL`` and where it is
legal, the three queries of the weight gradient's plan (form, splits, direct stores) against the rule restated here, the
workspace queries, and the modules' switch (``set_low_latency_training(model)``)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
NEW_NAMES = ("stgcn_vit_wgrad_tile", "stgcn_vit_wgrad_splits", "stgcn_vit_wgrad_writes_direct",
             "stgcn_vit_block_train_small_ws_bytes", "stgcn_vit_linear_backward_small_ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import stgcn_amd
    return stgcn_amd.lib()


def cd(a, b):
    return -(-a // b)


def parent_splits(M, K, Nout):
    """wgrad_rows_per_split of the parent commit, restated: about 512 workgroups of 128 x 128 tiles, a split at least 256
    tokens long, ranges multiples of the chunk of 32."""
    tiles = cd(Nout, 128) * cd(K, 128)
    splits = min(cd(512, tiles), cd(M, 256))
    rps = cd(cd(M, splits), 32) * 32
    return cd(M, rps)


def workgroups(tile, splits, K, Nout):
    return cd(Nout, tile) * cd(K, tile) * splits


def block_products(D, hidden):
    return ((D, 3 * D), (D, D), (D, hidden), (hidden, D))   # (K, Nout) of qkv, proj, fc1, fc2


# the block shapes of both heads (22 or 46 joints, 180 frames; D = 256 and 512 at hidden = 2 D) at batch 1, 2, 16 and 32:
# the first stage has batch * frames (or joints) sequences, the second batch
HEAD_TOKENS = sorted({b * t * v for b in (1, 2, 16, 32) for t, v in ((180, 22), (180, 46))} | {b * n for b in (1, 2, 16, 32) for n in (22, 46, 180)})
GRID = [(M, K, N) for M in HEAD_TOKENS + [1, 31, 32, 33, 255, 256, 257, 333, 704, 1472, 5760, 13200] for D in (256, 512)
        for K, N in block_products(D, 2 * D)] + [(M, K, N) for M in (1, 70, 333, 5000) for K, N in ((32, 4), (96, 100), (160, 196), (2048, 1024))]


# ---- 1. the C ABI -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_documented_and_the_abi_is_still_11(lib):
    from stgcn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW_NAMES:
        m = re.search(rf"\b(int|size_t)\s+{n}\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        res, args = _capi.PROTOTYPES[n]
        assert res is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t), n
        want = [ctypes.c_uint if a.strip().startswith("unsigned") else ctypes.c_int for a in m.group(2).split(",")]
        assert args == want, (n, m.group(2))
        assert hasattr(lib, n) and n in doc, n
    assert re.search(r"#define\s+STGCN_VIT_WGRAD_SMALL\s+\(?0x10000000u\)?", hdr) and _capi.VIT_WGRAD_SMALL == 0x10000000
    assert "STGCN_VIT_WGRAD_SMALL" in doc
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11


def test_the_flag_is_a_bit_of_its_own(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    bit = _capi.VIT_WGRAD_SMALL
    assert bit and bit & (bit - 1) == 0
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    for name, val in re.findall(r"#define\s+(STGCN_(?:VIT|MATH|IN|OUT|EMBED|BN|STEM|CONV|RAW)\w*)\s+\(?(0x[0-9A-Fa-f]+)u\)?", hdr):
        if name != "STGCN_VIT_WGRAD_SMALL":
            assert int(val, 16) & bit == 0, name
    assert (_capi.VIT_TRAIN_BF16 << 2) & bit == 0 and _capi.MATH_MASK & bit == 0 and _capi.VIT_TILE_MASK & bit == 0
    for n in dir(_capi):
        if n.isupper() and isinstance(getattr(_capi, n), int) and n not in ("VIT_WGRAD_SMALL", "ABI_VERSION"):
            assert getattr(_capi, n) & bit == 0, n
    # the word of the older pair never carries it; the _drop pair's does; the two unknown bits are still dropped
    assert F._vit_train_flags(bit | 0x400000 | 0x1000000) == 0
    assert F._vit_train_flags(bit | 0x400000 | 0x1000000 | _capi.VIT_TILE_AUTO, small=True) == bit | _capi.VIT_TILE_AUTO


def test_who_refuses_the_flag_and_who_reads_it(lib):
    from stgcn_amd._capi import MATH_BF16X3, VIT_TILE_AUTO, VIT_TRAIN_BF16, VIT_WGRAD_SMALL as S
    calls = {
        b"stgcn_vit_block_forward:": lambda fl: lib.stgcn_vit_block_forward(*([None] * 13), 1e-5, 0.1, None, 0, None, 2, 100, 512, 8, 512, fl, None),
        b"stgcn_vit_block_forward_train:": lambda fl: lib.stgcn_vit_block_forward_train(*([None] * 15), 1e-5, 0.1, None, 0, None, 2, 100, 512, 8, 512, fl, None),
        b"stgcn_vit_block_backward:": lambda fl: lib.stgcn_vit_block_backward(*([None] * 12), 0, *([None] * 14), 1e-5, 0.1, None, 0, 2, 100, 512, 8, 512, fl, None),
    }
    for name, call in calls.items():
        for fl in (S, S | MATH_BF16X3):
            assert call(fl) == ERR_ARG
            msg = lib.stgcn_last_error()
            assert name in msg and b"STGCN_VIT_WGRAD_SMALL" in msg, msg
        assert call(0) == ERR_ARG and b"STGCN_VIT_WGRAD_SMALL" not in lib.stgcn_last_error()
    past = {
        b"stgcn_vit_block_forward_train_drop:": lambda fl: lib.stgcn_vit_block_forward_train_drop(None, None, None, None, None, 1e-5, 0.1, None, 0, None, 2, 100, 512, 8, 512, fl, None),
        b"stgcn_vit_block_backward_drop:": lambda fl: lib.stgcn_vit_block_backward_drop(None, None, None, None, None, None, 0, None, None, None, 1e-5, 0.1, None, 0, 2, 100, 512, 8, 512, fl, None),
        b"stgcn_vit_linear_backward:": lambda fl: lib.stgcn_vit_linear_backward(*([None] * 8), 0, 64, 64, 64, fl, None),
    }
    for name, call in past.items():
        for fl in (S, S | VIT_TRAIN_BF16 | MATH_BF16X3) + ((S | VIT_TILE_AUTO,) if b"block" in name else ()):
            assert call(fl) == ERR_ARG
            msg = lib.stgcn_last_error()
            assert name in msg and b"null" in msg.lower() and b"WGRAD_SMALL" not in msg, (hex(fl), msg)   # stopped by the pointers


# ---- 2. the plan's queries --------------------------------------------------------------------------------------------------
def test_without_the_flag_the_queries_answer_the_parents_rule(lib):
    for M, K, N in GRID:
        assert lib.stgcn_vit_wgrad_tile(M, K, N, 0) == 128, (M, K, N)
        assert lib.stgcn_vit_wgrad_splits(M, K, N, 0) == parent_splits(M, K, N), (M, K, N)
        assert lib.stgcn_vit_wgrad_writes_direct(M, K, N, 0) == 0, "calls without the flag keep their summing launches"
    from stgcn_amd._capi import VIT_TILE_AUTO, VIT_TRAIN_BF16
    assert lib.stgcn_vit_wgrad_tile(704, 512, 512, VIT_TILE_AUTO | VIT_TRAIN_BF16) == 128, "only the flag itself is read"
    assert lib.stgcn_vit_wgrad_tile(0, 512, 512, 0) == 0 and lib.stgcn_vit_wgrad_splits(5, 0, 512, 0) == 0


def test_with_the_flag(lib):
    from stgcn_amd import functional as F
    from stgcn_amd._capi import VIT_WGRAD_SMALL as S
    forms = set()
    for M, K, N in GRID:
        tile, splits, direct = F.vit_wgrad_plan(M, K, N, S)
        forms.add(tile)
        chunks = cd(M, 32)
        assert tile in (128, 64) and 1 <= splits <= chunks, (M, K, N)   # whole chunks of 32 tokens, no empty range
        if tile == 64:
            assert splits == 1 or chunks // splits >= 4, "a split of the small form is at least 4 chunks long"
        unflagged = workgroups(128, parent_splits(M, K, N), K, N)
        assert workgroups(tile, splits, K, N) >= unflagged, (M, K, N)
        if unflagged >= 256:
            assert tile == 128, (M, K, N)
        assert direct is (splits == 1), (M, K, N)
    assert forms == {128, 64}
    assert F.vit_wgrad_plan(704, 512, 512, S) == (64, 4, False), "the TS spatial stage's proj product: 256 workgroups for 48"
    assert F.vit_wgrad_plan(704, 512, 1536, S) == (64, 1, True)
    assert F.vit_wgrad_plan(126720, 512, 512, S)[0] == 128 and F.vit_wgrad_plan(126720, 256, 768, S)[0] == 128


@pytest.mark.parametrize("D", [256, 512])
def test_the_workgroup_count_never_falls_as_the_tokens_grow(D, lib):
    from stgcn_amd._capi import VIT_WGRAD_SMALL as S
    for K, N in block_products(D, 2 * D) + ((96, 100), (160, 196)):
        last = 0
        for M in range(1, 40000, 97):
            n = workgroups(lib.stgcn_vit_wgrad_tile(M, K, N, S), lib.stgcn_vit_wgrad_splits(M, K, N, S), K, N)
            assert n >= last, (M, K, N, last, n)
            last = n


# ---- 3. workspaces ----------------------------------------------------------------------------------------------------------
def test_workspace_queries(lib):
    from stgcn_amd._capi import VIT_WGRAD_SMALL as S
    grew = 0
    for B, L, D, heads, hidden in ((1, 180, 512, 8, 1024), (2, 22, 256, 8, 512), (32, 22, 512, 8, 1024), (32, 180, 512, 8, 1024),
                                   (704, 180, 256, 8, 512), (1, 240, 256, 8, 512), (3, 300, 256, 8, 512), (0, 22, 256, 8, 512), (2, 22, 384, 8, 512)):
        old = lib.stgcn_vit_block_train_drop_ws_bytes(B, L, D, heads, hidden)
        assert lib.stgcn_vit_block_train_small_ws_bytes(B, L, D, heads, hidden, 0) == old
        new = lib.stgcn_vit_block_train_small_ws_bytes(B, L, D, heads, hidden, S)
        assert new >= old and (new > 0) == (old > 0)
        grew += new > old
    assert grew, "more splits need more slab space somewhere"
    for M, K, N in ((1, 32, 4), (704, 512, 512), (333, 160, 196), (5, 48, 4)):
        old = lib.stgcn_vit_linear_backward_ws_bytes(M, K, N)
        assert lib.stgcn_vit_linear_backward_small_ws_bytes(M, K, N, 0) == old
        assert lib.stgcn_vit_linear_backward_small_ws_bytes(M, K, N, S) >= old


def test_an_entry_point_checks_the_workspace_of_its_own_flags(lib):
    """Fake non-null host pointers that no launch ever sees: the answer comes before the first one."""
    from stgcn_amd import _capi
    S = _capi.VIT_WGRAD_SMALL
    buf = (ctypes.c_float * 64)()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ctypes.byref(buf, 16), ctypes.c_void_p)
    w, g = _capi.VitBlockWeights(), _capi.VitBlockGrads()
    for s in (w, g):
        for f, _ in s._fields_:
            setattr(s, f, p)
    B, L, D, heads, hidden = 1, 240, 256, 8, 512   # one split of every product without the flag, two of the qkv product with it
    saved = lib.stgcn_vit_block_train_long_saved_bytes(B, L, D, hidden)
    old, new = lib.stgcn_vit_block_train_drop_ws_bytes(B, L, D, heads, hidden), lib.stgcn_vit_block_train_small_ws_bytes(B, L, D, heads, hidden, S)
    assert new > old
    for fl in (S, S | _capi.VIT_TILE_AUTO, S | _capi.VIT_TRAIN_BF16 | _capi.MATH_BF16X3 | _capi.VIT_QKV_F32):
        for short in (new - 1, old):
            rc = lib.stgcn_vit_block_backward_drop(p, ctypes.byref(w), None, None, None, p, saved, p, q, ctypes.byref(g), 1e-5, 0.1, p,
                                                   short, B, L, D, heads, hidden, fl, None)
            assert rc == ERR_WORKSPACE and f"< {new} bytes".encode() in lib.stgcn_last_error(), hex(fl)
    M, K, N = 704, 512, 512
    need = lib.stgcn_vit_linear_backward_small_ws_bytes(M, K, N, S)
    assert need > lib.stgcn_vit_linear_backward_ws_bytes(M, K, N)
    rc = lib.stgcn_vit_linear_backward(p, p, p, None, q, p, p, p, need - 1, M, K, N, S, None)
    assert rc == ERR_WORKSPACE and f"< {need} bytes".encode() in lib.stgcn_last_error()


# ---- 4. the modules ---------------------------------------------------------------------------------------------------------
def test_the_switch_and_the_flag_word():
    import stgcn_amd
    from stgcn_amd import altformer
    from stgcn_amd._capi import VIT_TILE_AUTO, VIT_TILE_MASK, VIT_TRAIN_ATTN_BF16, VIT_TRAIN_BF16, VIT_WGRAD_SMALL
    from stgcn_amd.altformer import (HIP_TRAIN_MIN_TOKENS, LOW_LATENCY_TRAIN_MIN_TOKENS, Block, set_low_latency,
                                     set_low_latency_training, set_train_attention_math, set_train_math)
    assert stgcn_amd.VIT_WGRAD_SMALL == VIT_WGRAD_SMALL and stgcn_amd.LOW_LATENCY_TRAIN_MIN_TOKENS == LOW_LATENCY_TRAIN_MIN_TOKENS
    assert {"VIT_WGRAD_SMALL", "LOW_LATENCY_TRAIN_MIN_TOKENS", "set_low_latency_training"} <= set(stgcn_amd.__all__)
    assert stgcn_amd.set_low_latency_training is set_low_latency_training
    assert 0 <= LOW_LATENCY_TRAIN_MIN_TOKENS <= HIP_TRAIN_MIN_TOKENS == 13200
    model = torch.nn.Sequential(Block(256, 8, mlp_ratio=2., qkv_bias=True), Block(256, 8, mlp_ratio=2., qkv_bias=True))
    blk = model[0]
    x = torch.zeros(2, 22, 256)
    small = VIT_TILE_MASK | VIT_WGRAD_SMALL
    assert blk.small_tiles_train is False and blk._hip_flags(x, train=True) & small == 0
    set_low_latency(model)
    assert all(b.small_tiles and b.small_tiles_train is False and b.hip_train_min_tokens == HIP_TRAIN_MIN_TOKENS for b in model)
    assert blk._hip_flags(x, train=True) & small == 0, "small_tiles alone: a training word without a tile field"
    set_low_latency(model, min_tokens=0, split_attention=True)
    assert all(b.small_tiles_train is False and b.hip_train_min_tokens == HIP_TRAIN_MIN_TOKENS for b in model)
    set_low_latency_training(model)
    assert all(b.small_tiles_train is True and b.hip_train_min_tokens == LOW_LATENCY_TRAIN_MIN_TOKENS for b in model)
    base = blk._train_flags()
    assert blk._hip_flags(x, train=True) == base | VIT_TILE_AUTO | VIT_WGRAD_SMALL
    assert blk._hip_flags(x, train=False) & VIT_WGRAD_SMALL == 0, "the inference word never carries it"
    set_train_math(model, "bf16")
    set_train_attention_math(model, "bf16")
    assert blk._hip_flags(x, train=True) == altformer.HEAD_TRAIN_MATH["bf16"] | VIT_TRAIN_ATTN_BF16 | VIT_TILE_AUTO | VIT_WGRAD_SMALL
    assert blk._hip_flags(x, train=True) & VIT_TRAIN_BF16
    set_train_math(model, None)
    set_train_attention_math(model, None)
    set_low_latency_training(model, train_min_tokens=0)
    assert all(b.hip_train_min_tokens == 0 for b in model)
    set_low_latency(model, enabled=False)
    assert all(b.small_tiles_train is False and not b.small_tiles and b.hip_train_min_tokens == HIP_TRAIN_MIN_TOKENS for b in model)
    assert blk._hip_flags(x, train=True) & small == 0
    set_low_latency(model)
    set_low_latency_training(model, train_min_tokens=5)
    set_low_latency_training(model, False)
    assert all(b.small_tiles_train is False and b.small_tiles and b.hip_train_min_tokens == HIP_TRAIN_MIN_TOKENS for b in model), \
        "the training switch goes back on its own and leaves the inference one"


def test_the_stvit_layer_has_the_switch_too():
    from stgcn_amd import vit
    from stgcn_amd._capi import VIT_TILE_AUTO, VIT_TILE_MASK, VIT_WGRAD_SMALL
    from stgcn_amd.altformer import set_low_latency, set_low_latency_training
    net = vit.Transformer(64, 2, 2, 32, 128)
    layers = [m for m in net.modules() if isinstance(m, vit.Layer)]
    assert layers and all(m.small_tiles_train is False for m in layers)
    words = [m._train_flags(tiles=True) for m in layers]
    assert all(w & VIT_WGRAD_SMALL == 0 for w in words), "the default word does not move"
    keep = [m.hip_train_min_tokens for m in layers]
    set_low_latency_training(net, train_min_tokens=7)
    assert all(m.small_tiles_train and m.hip_train_min_tokens == 7 for m in layers)
    assert all(m._train_flags(tiles=True) & (VIT_TILE_MASK | VIT_WGRAD_SMALL) == VIT_TILE_AUTO | VIT_WGRAD_SMALL for m in layers)
    assert all(m._train_flags() & VIT_WGRAD_SMALL == 0 for m in layers), "the patch embedding's word never carries it"
    set_low_latency(net, enabled=False)
    assert [m._train_flags(tiles=True) for m in layers] == words and [m.hip_train_min_tokens for m in layers] == keep


def test_trains_on_hip_at_704_tokens_needs_a_device():
    """``trains_on_hip`` asks for a CUDA tensor before anything else (the existing host tests query it on the CPU only to see it
    answer False), so the threshold's effect is asserted here on the one term that does not need a device; the GPU tests hold
    the whole predicate at 704 tokens."""
    from stgcn_amd.altformer import Block, set_low_latency_training
    blk = Block(512, 8, mlp_ratio=2., qkv_bias=True)
    x = torch.zeros(32, 22, 512, requires_grad=True)
    set_low_latency_training(blk, train_min_tokens=0)
    assert x.shape[0] * x.shape[1] == 704 >= blk.hip_train_min_tokens
    assert not blk.trains_on_hip(x), "a CPU tensor trains on torch ops"
