"""Host tests (no GPU) of training the ST-ViT layers on HIP: the C ABI of the two ``_drop`` entry points and their queries,
``Layer.draw_dropout`` on the CPU, the switches, and the fp64 restatement (tests/stvit_train_ref.py) held to the reference's
own gradients (tests/golden/make_golden_stvit_train.py), which pins where a layer's three dropouts sit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import stvit_ref as sr
import stvit_train_ref as vr
from _util import MATH_GATES, gather_flat, load_golden, parity_gate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = MATH_GATES["f32"][0]
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
NEW_NAMES = ("stgcn_vit_block_forward_train_drop", "stgcn_vit_block_backward_drop", "stgcn_vit_block_train_drop_supported",
             "stgcn_vit_block_train_drop_ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import stgcn_amd
    return stgcn_amd.lib()


# ---- 1. the C ABI -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported_and_the_abi_is_still_11(lib):
    from stgcn_amd import _capi
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    handle = ctypes.CDLL(build())
    for n in NEW_NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
        assert n in open(os.path.join(ROOT, "INTEGRATION.md")).read(), n
    assert "stgcn_vit_drop_masks" in hdr and "stgcn_vit_block_grads" in hdr
    assert [f for f, _ in _capi.VitDropMasks._fields_] == ["m_proj", "m_act", "m_fc2"]
    assert [f for f, _ in _capi.VitBlockGrads._fields_] == [f for f, _ in _capi.VitBlockWeights._fields_]
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11


def _structs():
    from stgcn_amd import _capi
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    w, g, m = _capi.VitBlockWeights(), _capi.VitBlockGrads(), _capi.VitDropMasks()
    for s in (w, g, m):
        for f, _ in s._fields_:
            setattr(s, f, p)
    return buf, p, ctypes.cast(ctypes.byref(buf, 16), ctypes.c_void_p), w, g, m


def test_flag_refusals_come_before_the_pointers_and_a_tile_field_is_accepted(lib):
    from stgcn_amd._capi import (MATH_BF16, MATH_BF16X3, VIT_ATTN_SPLIT, VIT_BF16, VIT_QKV_F32, VIT_TILE_32, VIT_TILE_64,
                                 VIT_TILE_AUTO, VIT_TRAIN_ATTN_BF16, VIT_TRAIN_BF16)

    def fwd(fl):
        return lib.stgcn_vit_block_forward_train_drop(None, None, None, None, None, 1e-5, 0.1, None, 0, None, 2, 100, 512, 8, 512, fl, None)

    def bwd(fl):
        return lib.stgcn_vit_block_backward_drop(None, None, None, None, None, None, 0, None, None, None, 1e-5, 0.1, None, 0,
                                                 2, 100, 512, 8, 512, fl, None)
    for call, name in ((fwd, b"stgcn_vit_block_forward_train_drop:"), (bwd, b"stgcn_vit_block_backward_drop:")):
        for legal in (0, MATH_BF16X3, MATH_BF16X3 | VIT_QKV_F32, VIT_TRAIN_BF16 | MATH_BF16X3 | VIT_QKV_F32, VIT_TRAIN_ATTN_BF16,
                      VIT_TILE_AUTO, VIT_TILE_64, VIT_TILE_32, VIT_TILE_AUTO | VIT_TRAIN_BF16 | VIT_TRAIN_ATTN_BF16):
            assert call(legal) == ERR_ARG, hex(legal)
            msg = lib.stgcn_last_error()
            assert name in msg and b"null" in msg.lower(), (hex(legal), msg)       # past the flag check, stopped by the pointers
        assert call(VIT_BF16) == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error() and name in lib.stgcn_last_error()
        assert call(VIT_ATTN_SPLIT) == ERR_ARG and b"STGCN_VIT_ATTN_SPLIT" in lib.stgcn_last_error() and name in lib.stgcn_last_error()
        assert call(VIT_TILE_64 | VIT_BF16) == ERR_ARG and b"STGCN_VIT_BF16" in lib.stgcn_last_error()
    # the older pair keeps its answer to a tile field
    rc = lib.stgcn_vit_block_forward_train(*([None] * 15), 1e-5, 0.1, None, 0, None, 2, 100, 512, 8, 512, VIT_TILE_64, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TILE" in lib.stgcn_last_error() and b"stgcn_vit_block_forward_train:" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_block_backward(*([None] * 12), 0, *([None] * 14), 1e-5, 0.1, None, 0, 2, 100, 512, 8, 512, VIT_TILE_AUTO, None)
    assert rc == ERR_ARG and b"STGCN_VIT_TILE" in lib.stgcn_last_error()
    # after the pointers: coverage, then sizes; host buffers that are never touched
    buf, p, q, w, g, m = _structs()
    W, G, M = ctypes.byref(w), ctypes.byref(g), ctypes.byref(m)
    rc = lib.stgcn_vit_block_forward_train_drop(p, W, None, None, M, 1e-5, 0.1, p, 0, q, 2, 100, 512, 8, 512, MATH_BF16, None)
    assert rc == ERR_UNSUPPORTED and b"math" in lib.stgcn_last_error()
    rc = lib.stgcn_vit_block_forward_train_drop(p, W, None, None, M, 1e-5, 0.1, p, 0, q, 2, 100, 384, 8, 512, VIT_TILE_64, None)
    assert rc == ERR_UNSUPPORTED, "head_dim 48"
    rc = lib.stgcn_vit_block_forward_train_drop(p, W, None, None, M, 1e-5, 0.1, p, 0, p, 2, 100, 512, 8, 512, 0, None)
    assert rc == ERR_ARG and b"alias" in lib.stgcn_last_error()
    odd = ctypes.cast(ctypes.byref(buf, 4), ctypes.c_void_p)
    m.m_fc2 = odd
    saved = lib.stgcn_vit_block_train_long_saved_bytes(2, 100, 512, 512)
    rc = lib.stgcn_vit_block_backward_drop(p, W, None, None, M, p, saved, p, q, G, 1e-5, 0.1, p, 1 << 40, 2, 100, 512, 8, 512, 0, None)
    assert rc == ERR_ARG and b"16-byte" in lib.stgcn_last_error(), "a mask the vector kernel cannot read is refused before any launch"
    m.m_fc2 = p
    for fl in (0, VIT_TILE_AUTO, VIT_TRAIN_BF16 | MATH_BF16X3 | VIT_QKV_F32 | VIT_TILE_32):
        ws = lib.stgcn_vit_block_train_drop_ws_bytes(2, 100, 512, 8, 512)
        rc = lib.stgcn_vit_block_forward_train_drop(p, W, None, None, M, 1e-5, 0.1, p, saved - 1, q, 2, 100, 512, 8, 512, fl, None)
        assert rc == ERR_WORKSPACE and f"< {saved} bytes".encode() in lib.stgcn_last_error()
        rc = lib.stgcn_vit_block_backward_drop(p, W, None, None, M, p, saved, p, q, G, 1e-5, 0.1, p, ws - 1, 2, 100, 512, 8, 512, fl, None)
        assert rc == ERR_WORKSPACE and f"< {ws} bytes".encode() in lib.stgcn_last_error()
        rc = lib.stgcn_vit_block_backward_drop(p, W, None, None, None, p, saved - 1, p, q, G, 1e-5, 0.1, p, ws, 2, 100, 512, 8, 512, fl, None)
        assert rc == ERR_WORKSPACE and b"saved" in lib.stgcn_last_error()


def test_size_queries_answer_for_the_plan(lib):
    from stgcn_amd import functional as F
    ones = 0
    for L in (0, 1, 37, 100, 256, 257, 4096, 4097):
        for D, heads, hidden in ((512, 8, 512), (256, 8, 1024), (256, 8, 256), (384, 8, 768), (256, 8, 500), (256, 3, 512), (8192, 128, 64)):
            got = lib.stgcn_vit_block_train_drop_supported(L, D, heads, hidden)
            assert got == lib.stgcn_vit_block_train_long_supported(L, D, heads, hidden), (L, D, heads, hidden)
            assert F.vit_block_train_drop_supported(L, D, heads, hidden) is bool(got)
            ones += got
            for B in (0, 1, 2, 400):
                ws = lib.stgcn_vit_block_train_drop_ws_bytes(B, L, D, heads, hidden)
                assert ws == lib.stgcn_vit_block_train_long_ws_bytes(B, L, D, heads, hidden)
                assert (ws > 0) == (got == 1 and B >= 1), (B, L, D, heads, hidden)
    assert ones == 6 * 3, "six covered lengths x the three covered (D, heads, hidden) of the grid"


# ---- 2. draw_dropout ------------------------------------------------------------------------------------------------------------------
def _layer(D=64, heads=2, hidden=96, p=0.5, seed=3):
    from stgcn_amd.vit import Attention, FeedForward, Layer, PreNorm
    torch.manual_seed(seed)
    return Layer(PreNorm(D, Attention(D, heads=heads, dim_head=D // heads, dropout=p)), PreNorm(D, FeedForward(D, hidden, dropout=p)))


def _state(layer):
    n1, a, n2, net = layer._parts()
    return {"norm1.weight": n1.weight, "norm1.bias": n1.bias, "attn.qkv.weight": a.to_qkv.weight, "attn.proj.weight": a.to_out[0].weight,
            "attn.proj.bias": a.to_out[0].bias, "norm2.weight": n2.weight, "norm2.bias": n2.bias, "mlp.fc1.weight": net[0].weight,
            "mlp.fc1.bias": net[0].bias, "mlp.fc2.weight": net[3].weight, "mlp.fc2.bias": net[3].bias}


def test_draw_dropout_order_shapes_and_identity_with_the_torch_path():
    layer = _layer().train()
    x = torch.randn(3, 7, 64)
    torch.manual_seed(11)
    masks = layer.draw_dropout(x)
    assert [tuple(m.shape) for m in masks] == [(3, 7, 64), (3, 7, 96), (3, 7, 64)]
    for m in masks:
        assert m.dtype == torch.float32 and set(m.unique().tolist()) == {0.0, 2.0}
    # order and generator calls: the three draws of the torch path, one after the other
    torch.manual_seed(11)
    want = [torch.nn.functional.dropout(torch.ones(3, 7, w), 0.5, True) for w in (64, 96, 64)]
    assert all(torch.equal(a, b) for a, b in zip(masks, want))
    # the masks are the ones the torch path uses under the same seed: its output is layer64 fed those masks, within fp32
    torch.manual_seed(11)
    y = layer(x)
    with torch.no_grad():
        y64 = vr.layer64(x.double(), {k: v.double() for k, v in _state(layer).items()}, masks, heads=2, scale=layer[0].fn.scale)
    print(f"torch path vs layer64 under the drawn masks: {parity_gate(y, y64, REL, 'torch path y'):.3e}")
    wrong = vr.layer64(x.double(), {k: v.detach().double() for k, v in _state(layer).items()}, (masks[2], masks[1], masks[0]),
                       heads=2, scale=layer[0].fn.scale)
    assert (wrong - y64).abs().max() > 0.05 * y64.abs().max(), "the comparison tells the masks' places apart"


def test_draw_dropout_answers_none_without_a_live_dropout_and_zeros_at_p_one():
    x = torch.randn(2, 5, 64)
    layer = _layer().eval()
    state = torch.get_rng_state()
    assert layer.draw_dropout(x) == (None, None, None)
    assert torch.equal(torch.get_rng_state(), state), "nothing is drawn in .eval()"
    assert _layer(p=0.0).train().draw_dropout(x) == (None, None, None)
    layer = _layer().train()
    layer[1].fn.net[2].p = 0.0
    layer[1].fn.net[4].eval()
    m = layer.draw_dropout(x)
    assert m[0] is not None and m[1] is None and m[2] is None
    ones = _layer(p=1.0).train().draw_dropout(x)
    assert all(t is not None and not t.any() and torch.isfinite(t).all() for t in ones), "p == 1: all zeros"


def test_cpu_layers_and_uncovered_layers_do_not_train_on_hip(monkeypatch):
    layer = _layer().train()
    layer.hip_train_min_tokens = 0
    x = torch.randn(2, 5, 64, requires_grad=True)
    assert not layer.trains_on_hip(x) and not layer.uses_hip(x)
    layer(x).sum().backward()
    assert x.grad is not None and all(p.grad is not None for p in layer.parameters())


# ---- 3. the switches ------------------------------------------------------------------------------------------------------------------
def test_training_switches_reach_layers_and_still_reach_blocks(monkeypatch):
    from stgcn_amd import _capi
    from stgcn_amd.altformer import (HEAD_TRAIN_MATH, HIP_TRAIN_MIN_TOKENS, Block, set_hip_min_tokens, set_hip_train_min_tokens,
                                     set_low_latency, set_train_attention_math, set_train_math)
    from stgcn_amd.vit import VIT_HIP_TRAIN_MIN_TOKENS, Layer, ViT
    for k in ("STGCN_VIT_TRAIN_ATTENTION", "STGCN_VIT_TRAIN_MATH", "STGCN_VIT_MATH"):
        monkeypatch.delenv(k, raising=False)
    torch.manual_seed(0)
    vit = ViT(time_len=8, joint=4, p1=4, p2=2, num_classes=3, dim=64, depth=2, heads=2, mlp_dim=64, channels=4, dim_head=32, dropout=0.1)
    net = torch.nn.ModuleList([vit, Block(64, 2)])
    layers, blk = list(vit.transformer.layers), net[1]
    assert all(isinstance(l, Layer) for l in layers) and len(layers) == 2
    assert all(l.hip_train_min_tokens == VIT_HIP_TRAIN_MIN_TOKENS == Layer.DEFAULT_HIP_TRAIN_MIN_TOKENS for l in layers)
    assert blk.hip_train_min_tokens == HIP_TRAIN_MIN_TOKENS
    set_hip_train_min_tokens(net, 7)
    assert all(m.hip_train_min_tokens == 7 for m in layers + [blk]) and blk.hip_min_tokens != 7
    set_hip_min_tokens(net, 0)
    assert all(m.hip_train_min_tokens == 0 and m.hip_min_tokens == 0 for m in layers + [blk])
    set_train_math(net, "bf16")
    assert all(m.train_math_mode == HEAD_TRAIN_MATH["bf16"] for m in layers + [blk])
    set_train_attention_math(net, "bf16")
    assert all(m.train_attention_mode == "bf16" for m in layers + [blk])
    # the words: a Layer's carries VIT_TILE_AUTO where small_tiles is set (its default), a Block's never a tile field
    word = HEAD_TRAIN_MATH["bf16"] | _capi.VIT_TRAIN_ATTN_BF16
    x = torch.zeros(1, 5, 64)
    assert all(l.small_tiles for l in layers) and not blk.small_tiles
    assert all(l._train_flags(tiles=True) == word | _capi.VIT_TILE_AUTO for l in layers)
    set_low_latency(net)
    assert blk.small_tiles and blk._hip_flags(x, train=True) == word
    set_low_latency(net, False)
    layers[0].small_tiles = False
    assert layers[0]._train_flags(tiles=True) == word
    set_train_math(net, None)
    set_train_attention_math(net, None)
    assert all(m.train_math_mode is None and m.train_attention_mode is None for m in layers + [blk])
    assert layers[1]._train_flags(tiles=True) == _capi.MATH_F32 | _capi.VIT_TILE_AUTO and blk._hip_flags(x, train=True) == _capi.MATH_F32


# ---- the restatement against the reference --------------------------------------------------------------------------------------------
def test_restatement_matches_the_reference_training_fixture():
    """stvit_train_ref.vit_train64 (embedding, two layer64 with the fixture's masks, classifier) and its fp64 autograd against
    the reference ViT run in fp64 with its Dropouts replaced by the same masks: fp64 against fp64, so 1e-9 of max|.|."""
    from stgcn_amd.vit import ViT
    ref = load_golden("stvit_train_reference")
    depth = int(ref["depth"])
    assert depth == vr.FIXTURE_DEPTH
    torch.manual_seed(sr.MODEL_SEED)
    model = sr.prepare(ViT(**dict(sr.CONFIG, depth=depth), dropout=0.1, emb_dropout=0.0))
    sd = {k: v.detach().double().requires_grad_(True) for k, v in model.state_dict().items()}
    z = sr.make_input().double().requires_grad_(True)
    masks = [vr.fixture_masks(i) for i in range(depth)]
    assert all(not m[0].any() and set(m[1].unique().tolist()) == {0.0, 2.0} for ms in masks for m in ms)
    logits = vr.vit_train64(z, sd, depth, masks)
    logits.backward(vr.fixture_dlogits().double())
    tol = 1e-9
    parity_gate(logits.detach(), ref["logits"], tol, "logits")
    grads = {"dz": z.grad, **{"d" + k: v.grad for k, v in sd.items()}}
    assert {k[:-len("_absmax")] for k in ref if k.endswith("_absmax")} == set(grads)
    for k, g in grads.items():
        if k in ref:
            parity_gate(g, ref[k], tol, k)
        else:
            parity_gate(gather_flat(g, ref[k + "_idx"].astype(np.int64)), ref[k + "_val"], tol, k)
            assert abs(g.abs().max().item() - float(ref[k + "_absmax"])) <= tol * float(ref[k + "_absmax"]), k
    # a mask moved to another of its layer's places is told apart
    swapped = [(m[2], m[1], m[0]) for m in masks]
    other = vr.vit_train64(z.detach(), {k: v.detach() for k, v in sd.items()}, depth, swapped)
    assert (other - logits.detach()).abs().max() > 1e-3 * logits.detach().abs().max()
