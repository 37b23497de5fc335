"""ctypes binding of libstgcn_hip.so (C ABI declared in include/stgcn_hip.h).

The library is the product: if it is missing or fails to load, every op raises — there is
no CPU or PyTorch fallback behind any entry point.  (Only the AltFormer head modules of
altformer.py carry a torch-op path of their own, for autograd, CPU tensors and uncovered shapes.)
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_float, c_int, c_long, c_longlong, c_size_t, c_uint, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STGCN_LIB") or os.path.join(_HERE, "libstgcn_hip.so")   # STGCN_LIB: diagnostic builds
ABI_VERSION = 11

# stgcn_math / flags (include/stgcn_hip.h)
MATH_F32 = 0
MATH_BF16X3 = 1
MATH_BF16 = 2
MATH_F32_VALU = 3
MATH_MASK = 0xF
OUT_BF16 = 0x10
RAW = 0x20
IN_NTVC = 0x40    # stem entry points: x is (N,T,V,Cin)
OUT_NTVC = 0x80   # stem entry points: out is (N,T,V,C)
EMBED_TS = 0x100  # stgcn_patch_embed: rows ordered (clip, joint, frame)
BN_FROZEN = 0x200  # training entry points: BatchNorm on its running statistics (eval mode under autograd)
STEM_F16MX = 0x400  # stem entry points, with MATH_BF16X3: fp16 x fp16 + two scaled-e4m3 residual products where KF7 covers the shape
CONV_ALONG_V = 0x800  # stgcn_tcn_forward[_packed], MATH_F32_VALU: convolve along the joint axis (Unit2D(dim=3))
VIT_GELU = 0x1000  # stgcn_vit_linear: exact GELU after the bias
VIT_QKV_F32 = 0x2000  # stgcn_vit_block_forward: the qkv linear in f32 whatever the math bits say
VIT_DGELU = 0x4000  # stgcn_vit_linear_backward: dx times GELU'(h_pre)
VIT_ACCUMULATE = 0x8000  # stgcn_vit_linear_backward: dx += instead of dx =
VIT_TILE_MASK = 0x30000  # stgcn_vit_linear / stgcn_vit_block_forward: tile form of the linears (0: 128 x 128)
VIT_TILE_AUTO = 0x10000  # the plan picks by workgroup count (stgcn_vit_linear_tile tells)
VIT_TILE_64 = 0x20000  # force 64 x 64
VIT_TILE_32 = 0x30000  # force the 32-row form (32 x 64)
VIT_BF16 = 0x40000  # stgcn_vit_block_forward: the whole block on bf16 operands (inference, L <= 256); low math bits ignored
VIT_X_BF16 = 0x80000  # stgcn_vit_linear_bf16: x is bf16 storage
VIT_Y_BF16 = 0x100000  # stgcn_vit_linear_bf16: y is bf16 storage
VIT_TRAIN_BF16 = 0x200000  # the three training entry points: every linear product but the qkv forward on bf16 operands
VIT_TRAIN_ATTN_BF16 = 0x800000  # the block's two training entry points: the resident attention forward / backward on bf16 operands
VIT_ATTN_SPLIT = 0x2000000  # stgcn_vit_block_forward: the fp32 resident attention split over key tiles where the launch has few pairs
VIT_POOL_MAX = 0x4000000  # stgcn_vit_pool / stgcn_vit_pool_classify: the maximum over the tokens instead of the mean
VIT_POOL_CLS = 0x8000000  # stgcn_vit_pool / stgcn_vit_pool_classify: token 0 of every sequence (the ViT's class token)
VIT_WGRAD_SMALL = 0x10000000  # stgcn_vit_block_backward_drop / stgcn_vit_linear_backward: every weight gradient picks its form (128 / 64) and cut
MATH_F16MX = MATH_BF16X3 | STEM_F16MX  # as a "math mode" of the modules: bf16x3 everywhere, KF7 in the fused stem

STATUS = {0: "STGCN_OK", -1: "STGCN_ERR_ARG", -2: "STGCN_ERR_UNSUPPORTED",
          -3: "STGCN_ERR_WORKSPACE", -4: "STGCN_ERR_HIP"}

_P = c_void_p


# the three host structs of the whole-head call (include/stgcn_hip.h, "The whole AltFormer head"): device pointers and sizes
class VitBlockWeights(ctypes.Structure):
    _fields_ = [(n, _P) for n in ("norm1_weight", "norm1_bias", "Wqkv", "bqkv", "Wproj", "bproj", "norm2_weight", "norm2_bias",
                                  "W1", "b1", "W2", "b2")]


# the structs of the training pair with dropout (include/stgcn_hip.h, "ViT block: training with dropout")
class VitBlockGrads(ctypes.Structure):
    _fields_ = VitBlockWeights._fields_


class VitDropMasks(ctypes.Structure):
    _fields_ = [(n, _P) for n in ("m_proj", "m_act", "m_fc2")]


class AltformerHeadShape(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("N", "T", "V", "C", "E1", "E2", "heads", "hidden1", "hidden2", "depth1", "depth2", "classes")]


class AltformerHeadWeights(ctypes.Structure):
    _fields_ = [("embed1_weight", _P), ("embed1_bias", _P), ("pos1", _P), ("blocks1", ctypes.POINTER(VitBlockWeights)),
                ("embed2_weight", _P), ("embed2_bias", _P), ("pos2", _P), ("blocks2", ctypes.POINTER(VitBlockWeights)),
                ("head_norm_weight", _P), ("head_norm_bias", _P), ("head_weight", _P), ("head_bias", _P)]


_SHAPE_P = ctypes.POINTER(AltformerHeadShape)
# name -> (restype, argtypes); one entry per symbol declared in include/stgcn_hip.h
PROTOTYPES = {
    "stgcn_version": (c_int, []),
    "stgcn_last_error": (c_char_p, []),
    "stgcn_bn_fold": (c_int, [_P, _P, _P, _P, _P, c_float, _P, _P, c_int, _P]),
    "stgcn_agcn_attention": (c_int, [_P] * 7 + [c_int] * 6 + [_P]),
    "stgcn_agcn_forward": (c_int, [_P] * 16 + [c_int] * 7 + [_P]),
    "stgcn_agcn_attention_kernel_name": (c_char_p, [c_int] * 7),
    "stgcn_agcn_expand_kernel_name": (c_char_p, [c_int] * 7),
    "stgcn_tcn_packed_bytes": (c_size_t, [c_int, c_int, c_int, c_uint]),
    "stgcn_tcn_supported": (c_int, [c_int] * 6 + [c_uint]),
    "stgcn_tcn_kernel_name": (c_char_p, [c_int] * 6 + [c_uint]),
    "stgcn_tcn_pack": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_uint, _P]),
    "stgcn_tcn_forward_packed": (c_int, [_P] * 4 + [c_int] * 7 + [c_uint, _P]),
    "stgcn_tcn_forward": (c_int, [_P] * 5 + [c_int] * 7 + [_P, c_size_t, c_uint, _P]),
    "stgcn_stem_prep_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_uint]),
    "stgcn_stem_supported": (c_int, [c_int] * 6 + [c_uint]),
    "stgcn_stem_prepare": (c_int, [_P] * 11 + [c_int] * 4 + [c_uint, _P]),
    "stgcn_stem_ws_bytes": (c_size_t, [c_int] * 7 + [c_uint]),
    "stgcn_stem_features_used": (c_int, [c_int] * 6 + [c_uint]),
    "stgcn_stem_kernel_name": (c_char_p, [c_int] * 6 + [c_uint]),
    "stgcn_stem_short_tile_blocks": (c_int, [c_int] * 4),
    "stgcn_stem_walk_run": (c_int, [c_int] * 5 + [_P] * 2),
    "stgcn_stem_walk_order": (c_int, [c_int] * 5 + [_P, c_int, _P]),
    "stgcn_stem_attention": (c_int, [_P] * 7 + [c_size_t] + [c_int] * 8 + [c_uint, _P]),
    "stgcn_stem_tail_prepared": (c_int, [_P] * 2 + [c_size_t] + [_P] * 3 + [c_int] * 7 + [c_uint, _P]),
    "stgcn_stem_forward_prepared": (c_int, [_P] * 9 + [c_size_t] + [_P] + [c_int] * 8 + [c_uint, _P]),
    "stgcn_patch_embed": (c_int, [_P] * 5 + [c_int] * 5 + [c_uint, _P]),
    "stgcn_step_stats": (c_int, [_P, c_int, _P, c_int, c_int, c_long, c_long, c_float, _P, _P, _P, c_int, c_int, _P]),
    "stgcn_agcn_train_ws_bytes": (c_size_t, [c_int] * 7),
    "stgcn_agcn_forward_train": (c_int, [_P] * 18 + [c_float, c_float, _P, _P, c_size_t] + [_P] * 4 + [c_int] * 7 + [c_uint, _P]),
    "stgcn_agcn_backward_ws_bytes": (c_size_t, [c_int] * 7),
    "stgcn_agcn_backward_train": (c_int, [_P] * 34 + [_P, c_size_t] + [c_int] * 7 + [c_uint, _P]),
    "stgcn_tcn_train_ws_bytes": (c_size_t, [c_int] * 7 + [c_uint]),
    "stgcn_tcn_forward_train": (c_int, [_P] * 7 + [c_float, c_float, _P, c_size_t] + [_P] * 4 + [c_int] * 7 + [c_uint, _P]),
    "stgcn_tcn_backward_ws_bytes": (c_size_t, [c_int] * 7 + [c_uint]),
    "stgcn_tcn_backward_train": (c_int, [_P] * 13 + [_P, c_size_t] + [c_int] * 7 + [c_uint, _P]),
    "stgcn_st_attention_supported": (c_int, [c_int] * 5),
    "stgcn_st_attention_ws_bytes": (c_size_t, [c_int] * 8),
    "stgcn_st_attention_forward": (c_int, [_P] * 10 + [c_size_t, _P] + [c_int] * 7 + [_P]),
    "stgcn_st_attention_forward_train": (c_int, [_P] * 14 + [c_float, c_float, _P, c_size_t] + [_P] * 6 + [c_int] * 7
                                         + [c_uint, _P]),
    "stgcn_st_attention_backward": (c_int, [_P] * 24 + [c_size_t] + [c_int] * 7 + [c_uint, _P]),
    "stgcn_st_attention_math_supported": (c_int, [c_int] * 5 + [c_uint]),
    "stgcn_st_attention_forward_math": (c_int, [_P] * 10 + [c_size_t, _P] + [c_int] * 7 + [c_uint, _P]),
    "stgcn_wx_product_supported": (c_int, [c_int, c_int, c_longlong, c_uint]),
    "stgcn_wx_product_kernel_name": (c_char_p, [c_int, c_int, c_longlong, c_uint]),
    "stgcn_wx_product_ws_bytes": (c_size_t, [c_int, c_int, c_uint]),
    "stgcn_wx_product": (c_int, [_P] * 6 + [c_size_t] + [c_int] * 3 + [c_longlong, c_int, c_uint, _P]),
    "stgcn_vit_linear_supported": (c_int, [c_int] * 3 + [c_uint]),
    "stgcn_vit_linear_tile": (c_int, [c_int] * 3 + [c_uint]),
    "stgcn_vit_linear": (c_int, [_P] * 5 + [c_float] + [_P] * 2 + [c_int] * 3 + [c_uint, _P]),
    "stgcn_vit_attention_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention": (c_int, [_P] * 2 + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_attention_stream_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention_stream": (c_int, [_P] * 2 + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_block_forward_bf16_supported": (c_int, [c_int] * 4),
    "stgcn_vit_linear_bf16_supported": (c_int, [c_int] * 3 + [c_uint]),
    "stgcn_vit_linear_bf16": (c_int, [_P] * 5 + [c_float] + [_P] * 2 + [c_int] * 3 + [c_uint, _P]),
    "stgcn_vit_attention_bf16_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention_bf16": (c_int, [_P] * 2 + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_block_supported": (c_int, [c_int] * 4),
    "stgcn_vit_block_forward_supported": (c_int, [c_int] * 4),
    "stgcn_vit_block_ws_bytes": (c_size_t, [c_int] * 4),
    "stgcn_vit_block_forward": (c_int, [_P] * 13 + [c_float, c_float, _P, c_size_t, _P] + [c_int] * 5 + [c_uint, _P]),
    "stgcn_vit_linear_backward_supported": (c_int, [c_int] * 3 + [c_uint]),
    "stgcn_vit_linear_backward_ws_bytes": (c_size_t, [c_int] * 3),
    "stgcn_vit_linear_backward": (c_int, [_P] * 8 + [c_size_t] + [c_int] * 3 + [c_uint, _P]),
    "stgcn_vit_attention_backward_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention_backward": (c_int, [_P] * 4 + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_attention_backward_stream_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention_backward_stream_ws_bytes": (c_size_t, [c_int] * 3),
    "stgcn_vit_attention_backward_stream": (c_int, [_P] * 5 + [c_size_t] + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_layernorm_backward_ws_bytes": (c_size_t, [c_int] * 2),
    "stgcn_vit_layernorm_backward": (c_int, [_P] * 3 + [c_float] + [_P] * 5 + [c_size_t, c_int, c_int, _P]),
    "stgcn_vit_block_train_supported": (c_int, [c_int] * 4),
    "stgcn_vit_block_saved_bytes": (c_size_t, [c_int] * 4),
    "stgcn_vit_block_backward_ws_bytes": (c_size_t, [c_int] * 4),
    "stgcn_vit_block_train_long_supported": (c_int, [c_int] * 4),
    "stgcn_vit_block_train_long_saved_bytes": (c_size_t, [c_int] * 4),
    "stgcn_vit_block_train_long_ws_bytes": (c_size_t, [c_int] * 5),
    "stgcn_vit_block_train_bf16_supported": (c_int, [c_int] * 4),
    "stgcn_vit_linear_backward_bf16_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention_train_bf16_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention_train_bf16": (c_int, [_P] * 2 + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_attention_backward_bf16": (c_int, [_P] * 4 + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_block_train_attn_bf16_supported": (c_int, [c_int] * 4),
    "stgcn_vit_attention_split_supported": (c_int, [c_int] * 3),
    "stgcn_vit_attention_split": (c_int, [_P] * 2 + [c_int] * 4 + [c_float, _P]),
    "stgcn_vit_block_attention_form": (c_int, [c_int] * 5 + [c_uint]),
    "stgcn_vit_pool_supported": (c_int, [c_int] * 3),
    "stgcn_vit_pool": (c_int, [_P] * 2 + [c_int] * 3 + [c_uint, _P]),
    "stgcn_vit_pool_classify_supported": (c_int, [c_int] * 4),
    "stgcn_vit_pool_classify": (c_int, [_P] * 3 + [c_float] + [_P] * 3 + [c_int] * 4 + [c_uint, _P]),
    "stgcn_altformer_head_supported": (c_int, [_SHAPE_P, c_uint, c_uint, c_uint]),
    "stgcn_altformer_head_ws_bytes": (c_size_t, [_SHAPE_P, c_uint, c_uint, c_uint]),
    "stgcn_altformer_head_forward": (c_int, [_P, ctypes.POINTER(AltformerHeadWeights), _SHAPE_P] + [c_float] * 4
                                     + [_P, c_size_t, _P] + [c_uint] * 3 + [_P]),
    "stgcn_vit_patch_embed_supported": (c_int, [c_int] * 7 + [c_uint]),
    "stgcn_vit_patch_embed_ws_bytes": (c_size_t, [c_int] * 7 + [c_uint]),
    "stgcn_vit_patch_embed_cut": (c_int, [c_int] * 7 + [c_uint]),
    "stgcn_vit_patch_embed": (c_int, [_P] * 6 + [c_int] * 7 + [_P, c_size_t, c_uint, _P]),
    "stgcn_vit_block_forward_train": (c_int, [_P] * 15 + [c_float, c_float, _P, c_size_t, _P] + [c_int] * 5 + [c_uint, _P]),
    "stgcn_vit_block_backward": (c_int, [_P] * 12 + [c_size_t] + [_P] * 14 + [c_float, c_float, _P, c_size_t] + [c_int] * 5
                                 + [c_uint, _P]),
    "stgcn_vit_block_train_drop_supported": (c_int, [c_int] * 4),
    "stgcn_vit_block_train_drop_ws_bytes": (c_size_t, [c_int] * 5),
    "stgcn_vit_block_forward_train_drop": (c_int, [_P, ctypes.POINTER(VitBlockWeights), _P, _P, ctypes.POINTER(VitDropMasks),
                                                   c_float, c_float, _P, c_size_t, _P] + [c_int] * 5 + [c_uint, _P]),
    "stgcn_vit_block_backward_drop": (c_int, [_P, ctypes.POINTER(VitBlockWeights), _P, _P, ctypes.POINTER(VitDropMasks), _P, c_size_t,
                                              _P, _P, ctypes.POINTER(VitBlockGrads), c_float, c_float, _P, c_size_t] + [c_int] * 5
                                      + [c_uint, _P]),
    "stgcn_vit_patch_embed_backward_supported": (c_int, [c_int] * 7 + [c_uint]),
    "stgcn_vit_patch_embed_backward_ws_bytes": (c_size_t, [c_int] * 7 + [c_uint]),
    "stgcn_vit_patch_embed_backward_cut": (c_int, [c_int] * 7 + [c_uint]),
    "stgcn_vit_patch_embed_backward": (c_int, [_P] * 8 + [c_int] * 7 + [_P, c_size_t, c_uint, _P]),
    "stgcn_vit_pool_classify_backward_supported": (c_int, [c_int] * 4 + [c_uint]),
    "stgcn_vit_pool_classify_backward_ws_bytes": (c_size_t, [c_int] * 4 + [c_uint]),
    "stgcn_vit_pool_classify_backward": (c_int, [_P] * 3 + [c_float] + [_P] * 7 + [c_int] * 4 + [_P, c_size_t, c_uint, _P]),
    "stgcn_vit_wgrad_tile": (c_int, [c_int] * 3 + [c_uint]),
    "stgcn_vit_wgrad_splits": (c_int, [c_int] * 3 + [c_uint]),
    "stgcn_vit_wgrad_writes_direct": (c_int, [c_int] * 3 + [c_uint]),
    "stgcn_vit_block_train_small_ws_bytes": (c_size_t, [c_int] * 5 + [c_uint]),
    "stgcn_vit_linear_backward_small_ws_bytes": (c_size_t, [c_int] * 3 + [c_uint]),
}

_lib = None
_lock = threading.Lock()


class StgcnError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} -> {STATUS.get(code, code)}: {msg}")
        self.code = code


def lib() -> ctypes.CDLL:
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python st-gcn-altformer_amd/stgcn_amd/build.py` "
                "(needs hipcc; there is no fallback path)")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)  # AttributeError = ABI mismatch, on purpose
            fn.restype = res
            fn.argtypes = args
        ver = handle.stgcn_version()
        if ver != ABI_VERSION:
            raise RuntimeError(f"libstgcn_hip.so ABI {ver} != binding ABI {ABI_VERSION}; rebuild")
        _lib = handle
    return _lib


def call(name: str, *args):
    """Invoke a status-returning entry point and raise StgcnError on failure."""
    handle = lib()
    rc = getattr(handle, name)(*args)
    if rc != 0:
        msg = handle.stgcn_last_error()
        raise StgcnError(name, rc, msg.decode("utf-8", "replace") if msg else "")
    return rc
