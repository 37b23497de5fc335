"""stgcn_amd — MI355X (gfx950) native ST-GCN stem: HIP kernels behind the reference's nn.Module API.

    from stgcn_amd import unit_agcn, Unit2D, enable_stem_fusion

or, as a drop-in for the reference's own import lines, put ``st-gcn-altformer_amd/`` on ``sys.path``
and keep ``from model.unit_agcn import unit_agcn`` / ``from model.net import Unit2D, import_class``.
"""
from ._capi import (ABI_VERSION, LIB_PATH, MATH_BF16, MATH_BF16X3, MATH_F16MX, MATH_F32, MATH_F32_VALU, OUT_BF16,
                    VIT_WGRAD_SMALL, StgcnError, lib)
from .graphs import HandGraph, LMDHGGraph, SHREGraph
from .modules import (FusedStemOutput, Unit2D, conv_init, disable_stem_fusion, enable_stem_fusion, import_class,
                      set_math_mode, set_output_layout, unit_agcn)
from .st_attention import gcn_unit_attention, set_st_attention_math, spatial_attention
from .altformer import LOW_LATENCY_TRAIN_MIN_TOKENS, ST, TS, Block, ST_GCN_AltFormer, set_head_math, set_hip_min_tokens, set_hip_train_min_tokens, set_long_training, set_low_latency, set_low_latency_training, set_train_attention_math, set_train_math, set_whole_head
from .vit import ViT

__all__ = ["ST_GCN_AltFormer", "ST", "TS", "Block", "ViT", "set_head_math", "set_hip_min_tokens", "set_hip_train_min_tokens", "set_low_latency", "set_low_latency_training", "set_long_training", "set_train_math", "set_train_attention_math", "set_whole_head", "set_st_attention_math", "unit_agcn", "Unit2D", "gcn_unit_attention", "spatial_attention", "FusedStemOutput", "conv_init", "import_class", "enable_stem_fusion", "disable_stem_fusion",
           "set_math_mode", "set_output_layout", "SHREGraph", "LMDHGGraph", "HandGraph", "lib", "StgcnError", "LIB_PATH",
           "ABI_VERSION", "MATH_F32", "MATH_BF16X3", "MATH_BF16", "MATH_F32_VALU", "MATH_F16MX", "OUT_BF16",
           "VIT_WGRAD_SMALL", "LOW_LATENCY_TRAIN_MIN_TOKENS"]
