"""The AltFormer transformer heads (``ST``: spatial blocks then temporal blocks, ``TS``: the other way round) and the whole
``ST_GCN_AltFormer`` model, with the blocks' inference forward on libstgcn_hip.so.

``Mlp``, ``Attention``, ``Block``, ``ST``, ``TS`` mirror model/AltFormer/model_ST.py and model_TS.py of the reference: the same
constructor arguments, attribute names, ``state_dict`` keys, shapes and order, and the same RNG draws in the same order
(``torch.manual_seed(s)`` followed by construction gives the reference's initial parameters; checkpoints load strictly).
``timm`` and ``einops`` are not needed: stochastic depth is the local ``DropPath``, the rearranges are permutes.

Two paths, one result:

* HIP (``stgcn_vit_block_forward``): CUDA float32 input of a covered shape (sequences of up to 4096 tokens: the attention
  kernel keeps K and V on chip up to 256 and streams them in key tiles under a running soft-max above) while autograd records
  nothing that concerns the block (``torch.no_grad()``, or no input and no parameter requires a gradient), no dropout /
  stochastic depth is active, and the call has at least ``HIP_MIN_TOKENS`` tokens (smaller calls are latency-bound; ``set_hip_min_tokens(model, 0)`` lifts it).
  The head's first patch embedding then runs through ``functional.patch_embed`` on the stem output (contiguous or
  channels-last, consumed in place); on this per-block path pooling, the second embedding and ``mlp_head`` are torch ops.
* HIP, the whole head (``set_whole_head(model)``, opt-in; ``stgcn_altformer_head_forward``): one library call from the stem
  output to the logits - both embeddings, every block under its stage's plan, the pooling between the stages
  (``stgcn_vit_pool``) and the pooled LayerNorm + classifier (``stgcn_vit_pool_classify``) - on one workspace from torch's
  allocator, so it captures under ``torch.cuda.graph``.  It runs under the inference conditions above for the whole head
  (``_Head.runs_whole(z)`` tells) and does NOT consult the per-block token thresholds: the caller asked for the whole head.
  Each stage runs under the flag word of its first block; a stage whose blocks disagree takes the per-block path.
  Measured against the per-block path (DESIGN section 14 "the whole head"): 1.7 - 2.5 % faster at one clip under a captured
  graph, level eager, and not faster (the ``TS`` head 6 - 10 % slower) at 32 clips, where the per-block default stays the one to use.
* HIP, training (``stgcn_vit_block_forward_train`` / ``stgcn_vit_block_backward`` behind one ``autograd.Function``): the same
  input conditions while autograd IS recording something that concerns the block (``.train()``, or ``.eval()`` with gradients),
  sequences of up to 256 tokens (longer ones train on torch ops unless ``set_long_training(model)`` opts in: then up to
  4096, on the streaming attention forward and the two streaming backward kernels), no ``nn.Dropout`` active, at least ``HIP_TRAIN_MIN_TOKENS``
  tokens (``set_hip_train_min_tokens``; ``set_hip_min_tokens`` sets both thresholds), env ``STGCN_VIT_TRAIN`` not ``0``.  Stochastic depth is covered: ``Block.draw_drop_path`` draws the two masks
  with the torch path's calls in its order (same seed, same masks) and the kernels apply them per sequence.  The parameters
  are taken by attribute, so an ``nn.DataParallel`` replica's gradients reach its master.  ``Block.trains_on_hip(x)`` tells.
  Default arithmetic ``'f32'`` (``DEFAULT_TRAIN_MATH``, env ``STGCN_VIT_TRAIN_MATH``; ``set_head_math`` overrides both paths).
* HIP, low latency (``set_low_latency(model, min_tokens=0)``): the inference path above for small calls, down to one clip.
  Each ``Block`` gets ``small_tiles`` (its four linears run the tile form ``VIT_TILE_AUTO`` picks for their size: 64 x 64 or
  32 x 64 tiles where 128 x 128 ones would leave most of the part idle) and the inference threshold ``min_tokens``.  Without
  ``min_tokens`` the threshold is ``LOW_LATENCY_MIN_TOKENS`` (see there for what has been measured).  Every form
  computes an output element with the same instructions in the same order, so the result is bit-identical to the
  128 x 128 form's.  The forward launches on one stream and takes its workspace from torch's allocator, so it captures under
  ``torch.cuda.graph`` as one sequential graph.  Training is not touched by these two keywords (see the next entry).  The
  attention kernel at one clip has one workgroup per head;
  ``set_low_latency(model, min_tokens=0, split_attention=True)`` (opt-in) adds ``VIT_ATTN_SPLIT`` to the inference call: the
  fp32 attention of a call with fewer than 192 (sequence, head) pairs and more than 32 tokens per sequence then runs split
  over key tiles, one workgroup per (pair, 32 queries) - the same result up to the summation order, measured 1.07 - 1.08 x
  on the one-clip ``ST`` model and level on ``TS``.
* HIP, small training calls (``set_low_latency_training(model)``, opt-in): each ``Block`` gets ``small_tiles_train``.  Its
  training call then goes to the ``_drop`` pair of entry points with no masks (``stgcn_vit_block_forward_train_drop`` /
  ``stgcn_vit_block_backward_drop``) under ``VIT_TILE_AUTO | VIT_WGRAD_SMALL``: the forward and dgrad linears pick their tile
  form by call size (bit-identical to the 128 x 128 form), and every weight gradient picks between the 128 x 128 and the
  64 x 64 form of its kernel and cuts the tokens to suit (``functional.vit_wgrad_plan`` tells; a product with one split
  stores ``dW`` itself and skips its two summing launches).  ``y``, ``dx`` and the LayerNorm gradients are the bits of the
  switch-off run, the eight weight and bias gradients differ from it in summation order only.  The training threshold
  becomes ``LOW_LATENCY_TRAIN_MIN_TOKENS`` (see there for the measurement), or ``train_min_tokens``.  Stochastic depth,
  ``nn.DataParallel`` replicas, ``set_train_math``, ``set_train_attention_math`` and ``set_long_training`` compose with it
  as they do with the default path.
* torch ops: everything else - CPU tensors, shapes the kernels do not cover, active dropout, calls under the thresholds,
  ``force_torch``.  This is the reference's arithmetic op for op, so its training scripts keep working unchanged.

Arithmetic of the block's linears (``set_head_math`` / env ``STGCN_VIT_MATH``): ``'f32'`` (fp32 matrix cores, exact products),
``'bf16x3'`` (three bf16 products per fp32 product, fp32 accumulate) or ``'mixed'`` (bf16x3 with the qkv linear in f32: an
error in q or k is multiplied by the size of the scores before the exponential).  The attention itself is always fp32.
``'bf16'`` (opt-in, inference, sequences of up to 256 tokens) runs the whole block, attention included, on operands rounded to
bf16 with fp32 accumulation, and keeps qkv, the attention output and the fc1 hidden in bf16 between the launches: 1e-2 of
max|y| instead of 1e-4.  Longer sequences and training calls of such a block run in the default arithmetic of their path.

Arithmetic of the training path (``set_train_math`` / env ``STGCN_VIT_TRAIN_MATH``; ``HEAD_TRAIN_MATH``): the three above, or
``'bf16'`` (opt-in): every matrix product of the four linears - forward, dgrad and weight gradient - on operands rounded to
bf16 with fp32 accumulation, except the qkv forward linear, which runs in f32 for the reason ``'mixed'`` exists.  LayerNorm,
attention, GELU, bias gradients and every stored tensor stay fp32; gradients hold 1e-2 of max|.| per tensor instead of 1e-4.
A ``Block.train_math_mode`` that is not None wins over ``math_mode`` and the environment in the training branch only; this
``'bf16'`` is not the inference ``'bf16'`` (which also rounds qkv, the soft-max weights and the stored intermediates).

Arithmetic of the training path's attention (``set_train_attention_math`` / env ``STGCN_VIT_TRAIN_ATTENTION``): ``'f32'`` (the
default: the fp32 kernels in every training arithmetic above) or ``'bf16'`` (opt-in): for sequences of up to 256 tokens the
attention forward and backward on bf16 matrix cores, the scores as three bf16 products of q and k split into a high and a low
part, every other product on operands rounded once, sums and everything stored in fp32.  It adds ``VIT_TRAIN_ATTN_BF16`` to
whatever ``set_train_math`` chose (meant to go with ``'bf16'`` there) and never reaches the inference path; longer sequences
run the fp32 streaming kernels either way.

Nothing is packed or cached: the kernels read ``nn.Linear.weight`` as stored, so an ``nn.DataParallel`` replica (whose
parameters are plain attributes, fresh clones on every call) needs no staging on its master.
"""
from __future__ import annotations

import os
from functools import partial

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import functional as F
from ._capi import (MATH_BF16X3, MATH_F32, VIT_ATTN_SPLIT, VIT_BF16, VIT_QKV_F32, VIT_TILE_AUTO, VIT_TILE_MASK,
                    VIT_TRAIN_ATTN_BF16, VIT_TRAIN_BF16, VIT_WGRAD_SMALL)
from .modules import Unit2D, enable_stem_fusion, import_class, unit_agcn

HEAD_MATH = {"f32": MATH_F32, "bf16x3": MATH_BF16X3, "mixed": MATH_BF16X3 | VIT_QKV_F32, "bf16": VIT_BF16}
DEFAULT_HEAD_MATH = "mixed"
# the training path's modes: the three shared with inference, and 'bf16' = bf16 operands in every linear product but the qkv
# forward.  Not HEAD_MATH['bf16'], which is an inference mode that a training entry point refuses.
# The qkv forward of 'bf16' runs in f32 (VIT_QKV_F32), not in the bf16x3 the low bits name: the entry points accept both, and
# both hold 1e-2 of max|.| (measured 4.2e-3 at worst either way), but the 2^-17 of a bf16x3 product, multiplied by the size
# of the scores, moves enough gradients of the attention across a bf16 rounding boundary of the next product that the result
# sits 0.40-0.49 of the rounding error away from the mode's fp64 emulation, in the L2 norm, against 0.12-0.28 with exact
# products (DESIGN section 15 "bf16": the emulation with a bf16x3 qkv forward reproduces the 0.49 on the CPU).
HEAD_TRAIN_MATH = {"f32": MATH_F32, "bf16x3": MATH_BF16X3, "mixed": MATH_BF16X3 | VIT_QKV_F32,
                   "bf16": VIT_TRAIN_BF16 | MATH_BF16X3 | VIT_QKV_F32}


def _default_head_math() -> int:
    return HEAD_MATH[os.environ.get("STGCN_VIT_MATH", DEFAULT_HEAD_MATH).lower()]


DEFAULT_TRAIN_MATH = "f32"   # the fastest arithmetic whose gradients hold both criteria of the fp32 contract on every tensor,
#                              in the six block cases and through the twelve blocks of a whole model:
#                              'mixed' is 9-12 % faster and holds both on a single block, but only the max-norm criterion on some
#                              tensors of the whole model (1.1e-5 of max|.|); 'bf16x3' holds the max-norm criterion only


def _default_train_math() -> int:
    return HEAD_TRAIN_MATH[os.environ.get("STGCN_VIT_TRAIN_MATH", DEFAULT_TRAIN_MATH).lower()]


HIP_TRAIN_MIN_TOKENS = 13200   # forward + backward of a block (tools/time_altformer_train.py at batch 2, 4, 8, 32): every measured
#                                stage from 13,200 tokens up is faster on HIP by more than the spread (1.29-1.78 x); below, some
#                                thirty launches per block are latency-bound and the picture is mixed (5,760 tokens at D = 512:
#                                0.83 x; 6,600 at D = 256: 1.26 x), so such calls stay on torch ops
HIP_MIN_TOKENS = 4096   # below this many tokens (B * L) per call a block's five launches are latency-bound and the library's
#                         small GEMMs are as fast or faster (measured at batch 32: the TS head's spatial stage, 1472 and 704
#                         tokens, 0.32 against 0.27 ms per block): the block then takes its torch path


LOW_LATENCY_MIN_TOKENS = HIP_MIN_TOKENS   # the token count from which the auto-tile HIP block beats the torch path: NOT MEASURED yet
#                                          (tools/time_altformer.py --tiles sweep --batch 1 is the run), so it stays where the
#                                          128 x 128 measurement put it; set_low_latency(model, min_tokens=0) runs one clip on HIP


LOW_LATENCY_TRAIN_MIN_TOKENS = 6600   # forward + backward of a block with small_tiles_train (tools/time_altformer_train.py --small at
#                                       batch 2, 8, 16, 32; profiles/altformer_train_small_times.json): the smallest measured stage
#                                       from which every measured stage beats the torch path by more than the spread (1.33-1.73 x).
#                                       Below it the picture is mixed by the width, not the size: every stage of up to 2,880
#                                       tokens is faster (1.14-2.19 x, 44 to 2,880 tokens), the ST temporal stage at batch 32
#                                       (4,800 and 5,760 tokens at D = 512) is not (0.93-1.05 x), so a threshold cannot admit
#                                       the former without the latter; train_min_tokens=0 does, for batches of 16 and fewer


def set_low_latency(module: nn.Module, enabled: bool = True, min_tokens=None, split_attention: bool = False) -> None:
    """Small inference calls (down to one clip) of every ``Block`` below on the HIP kernels: ``small_tiles`` (the linears'
    tile form picked per call size, same result bit for bit) and the inference threshold ``min_tokens``
    (``LOW_LATENCY_MIN_TOKENS`` when None).  ``split_attention`` (opt-in) sets ``Block.split_attention``: the fp32 attention
    of a call with few (sequence, head) pairs runs split over key tiles (``VIT_ATTN_SPLIT``; the same result up to the
    summation order).  ``enabled=False`` restores ``small_tiles = False``, ``split_attention = False`` and ``HIP_MIN_TOKENS``
    (for the ST-ViT head's modules: their own defaults, ``HipSwitches.DEFAULT_*``).  The training threshold is not touched;
    the training twin of this switch is ``set_low_latency_training``, and ``enabled=False`` here takes that one back too
    (``set_low_latency_training(module, False)``: nothing moves where it was never set)."""
    if not enabled:
        set_low_latency_training(module, False)
    for sub in module.modules():
        if isinstance(sub, HipSwitches):
            sub.small_tiles = bool(enabled) or sub.DEFAULT_SMALL_TILES
            sub.split_attention = bool(enabled) and bool(split_attention)
            if not enabled:
                sub.hip_min_tokens = sub.DEFAULT_HIP_MIN_TOKENS
            else:
                sub.hip_min_tokens = min(LOW_LATENCY_MIN_TOKENS, sub.DEFAULT_HIP_MIN_TOKENS) if min_tokens is None else int(min_tokens)


def set_low_latency_training(module: nn.Module, enabled: bool = True, train_min_tokens=None) -> None:
    """Small TRAINING calls of every ``Block`` (and ST-ViT ``Layer``) below on the HIP kernels, opt-in: ``small_tiles_train``
    (the training word gets ``VIT_TILE_AUTO | VIT_WGRAD_SMALL``: the linears' tile form and every weight gradient's form and
    token cut picked per call size, the module docstring) and the training threshold ``train_min_tokens``
    (``LOW_LATENCY_TRAIN_MIN_TOKENS`` when None, never above the module's own default; 0: every call).  ``enabled=False``
    restores ``small_tiles_train = False`` and ``DEFAULT_HIP_TRAIN_MIN_TOKENS`` on the modules where the switch was on; a
    threshold set by hand on a module whose switch is off stays.  Inference (``set_low_latency``) is not touched."""
    for sub in module.modules():
        if isinstance(sub, HipSwitches):
            if enabled:
                sub.small_tiles_train = True
                sub.hip_train_min_tokens = (min(LOW_LATENCY_TRAIN_MIN_TOKENS, sub.DEFAULT_HIP_TRAIN_MIN_TOKENS)
                                            if train_min_tokens is None else int(train_min_tokens))
            elif sub.small_tiles_train:
                sub.small_tiles_train = False
                sub.hip_train_min_tokens = sub.DEFAULT_HIP_TRAIN_MIN_TOKENS


def set_whole_head(module: nn.Module, enabled: bool = True) -> None:
    """Every ``ST`` / ``TS`` head below runs from the stem output to the logits in ONE library call
    (``stgcn_altformer_head_forward``: both embeddings, every block, the pooling between the stages and the pooled LayerNorm +
    classifier) wherever ``_Head.runs_whole(z)`` says it can; everywhere else, and with ``enabled=False`` (the default of a
    new head), the forward is the per-block one.  The caller asks for the whole head: the per-block token thresholds
    (``hip_min_tokens``) are NOT consulted, the blocks' arithmetic, tile and split-attention settings are."""
    for sub in module.modules():
        if isinstance(sub, _Head):
            sub.whole_head = bool(enabled)


HIP_TRAIN_MAX_LEN = 256        # longest sequence a Block trains on HIP by default: the resident attention kernels' limit
HIP_TRAIN_LONG_MAX_LEN = 4096  # with set_long_training: the streaming kernels' limit.  Opt-in because the measurement at 500
#                                frames, batch 32 (tools/time_altformer_train.py --frames 500, DESIGN section 15 "long sequences")
#                                is mixed: the TS temporal stage 1.50 x faster than torch ops, the ST temporal stage a tie


def set_long_training(module: nn.Module, enabled: bool = True) -> None:
    """Sequences of 257 to 4096 tokens of every ``Block`` below train on the HIP kernels (the streaming attention forward
    and backward) instead of torch ops: ``hip_train_max_len`` = 4096, or back to 256 with ``enabled=False``.  Shorter
    sequences and both token thresholds are not touched."""
    for sub in module.modules():
        if isinstance(sub, Block):
            sub.hip_train_max_len = HIP_TRAIN_LONG_MAX_LEN if enabled else HIP_TRAIN_MAX_LEN


def set_hip_min_tokens(module: nn.Module, tokens: int) -> None:
    """The token count (B * L) from which every ``Block`` below uses the HIP path where it applies (0: always).  One knob for
    "always HIP": it sets the training threshold (``set_hip_train_min_tokens``) to the same value."""
    for sub in module.modules():
        if isinstance(sub, HipSwitches):
            sub.hip_min_tokens = int(tokens)
            sub.hip_train_min_tokens = int(tokens)


def set_hip_train_min_tokens(module: nn.Module, tokens: int) -> None:
    """The token count (B * L) from which every ``Block`` (and ST-ViT ``Layer``) below trains on the HIP kernels where they
    apply (0: always)."""
    for sub in module.modules():
        if isinstance(sub, HipSwitches):
            sub.hip_train_min_tokens = int(tokens)


def set_head_math(module: nn.Module, mode) -> None:
    """Arithmetic of the linears of every ``Block`` below: 'f32' | 'bf16x3' | 'mixed' | 'bf16' (the whole block on bf16
    operands: inference and L <= 256 only, anything else of such a block runs its path's default), or None for the default."""
    m = None if mode is None else HEAD_MATH[mode] if isinstance(mode, str) else int(mode)
    for sub in module.modules():
        if isinstance(sub, HipSwitches):
            sub.math_mode = m


TRAIN_ATTENTION_MATH = ("f32", "bf16")


def _default_train_attention() -> str:
    mode = os.environ.get("STGCN_VIT_TRAIN_ATTENTION", "f32").lower()
    if mode not in TRAIN_ATTENTION_MATH:
        raise KeyError(mode)
    return mode


def set_train_attention_math(module: nn.Module, mode) -> None:
    """Arithmetic of the attention in the HIP training path of every ``Block`` below: 'f32' (the fp32 kernels) | 'bf16' (forward
    and backward on bf16 matrix operands for sequences of up to 256 tokens, opt-in; see the module docstring), or None for what
    env ``STGCN_VIT_TRAIN_ATTENTION`` gives, else 'f32'.  ``set_train_math`` and inference are not touched."""
    if mode is not None and mode not in TRAIN_ATTENTION_MATH:
        raise KeyError(mode)
    for sub in module.modules():
        if isinstance(sub, HipSwitches):
            sub.train_attention_mode = mode


def set_train_math(module: nn.Module, mode) -> None:
    """Arithmetic of the HIP training path of every ``Block`` below: 'f32' | 'bf16x3' | 'mixed' | 'bf16' (``HEAD_TRAIN_MATH``;
    'bf16': every linear product but the qkv forward on bf16 operands, opt-in, 1e-2 of max|.| per gradient tensor), or None
    for what ``set_head_math`` / ``STGCN_VIT_TRAIN_MATH`` / ``DEFAULT_TRAIN_MATH`` give.  Inference is not touched."""
    m = None if mode is None else HEAD_TRAIN_MATH[mode] if isinstance(mode, str) else int(mode)
    for sub in module.modules():
        if isinstance(sub, HipSwitches):
            sub.train_math_mode = m


class HipSwitches:
    """What a module that runs ``stgcn_vit_block_forward`` carries for ``set_head_math``, ``set_low_latency`` and
    ``set_hip_min_tokens``, and the one place that turns it into the inference flag word: ``Block`` here, and the layers and
    the front of the ST-ViT head (``stgcn_amd.vit``)."""

    DEFAULT_HIP_MIN_TOKENS = HIP_MIN_TOKENS
    DEFAULT_HIP_TRAIN_MIN_TOKENS = HIP_TRAIN_MIN_TOKENS
    DEFAULT_SMALL_TILES = False

    def _init_switches(self):
        self.math_mode = None                  # None: _default_head_math() at call time
        self.train_math_mode = None            # set_train_math: the training branch's arithmetic; None: as math_mode decides
        self.train_attention_mode = None       # set_train_attention_math: 'f32' | 'bf16'; None: env STGCN_VIT_TRAIN_ATTENTION, else 'f32'
        self.force_torch = False               # diagnostics / timing: take the torch-op path even where the HIP path applies
        self.hip_min_tokens = self.DEFAULT_HIP_MIN_TOKENS   # set_hip_min_tokens
        self.hip_train_min_tokens = self.DEFAULT_HIP_TRAIN_MIN_TOKENS   # set_hip_train_min_tokens
        self.hip_train_max_len = HIP_TRAIN_MAX_LEN         # set_long_training
        self.small_tiles = self.DEFAULT_SMALL_TILES   # set_low_latency: the inference linears pick their tile form by call size
        self.split_attention = False           # set_low_latency(split_attention=True): VIT_ATTN_SPLIT on the inference word
        self.small_tiles_train = False         # set_low_latency_training: VIT_TILE_AUTO | VIT_WGRAD_SMALL on the training word

    def _inference_flags(self, L: int, D: int, heads: int, hidden: int) -> int:
        """The flag word of an inference call of a block of this shape: ``math_mode``, else ``_default_head_math()``;
        ``'bf16'`` only where its resident form covers the length (longer sequences run the default arithmetic, still on HIP);
        ``small_tiles`` adds ``VIT_TILE_AUTO`` unless ``math_mode`` forces a form; ``split_attention`` adds ``VIT_ATTN_SPLIT``."""
        math = _default_head_math() if self.math_mode is None else self.math_mode
        if math & VIT_BF16 and not F.vit_block_forward_bf16_supported(L, D, heads, hidden):
            math = HEAD_MATH[DEFAULT_HEAD_MATH] | (math & VIT_TILE_MASK)
        if self.small_tiles and not math & VIT_TILE_MASK:
            math |= VIT_TILE_AUTO
        if self.split_attention:
            math |= VIT_ATTN_SPLIT
        return math


    def _train_flags(self, tiles: bool = False) -> int:
        """The flag word of a training call (``Block._hip_flags`` describes the resolution).  ``tiles``: the caller's entry
        points take a tile field (the ST-ViT ``Layer``'s ``_drop`` pair always; a ``Block``'s older pair refuses one, so a
        ``Block`` asks for this only with ``small_tiles_train``, when it calls the ``_drop`` pair too), so ``small_tiles`` adds
        ``VIT_TILE_AUTO`` to the word and ``small_tiles_train`` adds ``VIT_TILE_AUTO | VIT_WGRAD_SMALL``."""
        attn = self.train_attention_mode if self.train_attention_mode is not None else _default_train_attention()
        bit = VIT_TRAIN_ATTN_BF16 if attn == "bf16" else 0
        if tiles and self.small_tiles:
            bit |= VIT_TILE_AUTO
        if tiles and getattr(self, "small_tiles_train", False):
            bit |= VIT_TILE_AUTO | VIT_WGRAD_SMALL
        if self.train_math_mode is not None:
            return self.train_math_mode & ~(VIT_TILE_MASK | VIT_BF16 | VIT_ATTN_SPLIT) | bit
        if self.math_mode is None or self.math_mode & VIT_BF16:
            return _default_train_math() | bit
        return self.math_mode & ~(VIT_TILE_MASK | VIT_ATTN_SPLIT) | bit


class DropPath(nn.Module):
    """Stochastic depth per sample: in training each sample's branch is kept with probability ``1 - drop_prob`` and the kept
    ones are scaled by ``1 / keep`` (one bernoulli draw of batch-size elements per call); identity in eval or at rate 0."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def draw(self, x):
        """This call's per-sample factors (0 or 1 / keep), shape (B, 1, ..., 1), or None where the module is the identity.
        The only place that consumes random numbers: the torch path multiplies by it, the HIP training path hands it to the
        kernels, so both use the same masks after the same seed."""
        if self.drop_prob == 0.0 or not self.training:
            return None
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        return mask

    def forward(self, x):
        mask = self.draw(x)
        return x if mask is None else x * mask

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3):0.3f}"


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        B, L, D = x.shape
        q, k, v = self.qkv(x).reshape(B, L, 3, self.num_heads, D // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        w = self.attn_drop(((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1))
        return self.proj_drop(self.proj((w @ v).transpose(1, 2).reshape(B, L, D)))


def _drop_active(mod: nn.Module) -> bool:
    """Any dropout or stochastic depth below ``mod`` that would draw random numbers in this call."""
    for sub in mod.modules():
        if sub.training and ((isinstance(sub, nn.Dropout) and sub.p > 0) or (isinstance(sub, DropPath) and sub.drop_prob > 0)):
            return True
    return False


class _BlockTrain(torch.autograd.Function):
    """One Block on the HIP training kernels: ``stgcn_vit_block_forward_train`` / ``stgcn_vit_block_backward``.  The twelve
    parameters arrive as arguments (taken by attribute from the module), so the gradients of an ``nn.DataParallel`` replica's
    clones flow back to its master through autograd like any other op's.  Three more tensors behind the twelve are the
    per-element dropout factors (m_proj, m_act, m_fc2, each may be None) of an ST-ViT ``Layer`` (``stgcn_amd.vit``): the call then
    goes to the ``_drop`` pair of entry points, which also takes a tile field in ``math``."""

    @staticmethod
    def forward(ctx, x, s1, s2, heads, eps, scale, math, *params):
        twelve = len(F.VIT_BLOCK_PARAMS)
        params, drop = params[:twelve], (tuple(params[twelve:]) if len(params) > twelve else None)
        x = x.contiguous()
        y, saved = F.vit_block_forward_train(x, params, heads, eps, scale, math, s1, s2, drop=drop)
        ctx.save_for_backward(x, s1, s2, *params, *(drop or ()))
        ctx.saved_buf, ctx.cfg = saved, (heads, eps, scale, math)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        twelve = len(F.VIT_BLOCK_PARAMS)
        x, s1, s2, *rest = ctx.saved_tensors
        params, drop = rest[:twelve], (tuple(rest[twelve:]) if len(rest) > twelve else None)
        heads, eps, scale, math = ctx.cfg
        dy = dy.contiguous()
        if drop is not None and (drop[0] is not None or drop[2] is not None):
            dy = F.aligned(dy)                  # with m_proj or m_fc2 the cotangent is a listed operand (16 bytes)
        g = F.vit_block_backward(x, params, ctx.saved_buf, dy, heads, eps, scale, math, s1, s2, drop=drop)
        ctx.saved_buf = None
        return (g["x"], None, None, None, None, None, None) + tuple(g[n] for n in F.VIT_BLOCK_PARAMS) + (None,) * len(drop or ())


class Block(nn.Module, HipSwitches):
    """``x + attn(norm1(x))`` then ``x + mlp(norm2(x))`` (each branch through ``drop_path``); x is (B, L, dim)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                              proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self._init_switches()

    def _weights(self):
        """The parameters by attribute (an nn.DataParallel replica has no ``parameters()``)."""
        for lin in (self.norm1, self.attn.qkv, self.attn.proj, self.norm2, self.mlp.fc1, self.mlp.fc2):
            yield lin.weight
            yield lin.bias

    def _kernels_cover(self, x: torch.Tensor, train: bool) -> bool:
        """CUDA float32 (B, L, D) input and a module the kernels implement (LayerNorms with affine, exact GELU, covered sizes).
        The sizes differ: inference reaches 4096 tokens per sequence (the streaming attention kernel above 256), training
        ``hip_train_max_len`` (256 unless ``set_long_training`` raised it)."""
        if self.force_torch or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3:
            return False
        if not (type(self.norm1) is nn.LayerNorm and type(self.norm2) is nn.LayerNorm and isinstance(self.mlp.act, nn.GELU)
                and getattr(self.mlp.act, "approximate", "none") == "none" and self.norm1.elementwise_affine
                and self.norm2.elementwise_affine and self.norm1.eps == self.norm2.eps
                and self.norm1.bias is not None and self.norm2.bias is not None):
            return False
        B, L, D = x.shape
        if B < 1 or D != self.norm1.normalized_shape[0] or self.mlp.fc2.out_features != D:
            return False
        if train:
            return L <= self.hip_train_max_len and F.vit_block_train_long_supported(L, D, self.attn.num_heads,
                                                                                    self.mlp.fc1.out_features)
        return F.vit_block_forward_supported(L, D, self.attn.num_heads, self.mlp.fc1.out_features)

    def _records_grad(self, x: torch.Tensor) -> bool:
        return torch.is_grad_enabled() and (x.requires_grad or any(t is not None and t.requires_grad for t in self._weights()))

    def hip_applies(self, x: torch.Tensor) -> bool:
        """Whether this call can run on the inference kernels (see the module docstring)."""
        if x.dim() != 3 or self._records_grad(x) or _drop_active(self):
            return False
        return self._kernels_cover(x, train=False)

    def trains_on_hip(self, x: torch.Tensor) -> bool:
        """Whether this call runs on the HIP training kernels (forward that saves for the backward, backward on
        ``loss.backward()``): autograd is recording something that concerns the block, no ``nn.Dropout`` is active
        (stochastic depth may be), the shape is covered and the call has at least ``hip_train_min_tokens`` tokens."""
        if x.dim() != 3 or os.environ.get("STGCN_VIT_TRAIN", "1") == "0" or not self._records_grad(x):
            return False
        if x.shape[0] * x.shape[1] < self.hip_train_min_tokens:
            return False
        if any(sub.training and sub.p > 0 for sub in self.modules() if isinstance(sub, nn.Dropout)):
            return False
        if not isinstance(self.drop_path, (DropPath, nn.Identity)):
            return False
        return self._kernels_cover(x, train=True)

    def draw_drop_path(self, x: torch.Tensor):
        """The stochastic-depth factors of this call, attention branch first, then the MLP branch - the order, shapes and
        generator calls of the torch path - as two (B, 1, 1) tensors, or None where nothing is drawn."""
        if not isinstance(self.drop_path, DropPath):
            return None, None
        return self.drop_path.draw(x), self.drop_path.draw(x)

    def uses_hip(self, x: torch.Tensor) -> bool:
        """``hip_applies`` and the call is large enough for the HIP path to be the faster one (``hip_min_tokens``)."""
        return x.dim() == 3 and x.shape[0] * x.shape[1] >= self.hip_min_tokens and self.hip_applies(x)

    def _hip_flags(self, x: torch.Tensor, train: bool) -> int:
        """The flag word this call hands to its HIP path, resolved here and nowhere else.  Training: ``train_math_mode``
        (``set_train_math`` wins), else ``math_mode``, else ``_default_train_math()``; tile forms and ``HEAD_MATH['bf16']`` are
        inference modes that never reach a training entry point (a block set to the latter trains in its path's default);
        ``train_attention_mode`` (``set_train_attention_math``), else env ``STGCN_VIT_TRAIN_ATTENTION``, adds
        ``VIT_TRAIN_ATTN_BF16`` on top of any of them when it says ``'bf16'``, and nothing otherwise.
        ``small_tiles_train`` (``set_low_latency_training``) adds ``VIT_TILE_AUTO | VIT_WGRAD_SMALL``: the call then goes
        to the ``_drop`` pair, which takes both; without it the word carries neither, whatever ``small_tiles`` says.
        Inference: ``HipSwitches._inference_flags`` (the training word never carries ``VIT_ATTN_SPLIT``)."""
        if train:
            return self._train_flags(tiles=self.small_tiles_train)
        return self._inference_flags(x.shape[1], x.shape[2], self.attn.num_heads, self.mlp.fc1.out_features)

    def forward(self, x):
        if self.uses_hip(x):
            a, m = self.attn, self.mlp
            with torch.no_grad():
                return F.vit_block_forward(x.contiguous(), (self.norm1.weight, self.norm1.bias), (a.qkv.weight, a.qkv.bias),
                                           (a.proj.weight, a.proj.bias), (self.norm2.weight, self.norm2.bias),
                                           (m.fc1.weight, m.fc1.bias), (m.fc2.weight, m.fc2.bias), a.num_heads, self.norm1.eps,
                                           a.scale, self._hip_flags(x, train=False))
        if self.trains_on_hip(x):
            s1, s2 = self.draw_drop_path(x)
            # small_tiles_train: three absent dropout masks behind the twelve parameters send the call to the _drop pair
            return _BlockTrain.apply(x, None if s1 is None else s1.reshape(-1), None if s2 is None else s2.reshape(-1),
                                     self.attn.num_heads, self.norm1.eps, self.attn.scale, self._hip_flags(x, train=True),
                                     *self._weights(), *((None, None, None) if self.small_tiles_train else ()))
        x = x + self.drop_path(self.attn(self.norm1(x)))
        return x + self.drop_path(self.mlp(self.norm2(x)))


def max_over_tokens(x):
    """``x.max(dim=1).values``, the heads' pooling over the frames.  Its gradient goes to the token that holds the maximum, so
    a tie at the last bit sends it elsewhere; the one place where a comparison of two arithmetic paths can pin the picks."""
    return x.max(dim=1).values


def _embed_on_hip(x, lin) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and not (torch.is_grad_enabled() and (x.requires_grad or lin.weight.requires_grad or lin.bias.requires_grad)))


class _Head(nn.Module):
    """What ST and TS share: the construction after the two embeddings (so that the RNG draws keep the reference's order) and
    the two stages of the forward."""

    def _build_common(self, class_num, num_frame, embed_dim, spatial_dim, temporal_dim, depth, num_heads, mlp_ratio, qkv_bias,
                      qk_scale, drop_rate, attn_drop_rate, drop_path_rate, norm_layer):
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, depth)]

        def stack(dim):
            return nn.ModuleList([Block(dim=dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                        drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer)
                                  for i in range(depth)])
        self.Spatial_blocks = stack(spatial_dim)
        self.blocks = stack(temporal_dim)
        self.Spatial_norm = norm_layer(spatial_dim)       # in the state_dict, not in the forward (as in the reference)
        self.Temporal_norm = norm_layer(temporal_dim)
        self.pool = 'cls'
        self.to_latent = nn.Identity()
        self.weighted_mean = nn.Conv1d(in_channels=num_frame, out_channels=1, kernel_size=1)
        self.mlp_head = nn.Sequential(nn.LayerNorm(embed_dim), nn.Linear(embed_dim, class_num))
        self.fcn = nn.Conv1d(512, class_num, kernel_size=1)

    whole_head = False   # set_whole_head: the one-call forward where runs_whole(z) allows it

    def _stages(self):
        """(order, first embedding, its position table, its blocks, second embedding, its position table, its blocks)."""
        raise NotImplementedError

    def _whole_plan(self, z):
        """The arguments of ``functional.altformer_head_forward`` for this call, taken by attribute (an nn.DataParallel
        replica has no ``parameters()``), or None where the head takes the per-block forward."""
        if not self.whole_head or not torch.is_tensor(z) or not z.is_cuda or z.dtype != torch.float32 or z.dim() != 4:
            return None
        if not (z.is_contiguous() or F._is_channels_last(z)):
            return None
        order, lin1, pos1, blocks1, lin2, pos2, blocks2 = self._stages()
        head = self.mlp_head
        if not (isinstance(head, nn.Sequential) and len(head) == 2 and type(head[0]) is nn.LayerNorm and type(head[1]) is nn.Linear
                and head[0].elementwise_affine and head[0].bias is not None and type(lin1) is nn.Linear and type(lin2) is nn.Linear
                and lin1.bias is not None and lin2.bias is not None and len(blocks1) and len(blocks2)
                and all(type(b) is Block for b in list(blocks1) + list(blocks2))):
            return None
        glue = (lin1.weight, lin1.bias, pos1, lin2.weight, lin2.bias, pos2, head[0].weight, head[0].bias, head[1].weight, head[1].bias)
        if torch.is_grad_enabled() and (z.requires_grad or any(t is not None and t.requires_grad for t in glue)):
            return None
        if _drop_active(self):
            return None
        N, C, T, V = z.shape
        E1, E2 = lin1.out_features, lin2.out_features
        L1, L2 = (T, V) if order == "TS" else (V, T)
        if lin1.in_features != C or lin2.in_features != E1 or head[0].normalized_shape != (E2,) or head[1].in_features != E2:
            return None
        if pos1.numel() != L1 * E1 or pos2.numel() != L2 * E2:
            return None
        first = blocks1[0]
        words = []
        for blocks, B, L, D in ((blocks1, N * L2, L1, E1), (blocks2, N, L2, E2)):
            probe = z.as_strided((B, L, D), (0, 0, 0))      # the stage's shape without its memory
            b0 = blocks[0]
            word = b0._hip_flags(probe, train=False)
            for b in blocks:
                if not b.hip_applies(probe) or b._hip_flags(probe, train=False) != word:
                    return None
                if (b.attn.num_heads != first.attn.num_heads or b.norm1.eps != first.norm1.eps or b.attn.scale != b0.attn.scale
                        or b.mlp.fc1.out_features != b0.mlp.fc1.out_features):
                    return None
            words.append(word)
        if not F.altformer_head_supported(N, T, V, C, E1, E2, first.attn.num_heads, blocks1[0].mlp.fc1.out_features,
                                          blocks2[0].mlp.fc1.out_features, len(blocks1), len(blocks2), head[1].out_features,
                                          order, words[0], words[1]):
            return None
        return dict(embed1=(lin1.weight, lin1.bias), pos1=pos1, blocks1=[tuple(b._weights()) for b in blocks1],
                    embed2=(lin2.weight, lin2.bias), pos2=pos2, blocks2=[tuple(b._weights()) for b in blocks2],
                    head_norm=(head[0].weight, head[0].bias), head_linear=(head[1].weight, head[1].bias),
                    heads=first.attn.num_heads, eps_blocks=first.norm1.eps, eps_head=head[0].eps, scale1=blocks1[0].attn.scale,
                    scale2=blocks2[0].attn.scale, order=order, math1=words[0], math2=words[1])

    def runs_whole(self, z) -> bool:
        """Whether ``forward(z)`` is the one library call: ``whole_head`` is on (``set_whole_head``), z is CUDA float32
        (contiguous or channels-last), autograd records nothing that concerns the head, no dropout or stochastic depth is
        active, every ``Block`` answers ``hip_applies`` for its stage's shape, the blocks of a stage agree on their flag word
        (``Block._hip_flags`` of the stage's first block is the stage's) and ``stgcn_altformer_head_supported`` agrees."""
        return self._whole_plan(z) is not None

    def _forward_whole(self, z):
        """The logits from the one call, or None where this call takes the per-block forward."""
        plan = self._whole_plan(z)
        if plan is None:
            return None
        w, b = plan["head_linear"]
        plan["head_linear"] = (F.aligned(w), b)     # the call's one listed operand (16 bytes): a copy where a flat buffer holds it
        with torch.no_grad():
            return F.altformer_head_forward(z, **plan)

    def _first_stage(self, x, lin, pos, blocks, order):
        """Stem output (N, C, T, V) -> rows (N*T, V, E) ('ST') or (N*V, T, E) ('TS') through the first embedding and blocks."""
        if _embed_on_hip(x, lin):
            with torch.no_grad():
                x = F.patch_embed(x, lin.weight, lin.bias, pos, order=order)
        else:
            N, C, T, V = x.shape
            rows = x.permute(0, 2, 3, 1).reshape(N * T, V, C) if order == "ST" else x.permute(0, 3, 2, 1).reshape(N * V, T, C)
            x = lin(rows)
            x += pos
        x = self.pos_drop(x)
        for blk in blocks:
            x = blk(x)
        return x

    def _second_stage(self, x, lin, pos, blocks):
        x = lin(x)
        x += pos
        x = self.pos_drop(x)
        for blk in blocks:
            x = blk(x)
        return x


class ST(_Head):
    """Spatial blocks over the joints of every frame (dim ``embed_dim_ratio``), mean over joints, temporal blocks over the
    frames (dim 2 * ``embed_dim_ratio``), max over frames, ``mlp_head``.  Input: the stem output (N, in_chans, T, V)."""

    def __init__(self, class_num, num_frame=180, num_joints=22, in_chans=128, embed_dim_ratio=256, depth=4, num_heads=8,
                 mlp_ratio=2., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2,
                 norm_layer=None):
        super().__init__()
        self.class_num = class_num
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        embed_dim = embed_dim_ratio * 2
        self.Spatial_patch_to_embedding = nn.Linear(in_chans, embed_dim_ratio)
        self.Spatial_pos_embed = nn.Parameter(torch.zeros(1, num_joints, embed_dim_ratio))
        self.Spatial_cls_token = nn.Parameter(torch.randn(1, 1, embed_dim_ratio))
        self.Temporal_patch_to_embedding = nn.Linear(embed_dim_ratio, embed_dim)
        self.Temporal_pos_embed = nn.Parameter(torch.zeros(1, num_frame, embed_dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, embed_dim))
        self._build_common(class_num, num_frame, embed_dim, embed_dim_ratio, embed_dim, depth, num_heads, mlp_ratio, qkv_bias,
                           qk_scale, drop_rate, attn_drop_rate, drop_path_rate, norm_layer)

    def Spatial_forward_features(self, x):
        N, _, T, _ = x.shape
        x = self._first_stage(x, self.Spatial_patch_to_embedding, self.Spatial_pos_embed, self.Spatial_blocks, "ST")
        return x.mean(dim=1).reshape(N, T, -1)

    def forward_features(self, x):
        x = self._second_stage(x, self.Temporal_patch_to_embedding, self.Temporal_pos_embed, self.blocks)
        feature = max_over_tokens(x)
        return self.mlp_head(feature), feature.unsqueeze(-1)

    def _stages(self):
        return ("ST", self.Spatial_patch_to_embedding, self.Spatial_pos_embed, self.Spatial_blocks,
                self.Temporal_patch_to_embedding, self.Temporal_pos_embed, self.blocks)

    def forward(self, x):
        whole = self._forward_whole(x)
        if whole is not None:
            return whole
        return self.forward_features(self.Spatial_forward_features(x))[0]


class TS(_Head):
    """Temporal blocks over the frames of every joint (dim ``embed_dim_ratio``), max over frames, spatial blocks over the joints
    (dim 2 * ``embed_dim_ratio``), mean over joints, ``mlp_head``.  Input: the stem output (N, in_chans, T, V)."""

    def __init__(self, class_num, num_frame=180, num_joints=22, in_chans=128, embed_dim_ratio=256, depth=4, num_heads=8,
                 mlp_ratio=2., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2,
                 norm_layer=None):
        super().__init__()
        self.class_num = class_num
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        embed_dim = embed_dim_ratio * 2
        self.temporal_patch_to_embedding = nn.Linear(in_chans, embed_dim_ratio)
        self.Temporal_pos_embed = nn.Parameter(torch.zeros(1, num_frame, embed_dim_ratio))
        self.cls_token = nn.Parameter(torch.randn(1, 1, embed_dim_ratio))
        self.Spatial_patch_to_embedding = nn.Linear(embed_dim_ratio, embed_dim)
        self.Spatial_pos_embed = nn.Parameter(torch.zeros(1, num_joints, embed_dim))
        self.Spatial_cls_token = nn.Parameter(torch.randn(1, 1, embed_dim))
        self._build_common(class_num, num_frame, embed_dim, embed_dim, embed_dim_ratio, depth, num_heads, mlp_ratio, qkv_bias,
                           qk_scale, drop_rate, attn_drop_rate, drop_path_rate, norm_layer)

    def Temporal_forward_features(self, x):
        N, _, _, V = x.shape
        x = self._first_stage(x, self.temporal_patch_to_embedding, self.Temporal_pos_embed, self.blocks, "TS")
        return max_over_tokens(x).reshape(N, V, -1)

    def Spatial_forward_features(self, x):
        x = self._second_stage(x, self.Spatial_patch_to_embedding, self.Spatial_pos_embed, self.Spatial_blocks)
        return self.mlp_head(x.mean(dim=1))

    def _stages(self):
        return ("TS", self.temporal_patch_to_embedding, self.Temporal_pos_embed, self.blocks,
                self.Spatial_patch_to_embedding, self.Spatial_pos_embed, self.Spatial_blocks)

    def forward(self, x):
        whole = self._forward_whole(x)
        if whole is not None:
            return whole
        return self.Spatial_forward_features(self.Temporal_forward_features(x))


class ST_GCN_AltFormer(nn.Module):
    """The whole model of model/AltFormer/ST_GCN_AltFormer.py: ``gcn0`` -> ``tcn0`` (the fused HIP stem) -> ``modelA`` (ST) and /
    or ``modelB`` (TS), chosen by ``style`` ('ST', 'TS', anything else: the sum of both).  Input (N, T, V, channel) as the data
    loader delivers it; the stem reads the permuted view in place."""

    def __init__(self, channel, num_class, backbone_in_c=128, num_frame=180, num_joints=22, style=None, graph=None,
                 graph_args=dict(), mask_learning=False, use_local_bn=False):
        super().__init__()
        if graph is None:
            raise ValueError()
        self.graph = import_class(graph)(**graph_args)
        self.A = torch.from_numpy(self.graph.A.astype(np.float32))
        self.num_frame = num_frame
        self.num_joints = num_joints
        self.num_class = num_class
        self.backbone_in_c = backbone_in_c
        self.style = style
        self.gcn0 = unit_agcn(channel, backbone_in_c, self.A, mask_learning=mask_learning, use_local_bn=use_local_bn)
        self.tcn0 = Unit2D(backbone_in_c, backbone_in_c, kernel_size=9)
        head = dict(num_frame=num_frame, num_joints=num_joints, in_chans=128, embed_dim_ratio=256, depth=6, num_heads=8,
                    mlp_ratio=2., qkv_bias=True, qk_scale=None, drop_path_rate=0.1)
        self.modelA = ST(num_class, **head)
        self.modelB = TS(num_class, **head)
        enable_stem_fusion(self.gcn0, self.tcn0)

    def forward(self, x):
        x = self.tcn0(self.gcn0(x.permute(0, 3, 1, 2)))
        if self.style == 'ST':
            return self.modelA(x)
        if self.style == 'TS':
            return self.modelB(x)
        x_st = self.modelA(x)
        return self.modelB(x) + x_st
