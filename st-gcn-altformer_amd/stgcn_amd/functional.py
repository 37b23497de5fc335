"""Tensor-level wrappers over the C ABI: torch supplies device memory and the stream, nothing else.

Every function takes CUDA(HIP) tensors, validates dtype/contiguity/device, passes raw device
pointers plus ``torch.cuda.current_stream()`` to libstgcn_hip.so and returns freshly allocated
outputs.  Nothing here computes on the host and nothing falls back to torch ops.

Alignment (include/stgcn_hip.h, "Alignment"; DESIGN.md section 4 has the table).  A tensor operand - input, parameter,
cotangent, result, a caller's ``out`` - needs the alignment of its element only (4 bytes fp32, 2 bytes bf16): a contiguous
view at any element offset (``x[1:]``, a parameter that lives in a flat buffer) is served in place.  The exceptions are the
operands an entry point lists by name, which need ``ALIGN_LISTED`` = 16 bytes, and blobs and workspaces (``prep``, ``Wp``,
``ws``, the saved buffers), which need ``ALIGN_BLOB`` = 256 as the allocator gives them.  A wrapper here raises ``ValueError``
naming the operand that misses its demand, before anything is launched; ``aligned(t)`` returns ``t`` itself or, where its
address misses the demand, a copy that meets it - the modules and autograd functions hand every listed operand through it, so
they never surface such a refusal.
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_longlong, c_size_t, c_uint, c_void_p
from typing import Optional, Tuple

import torch

from . import _capi
from ._capi import MATH_BF16, MATH_BF16X3, MATH_F16MX, MATH_F32, MATH_F32_VALU, OUT_BF16, VIT_ATTN_SPLIT, VIT_BF16, VIT_TRAIN_ATTN_BF16, VIT_TRAIN_BF16, VIT_WGRAD_SMALL  # noqa: F401 (re-export)

BN_EPS = 1e-5
ALIGN_LISTED = 16     # the operands an entry point lists by name
ALIGN_BLOB = 256      # prep, Wp, ws and the saved buffers


def aligned(t: Optional[torch.Tensor], nbytes: int = ALIGN_LISTED) -> Optional[torch.Tensor]:
    """``t`` itself where its first byte sits on a multiple of ``nbytes`` (or ``t`` is None), else a copy from the allocator
    with the same values and dense strides (contiguous stays contiguous, channels-last stays channels-last).  For the
    operands an entry point lists as exceptions to element alignment; a caller that saves the operand saves what this
    returns."""
    if t is None or t.data_ptr() % nbytes == 0:
        return t
    return t.detach().clone(memory_format=torch.preserve_format)


def _require_aligned(t: Optional[torch.Tensor], name: str, nbytes: int) -> None:
    if t is not None and t.data_ptr() % nbytes:
        raise ValueError(f"{name} must be {nbytes}-byte aligned (its address is {t.data_ptr() % nbytes} past a multiple of {nbytes}); "
                         f"stgcn_amd.functional.aligned makes the copy")


def _dev_ptr(t: Optional[torch.Tensor], name: str, device=None, dtype=torch.float32, align: int = 0) -> c_void_p:
    """``align``: the operand is a listed exception (ALIGN_LISTED) or a blob (ALIGN_BLOB): refuse it off that boundary."""
    if t is None:
        return c_void_p(0)
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); this path has no CPU implementation")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if align:
        _require_aligned(t, name, align)
    return c_void_p(t.data_ptr())


def _blob_ptr(t: torch.Tensor, name: str) -> c_void_p:
    """A byte blob or workspace (any dtype): ALIGN_BLOB."""
    _require_aligned(t, name, ALIGN_BLOB)
    return c_void_p(t.data_ptr())


def _stream(device) -> c_void_p:
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _flags(math: int, out_bf16: bool) -> int:
    # (MATH_F16MX = MATH_BF16X3 | STEM_F16MX: the extra bit only means something to the stgcn_stem_* entry points)
    return (math & (_capi.MATH_MASK | _capi.STEM_F16MX)) | (OUT_BF16 if out_bf16 else 0)


def bn_fold(weight, bias, running_mean, running_var, conv_bias=None, eps: float = BN_EPS):
    """Eval-mode BatchNorm as per-channel (scale, shift); see stgcn_bn_fold."""
    dev = weight.device
    C = weight.numel()
    scale = torch.empty(C, device=dev, dtype=torch.float32)
    shift = torch.empty(C, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_bn_fold", _dev_ptr(weight, "weight", dev), _dev_ptr(bias, "bias", dev),
                   _dev_ptr(running_mean, "running_mean", dev), _dev_ptr(running_var, "running_var", dev),
                   _dev_ptr(conv_bias, "conv_bias", dev), c_float(eps), _dev_ptr(scale, "scale"),
                   _dev_ptr(shift, "shift"), c_int(C), _stream(dev))
    return scale, shift


def agcn_attention(x, A_eff, Wa, ba, Wb, bb) -> torch.Tensor:
    """P (N,S,V,V) of unit_agcn.py:81-85.  Wa/Wb (S,inter_c,Cin), ba/bb (S,inter_c), A_eff (S,V,V)."""
    dev = x.device
    N, Cin, T, V = x.shape
    S, inter_c, _ = Wa.shape
    P = torch.empty(N, S, V, V, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_agcn_attention", _dev_ptr(x, "x", dev), _dev_ptr(A_eff, "A_eff", dev),
                   _dev_ptr(Wa, "Wa", dev), _dev_ptr(ba, "ba", dev), _dev_ptr(Wb, "Wb", dev),
                   _dev_ptr(bb, "bb", dev), _dev_ptr(P, "P"), c_int(N), c_int(Cin), c_int(T), c_int(V),
                   c_int(inter_c), c_int(S), _stream(dev))
    return P


def agcn_forward(x, A_eff, Wa, ba, Wb, bb, Wd, bd, Wdown, bdown, bn_scale, bn_shift, down_scale,
                 down_shift) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval forward of unit_agcn.  Returns (y (N,Cout,T,V), P (N,S,V,V)).

    Wd (S,Cout,Cin), bd (S,Cout); Wdown (Cout,Cin)/bdown/down_scale/down_shift or all None for
    the identity residual (Cin == Cout).
    """
    dev = x.device
    N, Cin, T, V = x.shape
    S, inter_c, _ = Wa.shape
    Cout = Wd.shape[1]
    y = torch.empty(N, Cout, T, V, device=dev, dtype=torch.float32)
    P = torch.empty(N, S, V, V, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_agcn_forward", _dev_ptr(x, "x", dev), _dev_ptr(A_eff, "A_eff", dev),
                   _dev_ptr(Wa, "Wa", dev), _dev_ptr(ba, "ba", dev), _dev_ptr(Wb, "Wb", dev),
                   _dev_ptr(bb, "bb", dev), _dev_ptr(Wd, "Wd", dev), _dev_ptr(bd, "bd", dev),
                   _dev_ptr(Wdown, "Wdown", dev), _dev_ptr(bdown, "bdown", dev),
                   _dev_ptr(bn_scale, "bn_scale", dev), _dev_ptr(bn_shift, "bn_shift", dev),
                   _dev_ptr(down_scale, "down_scale", dev), _dev_ptr(down_shift, "down_shift", dev),
                   _dev_ptr(P, "P"), _dev_ptr(y, "y"), c_int(N), c_int(Cin), c_int(Cout), c_int(T), c_int(V),
                   c_int(inter_c), c_int(S), _stream(dev))
    return y, P


def agcn_attention_kernel_name(N, Cin, T, V, inter_c, S, extra=0) -> str:
    """Kernel (with template arguments) that computes P; extra: 1 features, 2 fragments, 3 fragments of a wide frame."""
    return _capi.lib().stgcn_agcn_attention_kernel_name(N, Cin, T, V, inter_c, S, extra).decode()


def agcn_expand_kernel_name(N, Cin, Cout, T, V, S, has_down=True) -> str:
    return _capi.lib().stgcn_agcn_expand_kernel_name(N, Cin, Cout, T, V, S, int(has_down)).decode()


def tcn_supported(Cin, Cout, T, V, K, stride, math=MATH_F32) -> bool:
    return bool(_capi.lib().stgcn_tcn_supported(Cin, Cout, T, V, K, stride, _flags(math, False)))


def tcn_out_frames(T: int, K: int, stride: int) -> int:
    pad = int((K - 1) / 2)
    return (T + 2 * pad - K) // stride + 1


def tcn_pack(W, scale, math=MATH_F32) -> torch.Tensor:
    """Pack conv.weight (Cout,Cin,K) * scale into the kernel's operand order; returns a byte buffer."""
    dev = W.device
    Cout, Cin, K = W.shape
    fl = _flags(math, False)
    nbytes = _capi.lib().stgcn_tcn_packed_bytes(Cin, Cout, K, fl)
    Wp = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _capi.call("stgcn_tcn_pack", _dev_ptr(W, "W", dev), _dev_ptr(scale, "scale", dev),
                   c_void_p(Wp.data_ptr()), c_int(Cin), c_int(Cout), c_int(K), c_uint(fl), _stream(dev))
    return Wp


def tcn_forward_packed(x, Wp, shift, Cout, K, stride=1, math=MATH_F32, out_bf16=False, along_v=False) -> torch.Tensor:
    """``along_v``: Unit2D(dim=3) (model/net.py:28-36) — the convolution runs along the joint axis of x (N,Cin,T,V), read in
    place; MATH_F32_VALU packing only; returns (N,Cout,T,V_out)."""
    dev = x.device
    N, Cin, T, V = x.shape
    Lout = tcn_out_frames(V if along_v else T, K, stride)
    if Lout < 1:
        raise ValueError(f"1-D conv: length {V if along_v else T}, K={K}, stride={stride} leaves no output position")
    if along_v and math != MATH_F32_VALU:
        raise ValueError("tcn_forward_packed(along_v=True) needs the MATH_F32_VALU packing")
    shape = (N, Cout, T, Lout) if along_v else (N, Cout, Lout, V)
    y = torch.empty(*shape, device=dev, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    fl = _flags(math, out_bf16) | (_capi.CONV_ALONG_V if along_v else 0)
    with torch.cuda.device(dev):
        _capi.call("stgcn_tcn_forward_packed", _dev_ptr(x, "x", dev), _blob_ptr(Wp, "Wp"),
                   _dev_ptr(shift, "shift", dev), c_void_p(y.data_ptr()), c_int(N), c_int(Cin), c_int(Cout),
                   c_int(T), c_int(V), c_int(K), c_int(stride), c_uint(fl), _stream(dev))
    return y


def tcn_forward(x, W, scale, shift, stride=1, math=MATH_F32, out_bf16=False) -> torch.Tensor:
    """One-shot temporal conv block: packs into a scratch buffer, then runs (stgcn_tcn_forward)."""
    dev = x.device
    N, Cin, T, V = x.shape
    Cout, _, K = W.shape
    Tout = tcn_out_frames(T, K, stride)
    if Tout < 1:
        raise ValueError(f"temporal conv: T={T}, K={K}, stride={stride} leaves no output frame")
    fl = _flags(math, out_bf16)
    nbytes = _capi.lib().stgcn_tcn_packed_bytes(Cin, Cout, K, fl)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    y = torch.empty(N, Cout, Tout, V, device=dev, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_tcn_forward", _dev_ptr(x, "x", dev), _dev_ptr(W, "W", dev),
                   _dev_ptr(scale, "scale", dev), _dev_ptr(shift, "shift", dev), c_void_p(y.data_ptr()),
                   c_int(N), c_int(Cin), c_int(Cout), c_int(T), c_int(V), c_int(K), c_int(stride),
                   c_void_p(ws.data_ptr()), c_size_t(nbytes), c_uint(fl), _stream(dev))
    return y


def stem_supported(Cin, C, T, V, K, S, math=MATH_F32) -> bool:
    return bool(_capi.lib().stgcn_stem_supported(Cin, C, T, V, K, S, _flags(math, False)))


def stem_prepare(Wd, bd, Wdown, bdown, bn_scale, bn_shift, down_scale, down_shift, Wt, t_scale,
                 math=MATH_F32) -> torch.Tensor:
    """Fold + pack everything the fused stem kernel reads besides x/P; returns the prep blob."""
    dev = Wd.device
    S, C, Cin = Wd.shape
    K = Wt.shape[2]
    fl = _flags(math, False)
    nbytes = _capi.lib().stgcn_stem_prep_bytes(Cin, C, K, S, fl)
    prep = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _capi.call("stgcn_stem_prepare", _dev_ptr(Wd, "Wd", dev), _dev_ptr(bd, "bd", dev),
                   _dev_ptr(Wdown, "Wdown", dev), _dev_ptr(bdown, "bdown", dev),
                   _dev_ptr(bn_scale, "bn_scale", dev), _dev_ptr(bn_shift, "bn_shift", dev),
                   _dev_ptr(down_scale, "down_scale", dev), _dev_ptr(down_shift, "down_shift", dev),
                   _dev_ptr(Wt, "Wt", dev), _dev_ptr(t_scale, "t_scale", dev), c_void_p(prep.data_ptr()),
                   c_int(Cin), c_int(C), c_int(K), c_int(S), c_uint(fl), _stream(dev))
    return prep


def _is_channels_last(x: torch.Tensor) -> bool:
    """(N,C,T,V)-shaped tensor whose memory is (N,T,V,C) — what ``x.permute(0,3,1,2)`` of the loader's batch is."""
    return x.dim() == 4 and not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous()


def stem_forward(x, A_eff, Wa, ba, Wb, bb, prep, t_shift, C, K, math=MATH_F32, out_bf16=False,
                 out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                 channels_last_out: bool = False):
    """Fused tcn0(gcn0(x)).  Returns (out (N,C,T,V), P (N,S,V,V) — a view of the workspace).

    x is (N,Cin,T,V), contiguous or channels-last strided (the permuted (N,T,V,Cin) batch of
    ST_GCN_AltFormer.py:62-68 — read in place, STGCN_IN_NTVC).  With ``channels_last_out`` the result is
    still shaped (N,C,T,V) but laid out (N,T,V,C) (STGCN_OUT_NTVC): the rearranges of model_ST.py:152 /
    model_TS.py:161 are views of it."""
    dev = x.device
    N, Cin, T, V = x.shape
    S, inter_c, _ = Wa.shape
    odt = torch.bfloat16 if out_bf16 else torch.float32
    fl = _flags(math, out_bf16)
    if _is_channels_last(x):
        fl |= _capi.IN_NTVC
        x = x.permute(0, 2, 3, 1)              # the contiguous (N,T,V,Cin) tensor behind the view
    oshape = (N, T, V, C) if channels_last_out else (N, C, T, V)
    if channels_last_out:
        fl |= _capi.OUT_NTVC
    if out is None:
        out = torch.empty(oshape, device=dev, dtype=odt)
    elif tuple(out.shape) != oshape or out.dtype != odt or not out.is_contiguous() or out.device != dev:
        raise ValueError("stem_forward: `out` has the wrong shape/dtype/device")
    need = _capi.lib().stgcn_stem_ws_bytes(N, Cin, C, T, V, K, S, fl)
    if ws is None or ws.numel() * ws.element_size() < need or ws.device != dev:
        ws = torch.empty((need + 3) // 4, device=dev, dtype=torch.float32)
    ws_bytes = c_size_t(ws.numel() * ws.element_size())
    st = _stream(dev)
    _require_aligned(prep, "prep", ALIGN_BLOB)        # (both before the first of the two calls)
    with torch.cuda.device(dev):
        _capi.call("stgcn_stem_attention", _dev_ptr(x, "x", dev), _dev_ptr(A_eff, "A_eff", dev),
                   _dev_ptr(Wa, "Wa", dev), _dev_ptr(ba, "ba", dev), _dev_ptr(Wb, "Wb", dev),
                   _dev_ptr(bb, "bb", dev), _dev_ptr(ws, "ws", dev, align=ALIGN_BLOB), ws_bytes, c_int(N), c_int(Cin), c_int(C),
                   c_int(T), c_int(V), c_int(inter_c), c_int(S), c_int(K), c_uint(fl), st)
        timer = kernel_timer
        if timer is not None:
            timer.start("stem_tail", dev)
        _capi.call("stgcn_stem_tail_prepared", _dev_ptr(x, "x", dev), _dev_ptr(ws, "ws", dev), ws_bytes,
                   c_void_p(prep.data_ptr()), _dev_ptr(t_shift, "t_shift", dev), c_void_p(out.data_ptr()),
                   c_int(N), c_int(Cin), c_int(C), c_int(T), c_int(V), c_int(S), c_int(K), c_uint(fl), st)
        if timer is not None:
            timer.stop("stem_tail", dev)
    if channels_last_out:
        out = out.permute(0, 3, 1, 2)          # (N,C,T,V) view, torch.channels_last strides
    return out, ws[:N * S * V * V].view(N, S, V, V)


def agcn_forward_train(x, A_eff, Wa, ba, Wb, bb, Wd, bd, Wdown, bdown, bn, down_bn, momentum=0.1, eps=BN_EPS,
                       save=False, frozen=False):
    """Training-mode forward of unit_agcn (batch-statistics BatchNorm; running buffers of `bn` / `down_bn` are
    updated in place like torch does).  bn / down_bn: (weight, bias, running_mean, running_var) tensors.
    Returns (y, P); with ``save`` (y, P, zm, zd, stats): stats = batch mean / invstd of both BatchNorms (4*Cout) and, on
    the stem class's moments path, the 63 feature moments behind them (STGCN_AGCN_SAVE_STATS_FLOATS);
    zm, zd = the pre-BatchNorm branches, kept only with ``save="branches"`` (else None: the stem shape class then runs
    the moments path, which never writes them, and its backward works from y, dy and the moments).
    ``frozen``: BatchNorm on its RUNNING statistics (eval mode under autograd): nothing is updated; stats = running mean /
    invstd, for agcn_backward_train(..., frozen=True)."""
    dev = x.device
    N, Cin, T, V = x.shape
    S, inter_c, _ = Wa.shape
    Cout = Wd.shape[1]
    y = torch.empty(N, Cout, T, V, device=dev, dtype=torch.float32)
    P = torch.empty(N, S, V, V, device=dev, dtype=torch.float32)
    branches = save == "branches"            # keep zm / zd (the materialising path); save=True keeps the statistics only
    nbytes = _capi.lib().stgcn_agcn_train_ws_bytes(N, Cin, Cout, T, V, S, 1 if (branches or down_bn is None or frozen) else 0)
    ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    d = down_bn if down_bn is not None else (None, None, None, None)
    zm = torch.empty_like(y) if branches else None
    zd = torch.empty_like(y) if branches and down_bn is not None else None
    stats = torch.empty(4 * Cout + 128, device=dev, dtype=torch.float32) if save else None
    with torch.cuda.device(dev):
        _capi.call("stgcn_agcn_forward_train", _dev_ptr(x, "x", dev), _dev_ptr(A_eff, "A_eff", dev),
                   _dev_ptr(Wa, "Wa", dev), _dev_ptr(ba, "ba", dev), _dev_ptr(Wb, "Wb", dev), _dev_ptr(bb, "bb", dev),
                   _dev_ptr(Wd, "Wd", dev), _dev_ptr(bd, "bd", dev), _dev_ptr(Wdown, "Wdown", dev),
                   _dev_ptr(bdown, "bdown", dev), *[_dev_ptr(t, "bn", dev) for t in bn],
                   *[_dev_ptr(t, "down_bn", dev) for t in d], c_float(momentum), c_float(eps), _dev_ptr(P, "P"),
                   c_void_p(ws.data_ptr()), c_size_t(ws.numel() * 8), _dev_ptr(y, "y"), _dev_ptr(zm, "save_zm"),
                   _dev_ptr(zd, "save_zd"), _dev_ptr(stats, "save_stats"), c_int(N), c_int(Cin), c_int(Cout),
                   c_int(T), c_int(V), c_int(inter_c), c_int(S), c_uint(_capi.BN_FROZEN if frozen else 0), _stream(dev))
    return (y, P, zm, zd, stats) if save else (y, P)


def agcn_backward_supported(N, Cin, Cout, T, V, S) -> bool:
    """Any shape the attention kernels cover (V <= 64) has a HIP backward: the fused kernel for the stem class, the GEMM
    chain otherwise."""
    return _capi.lib().stgcn_agcn_backward_ws_bytes(N, Cin, Cout, T, V, S, 3) > 0


def agcn_backward_train(x, A_eff, Wa, ba, Wb, bb, Wd, bd, Wdown, bdown, P, zm, zd, bn_weight, bn_bias, dbn_weight,
                        dbn_bias, stats, dy, need_dx=False, y=None, frozen=False):
    """Gradients of the training-mode unit_agcn forward.  zm / zd: the saved pre-BatchNorm branches, or None.  y: the
    forward's output — with it (and zm = zd = None, stats from a moments-path forward) the stem class runs its
    one-pass moment form; otherwise the GEMM chain, which rebuilds missing branches in the call's workspace.
    Wdown / bdown / dbn_* None = identity residual (Cin == Cout).  ``frozen``: the forward ran on running statistics
    (stats = running mean / invstd): they are constants of the backward (GEMM chain).
    Returns a dict keyed dWa, dba, dWb, dbb, dWd, dbd, dgamma, dbeta, dPA, plus dWdown, dbdown, ddgamma, ddbeta with a
    down branch and dx with ``need_dx`` (the input gradient, model/ST_TR/ST_TR_new.py:355-372)."""
    dev = x.device
    N, Cin, T, V = x.shape
    S, inter_c, _ = Wa.shape
    Cout = Wd.shape[1]
    has_down = Wdown is not None
    # bit 1: size for the generic path whenever the call may take it (dx, identity residual, non-stem shapes).  The one call
    # that cannot - the stem class's moment form, by stgcn_agcn_backward_train's own rule - asks for its own size: the
    # GEMM chain's workspace grows with N*Cout*T*V (58 GiB at 63553 clips of 12 x 22), the moment form's does not.  (The
    # shape test is belt and braces: the query itself answers the chain's size where the moment form does not cover the
    # shape, and the entry point compares the size it is given with the plan it takes.)
    moment_form = not (frozen or not has_down or need_dx or zm is not None or y is None) and Cin == 3 and S == 3
    nbytes = _capi.lib().stgcn_agcn_backward_ws_bytes(N, Cin, Cout, T, V, S, (1 if zm is None else 0) | (0 if moment_form else 2))
    if nbytes == 0:
        raise NotImplementedError(f"unit_agcn backward: shape Cin={Cin} S={S} Cout={Cout} V={V} is not covered by the HIP path")
    ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    g = dict(dWa=f(S, inter_c, Cin), dba=f(S, inter_c), dWb=f(S, inter_c, Cin), dbb=f(S, inter_c), dWd=f(S, Cout, Cin),
             dbd=f(S, Cout), dgamma=f(Cout), dbeta=f(Cout), dPA=f(S, V, V))
    if has_down:
        g.update(dWdown=f(Cout, Cin), dbdown=f(Cout), ddgamma=f(Cout), ddbeta=f(Cout))
    if need_dx:
        g["dx"] = torch.empty_like(x)
    o = lambda k: _dev_ptr(g.get(k), k)
    with torch.cuda.device(dev):
        _capi.call("stgcn_agcn_backward_train", _dev_ptr(x, "x", dev), _dev_ptr(A_eff, "A_eff", dev), _dev_ptr(Wa, "Wa", dev),
                   _dev_ptr(ba, "ba", dev), _dev_ptr(Wb, "Wb", dev), _dev_ptr(bb, "bb", dev), _dev_ptr(Wd, "Wd", dev),
                   _dev_ptr(bd, "bd", dev), _dev_ptr(Wdown, "Wdown", dev), _dev_ptr(bdown, "bdown", dev),
                   _dev_ptr(P, "P", dev), _dev_ptr(zm, "zm", dev), _dev_ptr(zd, "zd", dev),
                   _dev_ptr(bn_weight, "bn_weight", dev), _dev_ptr(bn_bias, "bn_bias", dev),
                   _dev_ptr(dbn_weight, "dbn_weight", dev), _dev_ptr(dbn_bias, "dbn_bias", dev),
                   _dev_ptr(stats, "stats", dev), _dev_ptr(y, "y", dev), _dev_ptr(dy, "dy", dev),
                   *[o(k) for k in ("dWa", "dba", "dWb", "dbb", "dWd", "dbd", "dWdown", "dbdown", "dgamma",
                                    "dbeta", "ddgamma", "ddbeta", "dPA", "dx")],
                   c_void_p(ws.data_ptr()), c_size_t(ws.numel() * 8), c_int(N), c_int(Cin), c_int(Cout), c_int(T),
                   c_int(V), c_int(inter_c), c_int(S), c_uint(_capi.BN_FROZEN if frozen else 0), _stream(dev))
    return g


def tcn_forward_train(x, W, conv_bias, bn, stride=1, math=MATH_F32, momentum=0.1, eps=BN_EPS, save=False, frozen=False):
    """Training-mode forward of Unit2D(dim=2, dropout=0): raw conv -> batch statistics -> normalise -> ReLU.

    ``save=True`` also returns what the backward needs: (y, z = conv_t(x)+b, batch mean, batch invstd).
    ``frozen``: normalise with the RUNNING statistics instead (eval mode under autograd; nothing is updated, mean / invstd
    returned are the running ones)."""
    dev = x.device
    N, Cin, T, V = x.shape
    Cout, _, K = W.shape
    Tout = tcn_out_frames(T, K, stride)
    if Tout < 1:
        raise ValueError(f"temporal conv: T={T}, K={K}, stride={stride} leaves no output frame")
    fl = _flags(math, False) | (_capi.BN_FROZEN if frozen else 0)
    nbytes = _capi.lib().stgcn_tcn_train_ws_bytes(N, Cin, Cout, T, V, K, stride, fl)
    ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    y = torch.empty(N, Cout, Tout, V, device=dev, dtype=torch.float32)
    z = torch.empty_like(y) if save else None
    mean = torch.empty(Cout, device=dev, dtype=torch.float32) if save else None
    invstd = torch.empty(Cout, device=dev, dtype=torch.float32) if save else None
    with torch.cuda.device(dev):
        _capi.call("stgcn_tcn_forward_train", _dev_ptr(x, "x", dev), _dev_ptr(W, "W", dev),
                   _dev_ptr(conv_bias, "conv_bias", dev), *[_dev_ptr(t, "bn", dev) for t in bn], c_float(momentum),
                   c_float(eps), c_void_p(ws.data_ptr()), c_size_t(ws.numel() * 8), _dev_ptr(y, "y"),
                   _dev_ptr(z, "save_z"), _dev_ptr(mean, "save_mean"), _dev_ptr(invstd, "save_invstd"), c_int(N),
                   c_int(Cin), c_int(Cout), c_int(T), c_int(V), c_int(K), c_int(stride), c_uint(fl), _stream(dev))
    return (y, z, mean, invstd) if save else y


def tcn_backward_train(x, W, z, bn_weight, bn_bias, mean, invstd, dy, stride=1, math=MATH_F32, need_dx=True,
                       has_bias=True, frozen=False):
    """Backward of the training-mode Unit2D forward: returns (dx | None, dW (Cout,Cin,K), dbias | None, dgamma, dbeta)."""
    dev = x.device
    N, Cin, T, V = x.shape
    Cout, _, K = W.shape
    fl = _flags(math, False) | (_capi.BN_FROZEN if frozen else 0)   # frozen: mean / invstd are constants (running statistics)
    nbytes = _capi.lib().stgcn_tcn_backward_ws_bytes(N, Cin, Cout, T, V, K, stride, fl)
    ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    dx = torch.empty_like(x) if need_dx else None
    dW = torch.empty_like(W)
    dbias = torch.empty(Cout, device=dev, dtype=torch.float32) if has_bias else None
    dgamma = torch.empty(Cout, device=dev, dtype=torch.float32)
    dbeta = torch.empty(Cout, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_tcn_backward_train", _dev_ptr(x, "x", dev), _dev_ptr(W, "W", dev), _dev_ptr(z, "z", dev),
                   _dev_ptr(bn_weight, "bn_weight", dev), _dev_ptr(bn_bias, "bn_bias", dev), _dev_ptr(mean, "mean", dev),
                   _dev_ptr(invstd, "invstd", dev), _dev_ptr(dy, "dy", dev), _dev_ptr(dx, "dx"), _dev_ptr(dW, "dW"),
                   _dev_ptr(dbias, "dbias"), _dev_ptr(dgamma, "dgamma"), _dev_ptr(dbeta, "dbeta"),
                   c_void_p(ws.data_ptr()), c_size_t(ws.numel() * 8), c_int(N), c_int(Cin), c_int(Cout), c_int(T), c_int(V),
                   c_int(K), c_int(stride), c_uint(fl), _stream(dev))
    return dx, dW, dbias, dgamma, dbeta


def patch_embed(z, weight, bias, pos=None, order="ST"):
    """First patch embedding of the transformer heads applied to the stem output z (N,C,T,V) — contiguous, or
    channels-last strided as the fused stem writes it with ``set_output_layout(..., "channels_last")``:

      order "ST": ``rearrange(z,'b c f p -> (b f) p c')`` -> ``nn.Linear(C,E)`` -> ``+= Spatial_pos_embed``
                  (model/AltFormer/model_ST.py:152-155)  -> (N*T, V, E)
      order "TS": ``rearrange(z,'b c f p -> (b p) f c')`` -> ``nn.Linear(C,E)`` -> ``+= Temporal_pos_embed``
                  (model/AltFormer/model_TS.py:161-163)  -> (N*V, T, E)

    One strided GEMM per clip (stgcn_patch_embed): the rearrange is folded into the addressing.  ``weight`` (E,C),
    ``bias`` (E), ``pos`` (1,V,E) / (1,T,E) or None."""
    dev = z.device
    N, C, T, V = z.shape
    E = weight.shape[0]
    fl = 0
    if _is_channels_last(z):
        fl |= _capi.IN_NTVC
        z = z.permute(0, 2, 3, 1)
    if order == "TS":
        fl |= _capi.EMBED_TS
    elif order != "ST":
        raise ValueError(f"order must be 'ST' or 'TS' (got {order!r})")
    if pos is not None:
        want = (T if order == "TS" else V) * E
        if pos.numel() != want:
            raise ValueError(f"pos has {pos.numel()} elements, expected {want}")
        pos = pos.reshape(-1, E)
    out = torch.empty((N * V, T, E) if order == "TS" else (N * T, V, E), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_patch_embed", _dev_ptr(z, "z", dev), _dev_ptr(weight, "weight", dev), _dev_ptr(bias, "bias", dev),
                   _dev_ptr(pos, "pos", dev), _dev_ptr(out, "out"), c_int(N), c_int(C), c_int(E), c_int(T), c_int(V),
                   c_uint(fl), _stream(dev))
    return out


class KernelTimer:
    """HIP-event bracket around individual kernel launches on the launching stream.

    Assign an instance to ``functional.kernel_timer`` to have the wrappers record an event pair per
    launch (no synchronisation while recording); ``mean_ms(name)`` synchronises and averages.
    """

    def __init__(self):
        self.pairs = {}
        self._open = {}

    def start(self, name, dev):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(dev))
        self._open[name] = ev

    def stop(self, name, dev):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(dev))
        self.pairs.setdefault(name, []).append((self._open.pop(name), ev))

    def reset(self):
        self.pairs.clear()
        self._open.clear()

    def count(self, name):
        return len(self.pairs.get(name, []))

    def mean_ms(self, name):
        pairs = self.pairs.get(name, [])
        if not pairs:
            return None
        pairs[-1][1].synchronize()
        return sum(a.elapsed_time(b) for a, b in pairs) / len(pairs)


kernel_timer: Optional[KernelTimer] = None


# ---- ST-TR spatial self-attention unit (gcn_unit_attention) --------------------------------------------------------------
def st_attention_supported(Cin, Cout, dk, V, heads) -> bool:
    return bool(_capi.lib().stgcn_st_attention_supported(Cin, Cout, dk, V, heads))


def _st_ws(dev, N, Cin, Cout, dk, T, V, heads, pass_):
    nbytes = _capi.lib().stgcn_st_attention_ws_bytes(N, Cin, Cout, dk, T, V, heads, pass_)
    return torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64), nbytes


def st_attention_math_supported(Cin, Cout, dk, V, heads, math=MATH_F32) -> bool:
    return bool(_capi.lib().stgcn_st_attention_math_supported(Cin, Cout, dk, V, heads, math & _capi.MATH_MASK))


def wx_product_supported(M, K, TV, math=MATH_F32) -> bool:
    return bool(_capi.lib().stgcn_wx_product_supported(M, K, TV, math))


def wx_product_kernel_name(M, K, TV, math=MATH_F32) -> str:
    return _capi.lib().stgcn_wx_product_kernel_name(M, K, TV, math).decode()


def wx_product(W, X, bias=None, R=None, w_transposed=False, math=MATH_F32) -> torch.Tensor:
    """C[n] = W . X[n] (+ bias per row) (+ R[n]): the product of gcn_unit_attention's 1x1 projections on its own.  X (N,K,TV),
    W (M,K), or (K,M) with ``w_transposed``; R (N,M,TV) or None.  ``math``: MATH_F32 (the strided fp32 GEMM) or MATH_BF16X3
    (three-term bf16 split, stgcn_wx_product).  Returns C (N,M,TV)."""
    dev = X.device
    N, K, TV = X.shape
    M = W.shape[1] if w_transposed else W.shape[0]
    nbytes = _capi.lib().stgcn_wx_product_ws_bytes(M, K, math)
    ws = _bytes(dev, nbytes) if nbytes else None
    C = torch.empty(N, M, TV, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_wx_product", _dev_ptr(W, "W", dev), _dev_ptr(X, "X", dev), _dev_ptr(bias, "bias", dev),
                   _dev_ptr(R, "R", dev), _dev_ptr(C, "C"), c_void_p(ws.data_ptr() if ws is not None else None),
                   c_size_t(nbytes), c_int(N), c_int(M), c_int(K), c_longlong(TV), c_int(1 if w_transposed else 0),
                   c_uint(math), _stream(dev))
    return C


def st_attention_forward(x, dbn_scale, dbn_shift, Wqkv, bqkv, Wout, bout, bn_scale, bn_shift, dk, heads,
                         math=MATH_F32) -> torch.Tensor:
    """Eval forward of gcn_unit_attention with both BatchNorms folded (data_bn over Cin*V channels).  Wqkv (2dk+Cout, Cin),
    Wout (Cout, Cout).  ``math``: MATH_F32, or MATH_BF16X3 for the two projections (stgcn_st_attention_forward_math).
    Returns y (N,Cout,T,V)."""
    dev = x.device
    N, Cin, T, V = x.shape
    Cout = Wout.shape[0]
    ws, nbytes = _st_ws(dev, N, Cin, Cout, dk, T, V, heads, 0)
    y = torch.empty(N, Cout, T, V, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        head = (_dev_ptr(x, "x", dev), _dev_ptr(dbn_scale, "dbn_scale", dev),
                _dev_ptr(dbn_shift, "dbn_shift", dev), _dev_ptr(Wqkv, "Wqkv", dev), _dev_ptr(bqkv, "bqkv", dev),
                _dev_ptr(Wout, "Wout", dev), _dev_ptr(bout, "bout", dev), _dev_ptr(bn_scale, "bn_scale", dev),
                _dev_ptr(bn_shift, "bn_shift", dev), c_void_p(ws.data_ptr()), c_size_t(nbytes), _dev_ptr(y, "y"),
                c_int(N), c_int(Cin), c_int(Cout), c_int(dk), c_int(T), c_int(V), c_int(heads))
        if math == MATH_F32:
            _capi.call("stgcn_st_attention_forward", *head, _stream(dev))
        else:
            _capi.call("stgcn_st_attention_forward_math", *head, c_uint(math), _stream(dev))
    return y


def st_attention_forward_train(x, data_bn, Wqkv, bqkv, Wout, bout, bn, mask, dk, heads, momentum=0.1, eps=BN_EPS,
                               frozen=False, math=MATH_F32):
    """Training forward (batch statistics, or running ones with ``frozen``; ``math``: MATH_F32 or MATH_BF16X3 for the two
    projections - the backward must be given the same).  ``data_bn`` / ``bn``: (weight, bias,
    running_mean, running_var); ``mask`` (N*T*heads*V) of 0 / 1, or None.  Returns (y, saved) with saved = dict of the
    tensors stgcn_st_attention_backward reads."""
    dev = x.device
    N, Cin, T, V = x.shape
    Cout = Wout.shape[0]
    Cq = Wqkv.shape[0]
    ws, nbytes = _st_ws(dev, N, Cin, Cout, dk, T, V, heads, 1)
    f32 = dict(device=dev, dtype=torch.float32)
    y = torch.empty(N, Cout, T, V, **f32)
    sv = {"qkv": torch.empty(N, Cq, T, V, **f32), "o": torch.empty(N, Cout, T, V, **f32),
          "z": torch.empty(N, Cout, T, V, **f32), "rowstats": torch.empty(N * T * heads * V, 4, **f32),
          "stats": torch.empty(2 * Cin * V + 2 * Cout, **f32)}
    with torch.cuda.device(dev):
        _capi.call("stgcn_st_attention_forward_train", _dev_ptr(x, "x", dev),
                   *[_dev_ptr(t, "data_bn", dev) for t in data_bn], _dev_ptr(Wqkv, "Wqkv", dev), _dev_ptr(bqkv, "bqkv", dev),
                   _dev_ptr(Wout, "Wout", dev), _dev_ptr(bout, "bout", dev), *[_dev_ptr(t, "bn", dev) for t in bn],
                   _dev_ptr(mask, "mask", dev), c_float(momentum), c_float(eps), c_void_p(ws.data_ptr()), c_size_t(nbytes),
                   _dev_ptr(y, "y"), *[_dev_ptr(sv[k], k) for k in ("qkv", "o", "z", "rowstats", "stats")], c_int(N),
                   c_int(Cin), c_int(Cout), c_int(dk), c_int(T), c_int(V), c_int(heads),
                   c_uint((_capi.BN_FROZEN if frozen else 0) | math), _stream(dev))
    return y, sv


def st_attention_backward(x, dbn_weight, dbn_bias, Wqkv, Wout, bn_weight, bn_bias, mask, saved, dy, dk, heads,
                          need_dx=True, frozen=False, math=MATH_F32):
    """Backward of st_attention_forward_train (same ``frozen`` and ``math``: the latter runs the two input-gradient products
    in that arithmetic, the weight gradients stay fp32).  Returns a dict: dx (or None), ddbn_weight, ddbn_bias (Cin*V), dWqkv, dbqkv,
    dWout, dbout, dbn_weight, dbn_bias."""
    dev = x.device
    N, Cin, T, V = x.shape
    Cout = Wout.shape[0]
    ws, nbytes = _st_ws(dev, N, Cin, Cout, dk, T, V, heads, 2)
    g = {"dx": torch.empty_like(x) if need_dx else None,
         "ddbn_weight": torch.empty_like(dbn_weight), "ddbn_bias": torch.empty_like(dbn_bias),
         "dWqkv": torch.empty_like(Wqkv), "dbqkv": torch.empty(Wqkv.shape[0], device=dev, dtype=torch.float32),
         "dWout": torch.empty_like(Wout), "dbout": torch.empty(Cout, device=dev, dtype=torch.float32),
         "dbn_weight": torch.empty_like(bn_weight), "dbn_bias": torch.empty_like(bn_bias)}
    with torch.cuda.device(dev):
        _capi.call("stgcn_st_attention_backward", _dev_ptr(x, "x", dev), _dev_ptr(dbn_weight, "dbn_weight", dev),
                   _dev_ptr(dbn_bias, "dbn_bias", dev), _dev_ptr(Wqkv, "Wqkv", dev), _dev_ptr(Wout, "Wout", dev),
                   _dev_ptr(bn_weight, "bn_weight", dev), _dev_ptr(bn_bias, "bn_bias", dev), _dev_ptr(mask, "mask", dev),
                   *[_dev_ptr(saved[k], k, dev) for k in ("qkv", "o", "z", "rowstats", "stats")], _dev_ptr(dy, "dy", dev),
                   *[_dev_ptr(g[k], k) for k in ("dx", "ddbn_weight", "ddbn_bias", "dWqkv", "dbqkv", "dWout", "dbout",
                                                  "dbn_weight", "dbn_bias")],
                   c_void_p(ws.data_ptr()), c_size_t(nbytes), c_int(N), c_int(Cin), c_int(Cout), c_int(dk), c_int(T),
                   c_int(V), c_int(heads), c_uint((_capi.BN_FROZEN if frozen else 0) | math), _stream(dev))
    return g


# ---- AltFormer heads: transformer block (stgcn_vit_*) ---------------------------------------------------------------------
def _vit_flags(math: int) -> int:
    return math & (_capi.MATH_MASK | _capi.VIT_QKV_F32 | _capi.VIT_TILE_MASK | _capi.VIT_BF16 | _capi.VIT_ATTN_SPLIT)


def _vit_train_flags(math: int, small: bool = False) -> int:
    """What the training entry points read of ``math``: the inference bits (which they refuse by name), VIT_TRAIN_BF16 and
    VIT_TRAIN_ATTN_BF16.  ``small``: the caller is the ``_drop`` pair (or ``vit_linear_backward``, which masks for itself), the
    entry points that know VIT_WGRAD_SMALL; to the older pair the bit never travels."""
    return _vit_flags(math) | (math & (_capi.VIT_TRAIN_BF16 | _capi.VIT_TRAIN_ATTN_BF16 | (_capi.VIT_WGRAD_SMALL if small else 0)))


def vit_wgrad_plan(M, K, Nout, math=0):
    """``(tile, splits, writes_direct)`` of the weight gradient of a linear over ``M`` tokens, ``dW`` (Nout, K): the form
    (128 or 64) and the token splits the library picks, and whether the kernel stores ``dW`` itself.  Only VIT_WGRAD_SMALL
    of ``math`` is read; without it the answer is the 128 form on the uniform cut.  A host function: no GPU needed."""
    lib, fl = _capi.lib(), math & _capi.VIT_WGRAD_SMALL
    return (lib.stgcn_vit_wgrad_tile(M, K, Nout, fl), lib.stgcn_vit_wgrad_splits(M, K, Nout, fl),
            bool(lib.stgcn_vit_wgrad_writes_direct(M, K, Nout, fl)))


def _bytes(dev, nbytes):
    return torch.empty((max(nbytes, 8) + 7) // 8, device=dev, dtype=torch.float64)


def vit_linear_supported(M, K, Nout, math=MATH_F32) -> bool:
    return bool(_capi.lib().stgcn_vit_linear_supported(M, K, Nout, math & _capi.MATH_MASK))


def vit_linear_tile(M, K, Nout, math=MATH_F32):
    """The tile ``(BM, BN)`` of the linear kernel that ``math`` (its ``VIT_TILE_*`` field) gives this shape; None if the linear
    does not cover it.  A host function: no GPU needed."""
    t = _capi.lib().stgcn_vit_linear_tile(M, K, Nout, math & (_capi.MATH_MASK | _capi.VIT_TILE_MASK))
    return (t >> 16, t & 0xFFFF) if t else None


def vit_linear(x, weight, bias=None, ln=None, residual=None, gelu=False, math=MATH_F32, y=None) -> torch.Tensor:
    """``act(LN?(x) W^T + b) (+ residual)`` on the last axis of x (..., K); weight (Nout, K) as nn.Linear stores it.
    ``ln`` = (weight, bias, eps) of a LayerNorm over K applied to x's rows first, or None; ``gelu``: exact GELU.
    ``math`` may carry a ``VIT_TILE_*`` field (the result does not depend on it).  ``y``: write here (may be ``residual``)."""
    dev = x.device
    K = x.shape[-1]
    M = x.numel() // K
    Nout = weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError(f"weight is {tuple(weight.shape)}, x has {K} features")
    if residual is not None and residual.numel() != M * Nout:
        raise ValueError(f"residual has {residual.numel()} elements, expected {M * Nout}")
    if y is None:
        y = torch.empty(x.shape[:-1] + (Nout,), device=dev, dtype=torch.float32)
    elif y.shape != x.shape[:-1] + (Nout,):
        raise ValueError(f"y is {tuple(y.shape)}, expected {tuple(x.shape[:-1]) + (Nout,)}")
    elif y.data_ptr() == x.data_ptr():
        raise ValueError("y must not alias x")
    lnw, lnb, eps = ln if ln is not None else (None, None, 0.0)
    fl = (math & (_capi.MATH_MASK | _capi.VIT_TILE_MASK)) | (_capi.VIT_GELU if gelu else 0)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_linear", _dev_ptr(x, "x", dev), _dev_ptr(weight, "weight", dev), _dev_ptr(bias, "bias", dev),
                   _dev_ptr(lnw, "ln weight", dev), _dev_ptr(lnb, "ln bias", dev), c_float(eps),
                   _dev_ptr(residual, "residual", dev), _dev_ptr(y, "y", dev), c_int(M), c_int(K), c_int(Nout), c_uint(fl), _stream(dev))
    return y


def vit_linear_bf16(x, weight, bias=None, ln=None, residual=None, gelu=False, y_bf16=False, tile=0, y=None) -> torch.Tensor:
    """``vit_linear`` in the bf16 arithmetic of the ``VIT_BF16`` block mode: x and the weight rounded to nearest-even bf16 as
    matrix-core operands, fp32 accumulate, LayerNorm / bias / GELU / residual in fp32.  x is float32 or ``torch.bfloat16``
    (bf16 storage, read as it is; no ``ln`` then); the result is ``torch.bfloat16`` with ``y_bf16`` (or a bfloat16 ``y``),
    else float32.  ``tile``: a ``VIT_TILE_*`` field (the result does not depend on it)."""
    dev = x.device
    K = x.shape[-1]
    M = x.numel() // K
    Nout = weight.shape[0]
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"x must be float32 or bfloat16 (got {x.dtype})")
    if weight.shape[1] != K:
        raise ValueError(f"weight is {tuple(weight.shape)}, x has {K} features")
    if residual is not None and residual.numel() != M * Nout:
        raise ValueError(f"residual has {residual.numel()} elements, expected {M * Nout}")
    if y is None:
        y = torch.empty(x.shape[:-1] + (Nout,), device=dev, dtype=torch.bfloat16 if y_bf16 else torch.float32)
    elif y.shape != x.shape[:-1] + (Nout,) or y.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"y is {tuple(y.shape)} {y.dtype}, expected {tuple(x.shape[:-1]) + (Nout,)} float32 or bfloat16")
    elif y.data_ptr() == x.data_ptr():
        raise ValueError("y must not alias x")
    lnw, lnb, eps = ln if ln is not None else (None, None, 0.0)
    fl = (tile & _capi.VIT_TILE_MASK) | (_capi.VIT_GELU if gelu else 0) \
        | (_capi.VIT_X_BF16 if x.dtype == torch.bfloat16 else 0) | (_capi.VIT_Y_BF16 if y.dtype == torch.bfloat16 else 0)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_linear_bf16", _dev_ptr(x, "x", dev, x.dtype), _dev_ptr(weight, "weight", dev),
                   _dev_ptr(bias, "bias", dev), _dev_ptr(lnw, "ln weight", dev), _dev_ptr(lnb, "ln bias", dev), c_float(eps),
                   _dev_ptr(residual, "residual", dev), _dev_ptr(y, "y", dev, y.dtype), c_int(M), c_int(K), c_int(Nout),
                   c_uint(fl), _stream(dev))
    return y


def vit_attention_bf16_supported(L, heads, head_dim) -> bool:
    return bool(_capi.lib().stgcn_vit_attention_bf16_supported(L, heads, head_dim))


def vit_attention_bf16(qkv, heads, scale=None) -> torch.Tensor:
    """``vit_attention`` (the resident form, L <= 256) on a ``torch.bfloat16`` packed qkv (B, L, 3*D); returns bfloat16
    (B, L, D).  Scores, soft-max and sums in fp32; exp(s - max) is rounded to bf16 as the operand of P V."""
    dev = qkv.device
    B, L, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    if D * 3 != D3 or hd * heads != D:
        raise ValueError(f"qkv is {tuple(qkv.shape)}: the last axis must be 3 * heads * head_dim (heads = {heads})")
    out = torch.empty(B, L, D, device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_attention_bf16", _dev_ptr(qkv, "qkv", dev, torch.bfloat16), _dev_ptr(out, "out", None, torch.bfloat16),
                   c_int(B), c_int(L), c_int(heads), c_int(hd), c_float(hd ** -0.5 if scale is None else scale), _stream(dev))
    return out


def vit_block_forward_bf16_supported(L, D, heads, hidden) -> bool:
    """What ``vit_block_forward`` runs with ``VIT_BF16``: the resident coverage (L <= 256)."""
    return bool(_capi.lib().stgcn_vit_block_forward_bf16_supported(L, D, heads, hidden))


def vit_attention_supported(L, heads, head_dim) -> bool:
    """The resident kernel's coverage (L <= 256), which is also the training entry points'."""
    return bool(_capi.lib().stgcn_vit_attention_supported(L, heads, head_dim))


def vit_attention_stream_supported(L, heads, head_dim) -> bool:
    """The streaming kernel's coverage (L <= 4096)."""
    return bool(_capi.lib().stgcn_vit_attention_stream_supported(L, heads, head_dim))


def _vit_attention(entry, qkv, heads, scale):
    dev = qkv.device
    B, L, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    if D * 3 != D3 or hd * heads != D:
        raise ValueError(f"qkv is {tuple(qkv.shape)}: the last axis must be 3 * heads * head_dim (heads = {heads})")
    out = torch.empty(B, L, D, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call(entry, _dev_ptr(qkv, "qkv", dev), _dev_ptr(out, "out"), c_int(B), c_int(L), c_int(heads),
                   c_int(hd), c_float(hd ** -0.5 if scale is None else scale), _stream(dev))
    return out


def vit_attention(qkv, heads, scale=None) -> torch.Tensor:
    """Multi-head attention over the packed qkv (B, L, 3*D) = (B, L, 3, heads, D/heads) as the qkv nn.Linear writes it;
    returns (B, L, D), heads concatenated.  ``scale`` defaults to head_dim ** -0.5.  Sequences of up to 256 tokens run the
    resident kernel, longer ones (up to 4096) the streaming one."""
    L, hd = qkv.shape[1], qkv.shape[2] // 3 // heads
    stream = not vit_attention_supported(L, heads, hd) and vit_attention_stream_supported(L, heads, hd)
    return _vit_attention("stgcn_vit_attention_stream" if stream else "stgcn_vit_attention", qkv, heads, scale)


def vit_attention_train_bf16_supported(L, heads, head_dim) -> bool:
    """Coverage of ``vit_attention_train_bf16`` / ``vit_attention_backward_bf16``: the resident lengths (L <= 256)."""
    return bool(_capi.lib().stgcn_vit_attention_train_bf16_supported(L, heads, head_dim))


def vit_attention_train_bf16(qkv, heads, scale=None) -> torch.Tensor:
    """The training forward's attention of ``VIT_TRAIN_ATTN_BF16`` on a float32 packed qkv (B, L, 3*D); returns float32
    (B, L, D).  Scores as three bf16 products of the split q and k, exp(s - max) and v rounded to bf16 for P V, sums in fp32."""
    return _vit_attention("stgcn_vit_attention_train_bf16", qkv, heads, scale)


def vit_attention_stream(qkv, heads, scale=None) -> torch.Tensor:
    """``vit_attention`` on the streaming kernel (K and V in key tiles through LDS, running soft-max) at every covered
    length, the short ones included: the same result up to the summation order."""
    return _vit_attention("stgcn_vit_attention_stream", qkv, heads, scale)


def vit_attention_split_supported(L, heads, head_dim) -> bool:
    """Coverage of ``vit_attention_split``: the resident lengths (L <= 256)."""
    return bool(_capi.lib().stgcn_vit_attention_split_supported(L, heads, head_dim))


def vit_attention_split(qkv, heads, scale=None) -> torch.Tensor:
    """``vit_attention`` (L <= 256) on the split kernel, whatever the batch: a workgroup per (sequence, head, 32 queries), a
    wave per tile of 32 keys, the waves' partial soft-maxes merged in a fixed order.  The same result up to the summation
    order; made for calls of a few clips, where the resident kernel leaves most of the device idle."""
    return _vit_attention("stgcn_vit_attention_split", qkv, heads, scale)


ATTENTION_FORMS = {0: None, 1: "resident", 2: "stream", 3: "resident_bf16", 4: "resident_split"}


def vit_block_attention_form(B, L, D, heads, hidden, math=MATH_F32):
    """The attention kernel ``vit_block_forward`` runs for this call with ``math`` (an ``ATTENTION_FORMS`` value; None: not
    covered, or the flags are refused).  A host function: no GPU needed."""
    return ATTENTION_FORMS[_capi.lib().stgcn_vit_block_attention_form(B, L, D, heads, hidden, _vit_flags(math))]


def vit_block_supported(L, D, heads, hidden) -> bool:
    """Coverage of the resident form (L <= 256): what the training entry points take."""
    return bool(_capi.lib().stgcn_vit_block_supported(L, D, heads, hidden))


def vit_block_forward_supported(L, D, heads, hidden) -> bool:
    """What ``vit_block_forward`` runs: the resident coverage plus 256 < L <= 4096 on the streaming attention kernel."""
    return bool(_capi.lib().stgcn_vit_block_forward_supported(L, D, heads, hidden))


def vit_block_forward(x, norm1, qkv, proj, norm2, fc1, fc2, heads, eps, scale, math=MATH_F32) -> torch.Tensor:
    """Eval forward of one transformer Block on x (B, L, D).  ``norm1`` / ``norm2`` = (weight, bias) of the LayerNorms (one
    ``eps``), ``qkv`` / ``proj`` / ``fc1`` / ``fc2`` = (weight, bias or None) of the nn.Linears as stored.  ``math``: MATH_F32
    or MATH_BF16X3, optionally | VIT_QKV_F32, optionally | a VIT_TILE_* form for the four linears (same result, bit for bit);
    or VIT_BF16 (optionally | a VIT_TILE_* form): the whole block on bf16 operands, L <= 256 (``vit_block_forward_bf16_supported``).
    Any of them optionally | VIT_ATTN_SPLIT: the fp32 resident attention in its split form where the call has few
    (sequence, head) pairs (``vit_block_attention_form`` tells)."""
    dev = x.device
    B, L, D = x.shape
    hidden = fc1[0].shape[0]
    nbytes = _capi.lib().stgcn_vit_block_ws_bytes(B, L, D, hidden)
    ws = _bytes(dev, nbytes)
    y = torch.empty_like(x)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_block_forward", _dev_ptr(x, "x", dev), _dev_ptr(norm1[0], "norm1.weight", dev),
                   _dev_ptr(norm1[1], "norm1.bias", dev), _dev_ptr(qkv[0], "qkv.weight", dev), _dev_ptr(qkv[1], "qkv.bias", dev),
                   _dev_ptr(proj[0], "proj.weight", dev), _dev_ptr(proj[1], "proj.bias", dev),
                   _dev_ptr(norm2[0], "norm2.weight", dev), _dev_ptr(norm2[1], "norm2.bias", dev),
                   _dev_ptr(fc1[0], "fc1.weight", dev), _dev_ptr(fc1[1], "fc1.bias", dev), _dev_ptr(fc2[0], "fc2.weight", dev),
                   _dev_ptr(fc2[1], "fc2.bias", dev), c_float(eps), c_float(scale), c_void_p(ws.data_ptr()), c_size_t(nbytes),
                   _dev_ptr(y, "y"), c_int(B), c_int(L), c_int(D), c_int(heads), c_int(hidden), c_uint(_vit_flags(math)),
                   _stream(dev))
    return y


# ---- AltFormer heads: the whole head (stgcn_vit_pool, stgcn_vit_pool_classify, stgcn_altformer_head_*) -----------------------
def vit_pool_supported(S, L, D) -> bool:
    return bool(_capi.lib().stgcn_vit_pool_supported(S, L, D))


_POOL_FLAGS = {"mean": 0, "max": _capi.VIT_POOL_MAX, "cls": _capi.VIT_POOL_CLS}


def _pool_flags(mode) -> int:
    if mode not in _POOL_FLAGS:
        raise ValueError(f"mode must be 'mean', 'max' or 'cls' (got {mode!r})")
    return _POOL_FLAGS[mode]


def vit_pool(x, mode="mean") -> torch.Tensor:
    """The mean (``sum / L``), the maximum over the tokens, or token 0 of every sequence of x (S, L, D) -> (S, D); ``mode``:
    'mean' | 'max' | 'cls'.  The maximum equals ``x.max(dim=1).values`` and 'cls' equals ``x[:, 0]`` bit for bit."""
    fl = _pool_flags(mode)
    dev = x.device
    S, L, D = x.shape
    out = torch.empty((S, D), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_pool", _dev_ptr(x, "x", dev, align=ALIGN_LISTED), _dev_ptr(out, "out"), c_int(S), c_int(L), c_int(D),
                   c_uint(fl), _stream(dev))
    return out


def vit_pool_classify_supported(N, L, D, classes) -> bool:
    return bool(_capi.lib().stgcn_vit_pool_classify_supported(N, L, D, classes))


def vit_pool_classify(x, ln_weight, ln_bias, eps, weight, bias=None, mode="max", logits=None) -> torch.Tensor:
    """``Linear(LayerNorm(pool(x)))`` on x (N, L, D) -> (N, classes): the pooling of ``vit_pool`` over L, an affine LayerNorm
    over D (biased variance, ``eps`` inside the root), ``weight`` (classes, D) and ``bias`` as nn.Linear stores them."""
    fl = _pool_flags(mode)
    dev = x.device
    N, L, D = x.shape
    classes = weight.shape[0]
    if weight.shape[1] != D or ln_weight.numel() != D or ln_bias.numel() != D:
        raise ValueError(f"weight is {tuple(weight.shape)}, the LayerNorm has {ln_weight.numel()} features, x has {D}")
    if logits is None:
        logits = torch.empty((N, classes), device=dev, dtype=torch.float32)
    elif logits.shape != (N, classes):
        raise ValueError(f"logits is {tuple(logits.shape)}, expected {(N, classes)}")
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_pool_classify", _dev_ptr(x, "x", dev, align=ALIGN_LISTED), _dev_ptr(ln_weight, "ln weight", dev),
                   _dev_ptr(ln_bias, "ln bias", dev), c_float(eps), _dev_ptr(weight, "weight", dev, align=ALIGN_LISTED),
                   _dev_ptr(bias, "bias", dev),
                   _dev_ptr(logits, "logits", dev), c_int(N), c_int(L), c_int(D), c_int(classes),
                   c_uint(fl), _stream(dev))
    return logits


# ---- The ST-ViT head: patch embedding with the class row (stgcn_vit_patch_embed) ----------------------------------------------
def _patch_flags(math: int, channels_last: bool) -> int:
    """The embedding's arithmetic from a block's flag word: f32 stays f32, everything else - bf16x3, 'mixed', and the
    blocks' bf16 mode, for which the embedding has no kernel - runs bf16x3."""
    low = MATH_F32 if not (math & VIT_BF16) and (math & _capi.MATH_MASK) == MATH_F32 else MATH_BF16X3
    return low | (_capi.IN_NTVC if channels_last else 0)


def vit_patch_embed_supported(N, C, T, V, p1, p2, E, math=MATH_F32, channels_last=False) -> bool:
    """Whether ``vit_patch_embed`` runs this shape.  A host function: no GPU needed."""
    return bool(_capi.lib().stgcn_vit_patch_embed_supported(N, C, T, V, p1, p2, E, _patch_flags(math, channels_last)))


def vit_patch_embed_ws_bytes(N, C, T, V, p1, p2, E, math=MATH_F32, channels_last=False) -> int:
    return int(_capi.lib().stgcn_vit_patch_embed_ws_bytes(N, C, T, V, p1, p2, E, _patch_flags(math, channels_last)))


def vit_patch_embed_cut(N, C, T, V, p1, p2, E, math=MATH_F32, channels_last=False):
    """``(tile rows, parts of K)`` the plan gives this call, or None where it is not covered.  A host function."""
    c = _capi.lib().stgcn_vit_patch_embed_cut(N, C, T, V, p1, p2, E, _patch_flags(math, channels_last))
    return (c >> 16, c & 0xFFFF) if c else None


def vit_patch_embed(z, weight, bias, cls, pos, p1, p2, math=MATH_F32) -> torch.Tensor:
    """The ST-ViT head's patch embedding of the stem output z (N, C, T, V) - contiguous, or channels-last strided as the fused
    stem writes it, consumed in place - with the class row and the position table: x (N, n + 1, E), n = (T / p1) (V / p2),

        x[:, 0] = cls + pos[0],   x[:, 1 + a w + b] = patch(a, b) W^T + bias + pos[1 + a w + b],

    patch(a, b)[(f p2 + j) C + c] = z[:, c, a p1 + f, b p2 + j].  ``weight`` (E, p1 p2 C) and ``bias`` (E or None) as
    nn.Linear stores them, ``cls`` E elements, ``pos`` the first n + 1 rows of the position table ((n + 1) E elements) or
    None.  ``math``: MATH_F32 or MATH_BF16X3 (a block's flag word is accepted: see ``_patch_flags``)."""
    dev = z.device
    N, C, T, V = z.shape
    E = weight.shape[0]
    if T % p1 or V % p2:
        raise ValueError(f"T = {T}, V = {V} are not whole patches of {p1} x {p2}")
    n = (T // p1) * (V // p2)
    if weight.shape[1] != p1 * p2 * C or cls.numel() != E or (bias is not None and bias.numel() != E):
        raise ValueError(f"weight is {tuple(weight.shape)}, cls has {cls.numel()} elements; expected ({E}, {p1 * p2 * C}) and {E}")
    if pos is not None:
        if pos.numel() != (n + 1) * E:
            raise ValueError(f"pos has {pos.numel()} elements, expected {(n + 1) * E}")
        pos = pos.reshape(n + 1, E)
    channels_last = _is_channels_last(z)
    if channels_last:
        z = z.permute(0, 2, 3, 1)
    fl = _patch_flags(math, channels_last)
    nbytes = int(_capi.lib().stgcn_vit_patch_embed_ws_bytes(N, C, T, V, p1, p2, E, fl))
    ws = _bytes(dev, nbytes)
    x = torch.empty((N, n + 1, E), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_patch_embed", _dev_ptr(z, "z", dev, align=ALIGN_LISTED),
                   _dev_ptr(weight, "weight", dev, align=ALIGN_LISTED), _dev_ptr(bias, "bias", dev),
                   _dev_ptr(cls.reshape(-1), "cls", dev), _dev_ptr(pos, "pos", dev), _dev_ptr(x, "x"), c_int(N), c_int(C), c_int(T),
                   c_int(V), c_int(p1), c_int(p2), c_int(E), c_void_p(ws.data_ptr()), c_size_t(nbytes), c_uint(fl), _stream(dev))
    return x


# ---- The ST-ViT head: training the two ends (stgcn_vit_patch_embed_backward, stgcn_vit_pool_classify_backward) ------------------
def vit_patch_embed_backward_supported(N, C, T, V, p1, p2, E, math=MATH_F32, channels_last=False) -> bool:
    """Whether ``vit_patch_embed_backward`` runs this shape.  A host function: no GPU needed."""
    return bool(_capi.lib().stgcn_vit_patch_embed_backward_supported(N, C, T, V, p1, p2, E, _patch_flags(math, channels_last)))


def vit_patch_embed_backward_ws_bytes(N, C, T, V, p1, p2, E, math=MATH_F32, channels_last=False) -> int:
    return int(_capi.lib().stgcn_vit_patch_embed_backward_ws_bytes(N, C, T, V, p1, p2, E, _patch_flags(math, channels_last)))


def vit_patch_embed_backward_cut(N, C, T, V, p1, p2, E, math=MATH_F32, channels_last=False):
    """``(tokens per split, splits)`` of the weight gradient's reduction over the tokens, or None where the call is not covered."""
    c = _capi.lib().stgcn_vit_patch_embed_backward_cut(N, C, T, V, p1, p2, E, _patch_flags(math, channels_last))
    return (c >> 16, c & 0xFFFF) if c else None


def vit_patch_embed_backward(z, weight, dx, p1, p2, math=MATH_F32, need_dw=True, need_dbias=True, need_dcls=True, need_dpos=True,
                             need_dz=True) -> dict:
    """Backward of ``vit_patch_embed``: from z (N, C, T, V) - contiguous, or channels-last strided, read in place - the weight
    (E, p1 p2 C) and dx (N, n + 1, E), the gradient of the embedding's output, the dict of ``dW`` (E, K), ``dbias`` (E),
    ``dcls`` (E), ``dpos`` (n + 1, E) and ``dz`` (the shape and strides of z), each None where ``need_*`` is off.  The patches
    are read from z and the gradient is written into z's layout directly: no (N, n, K) tensor exists.  ``math``: f32 or bf16x3
    for ``dz`` (a block's flag word is accepted: ``_patch_flags``); ``dW`` is fp32 matrix cores always."""
    dev = z.device
    N, C, T, V = z.shape
    E, K = weight.shape
    if T % p1 or V % p2:
        raise ValueError(f"T = {T}, V = {V} are not whole patches of {p1} x {p2}")
    n = (T // p1) * (V // p2)
    if K != p1 * p2 * C or tuple(dx.shape) != (N, n + 1, E):
        raise ValueError(f"weight is {tuple(weight.shape)}, dx is {tuple(dx.shape)}; expected ({E}, {p1 * p2 * C}) and {(N, n + 1, E)}")
    channels_last = _is_channels_last(z)
    zin = z.permute(0, 2, 3, 1) if channels_last else z
    fl = _patch_flags(math, channels_last)
    nbytes = int(_capi.lib().stgcn_vit_patch_embed_backward_ws_bytes(N, C, T, V, p1, p2, E, fl))
    ws = _bytes(dev, nbytes)
    out = {"dW": torch.empty((E, K), device=dev, dtype=torch.float32) if need_dw else None,
           "dbias": torch.empty(E, device=dev, dtype=torch.float32) if need_dbias else None,
           "dcls": torch.empty(E, device=dev, dtype=torch.float32) if need_dcls else None,
           "dpos": torch.empty((n + 1, E), device=dev, dtype=torch.float32) if need_dpos else None, "dz": None}
    dzin = None
    if need_dz:
        if channels_last:     # the strides of z: (N, T, V, C) memory seen as (N, C, T, V)
            dzin = torch.empty((N, T, V, C), device=dev, dtype=torch.float32)
            out["dz"] = dzin.permute(0, 3, 1, 2)
        else:
            dzin = out["dz"] = torch.empty((N, C, T, V), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_patch_embed_backward", _dev_ptr(zin, "z", dev, align=ALIGN_LISTED),
                   _dev_ptr(weight, "weight", dev, align=ALIGN_LISTED), _dev_ptr(dx, "dx", dev, align=ALIGN_LISTED),
                   _dev_ptr(out["dW"], "dW"), _dev_ptr(out["dbias"], "dbias"), _dev_ptr(out["dcls"], "dcls"),
                   _dev_ptr(out["dpos"], "dpos"), _dev_ptr(dzin, "dz"), c_int(N), c_int(C), c_int(T), c_int(V), c_int(p1), c_int(p2),
                   c_int(E), c_void_p(ws.data_ptr()), c_size_t(nbytes), c_uint(fl), _stream(dev))
    return out


def vit_pool_classify_backward_supported(N, L, D, classes, mode="cls") -> bool:
    """Whether ``vit_pool_classify_backward`` runs this shape and pooling ('max' has no backward).  A host function."""
    return bool(_capi.lib().stgcn_vit_pool_classify_backward_supported(N, L, D, classes, _pool_flags(mode)))


def vit_pool_classify_backward(x, ln_weight, ln_bias, eps, weight, dlogits, mode="cls", need_dx=True, need_dln=True, need_dw=True,
                               need_dbias=True) -> dict:
    """Backward of ``vit_pool_classify`` ('cls' or 'mean'): the dict of ``dx`` (N, L, D), written whole (for 'cls' the rows
    below the class token are zeros), ``dln_weight``, ``dln_bias`` (D), ``dW`` (classes, D) and ``dbias`` (classes), each None
    where ``need_*`` is off (``need_dln`` may be a pair, weight then bias).  The pooled row and its LayerNorm statistics are
    recomputed from x.  fp32."""
    fl = _pool_flags(mode)
    dev = x.device
    N, L, D = x.shape
    classes = weight.shape[0]
    if weight.shape[1] != D or ln_weight.numel() != D or ln_bias.numel() != D or tuple(dlogits.shape) != (N, classes):
        raise ValueError(f"weight is {tuple(weight.shape)}, the LayerNorm has {ln_weight.numel()} features, x has {D}, dlogits is "
                         f"{tuple(dlogits.shape)}")
    need_dlw, need_dlb = need_dln if isinstance(need_dln, (tuple, list)) else (need_dln, need_dln)

    def new(shape, need):
        return torch.empty(shape, device=dev, dtype=torch.float32) if need else None
    out = {"dx": new((N, L, D), need_dx), "dln_weight": new((D,), need_dlw), "dln_bias": new((D,), need_dlb),
           "dW": new((classes, D), need_dw), "dbias": new((classes,), need_dbias)}
    nbytes = int(_capi.lib().stgcn_vit_pool_classify_backward_ws_bytes(N, L, D, classes, fl))
    ws = _bytes(dev, nbytes)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_pool_classify_backward", _dev_ptr(x, "x", dev, align=ALIGN_LISTED), _dev_ptr(ln_weight, "ln weight", dev),
                   _dev_ptr(ln_bias, "ln bias", dev), c_float(eps), _dev_ptr(weight, "weight", dev), _dev_ptr(dlogits, "dlogits", dev),
                   _dev_ptr(out["dx"], "dx"), _dev_ptr(out["dln_weight"], "dln_weight"), _dev_ptr(out["dln_bias"], "dln_bias"),
                   _dev_ptr(out["dW"], "dW"), _dev_ptr(out["dbias"], "dbias"), c_int(N), c_int(L), c_int(D), c_int(classes),
                   c_void_p(ws.data_ptr()), c_size_t(nbytes), c_uint(fl), _stream(dev))
    return out


def _head_shape(N, T, V, C, E1, E2, heads, hidden1, hidden2, depth1, depth2, classes):
    return _capi.AltformerHeadShape(N, T, V, C, E1, E2, heads, hidden1, hidden2, depth1, depth2, classes)


def _head_flags(order, channels_last=False) -> int:
    if order not in ("ST", "TS"):
        raise ValueError(f"order must be 'ST' or 'TS' (got {order!r})")
    return (_capi.EMBED_TS if order == "TS" else 0) | (_capi.IN_NTVC if channels_last else 0)


def altformer_head_supported(N, T, V, C, E1, E2, heads, hidden1, hidden2, depth1, depth2, classes, order="ST", math1=MATH_F32,
                             math2=MATH_F32) -> bool:
    """Whether ``altformer_head_forward`` runs this head (both stages' blocks under their flag words, and the glue).  A host
    function: no GPU needed."""
    shape = _head_shape(N, T, V, C, E1, E2, heads, hidden1, hidden2, depth1, depth2, classes)
    return bool(_capi.lib().stgcn_altformer_head_supported(shape, _vit_flags(math1), _vit_flags(math2), _head_flags(order)))


def _head_ws_bytes(shape, flags1, flags2, head_flags) -> int:
    return int(_capi.lib().stgcn_altformer_head_ws_bytes(shape, flags1, flags2, head_flags))


def _block_structs(blocks, dev):
    arr = (_capi.VitBlockWeights * len(blocks))()
    for dst, params in zip(arr, blocks):
        if len(params) != len(VIT_BLOCK_PARAMS):
            raise ValueError(f"a block has {len(params)} parameters, expected {len(VIT_BLOCK_PARAMS)}")
        for (field, _), name, t in zip(_capi.VitBlockWeights._fields_, VIT_BLOCK_PARAMS, params):
            setattr(dst, field, _dev_ptr(t, name, dev))
    return arr


def altformer_head_forward(z, embed1, pos1, blocks1, embed2, pos2, blocks2, head_norm, head_linear, heads, eps_blocks, eps_head,
                           scale1, scale2, order="ST", math1=MATH_F32, math2=MATH_F32, logits=None) -> torch.Tensor:
    """An AltFormer head from the stem output z (N, C, T, V) - contiguous, or channels-last strided as ``patch_embed`` takes it -
    to the logits (N, classes) in one library call (stgcn_altformer_head_forward): both embeddings, every block of both stages,
    the pooling between them and the pooled LayerNorm + classifier.

    ``embed1`` / ``embed2`` / ``head_linear`` = (weight, bias) of the nn.Linears, ``head_norm`` = (weight, bias) of the
    LayerNorm before the classifier (``eps_head``), ``pos1`` / ``pos2`` the position tables or None, ``blocks1`` / ``blocks2``
    one sequence of the twelve tensors in ``VIT_BLOCK_PARAMS`` order per block (a bias may be None), ``math1`` / ``math2`` the
    two stages' flag words as ``vit_block_forward`` takes them, ``order`` 'ST' (mean over joints, then max over frames) or 'TS'.
    The structs are built from these tensors on every call - nothing is packed or cached - and the workspace comes from
    torch's allocator, so the call captures under ``torch.cuda.graph``."""
    dev = z.device
    N, C, T, V = z.shape
    channels_last = _is_channels_last(z)
    if channels_last:
        z = z.permute(0, 2, 3, 1)
    E1, E2, classes = embed1[0].shape[0], embed2[0].shape[0], head_linear[0].shape[0]
    L1, L2 = (T, V) if order == "TS" else (V, T)
    if embed1[0].shape[1] != C or embed2[0].shape[1] != E1 or head_linear[0].shape[1] != E2 or head_norm[0].numel() != E2:
        raise ValueError("the embeddings, the LayerNorm and the classifier do not chain")
    for pos, want, name in ((pos1, L1 * E1, "pos1"), (pos2, L2 * E2, "pos2")):
        if pos is not None and pos.numel() != want:
            raise ValueError(f"{name} has {pos.numel()} elements, expected {want}")
    if not blocks1 or not blocks2:
        raise ValueError("each stage needs at least one block")
    shape = _head_shape(N, T, V, C, E1, E2, heads, blocks1[0][8].shape[0], blocks2[0][8].shape[0], len(blocks1), len(blocks2),
                        classes)
    fl1, fl2, hf = _vit_flags(math1), _vit_flags(math2), _head_flags(order, channels_last)
    b1, b2 = _block_structs(blocks1, dev), _block_structs(blocks2, dev)
    w = _capi.AltformerHeadWeights(
        _dev_ptr(embed1[0], "embed1.weight", dev), _dev_ptr(embed1[1], "embed1.bias", dev), _dev_ptr(pos1, "pos1", dev), b1,
        _dev_ptr(embed2[0], "embed2.weight", dev), _dev_ptr(embed2[1], "embed2.bias", dev), _dev_ptr(pos2, "pos2", dev), b2,
        _dev_ptr(head_norm[0], "head_norm.weight", dev), _dev_ptr(head_norm[1], "head_norm.bias", dev),
        _dev_ptr(head_linear[0], "head.weight", dev, align=ALIGN_LISTED), _dev_ptr(head_linear[1], "head.bias", dev))
    nbytes = _head_ws_bytes(shape, fl1, fl2, hf)
    ws = _bytes(dev, nbytes)
    if logits is None:
        logits = torch.empty((N, classes), device=dev, dtype=torch.float32)
    elif logits.shape != (N, classes):
        raise ValueError(f"logits is {tuple(logits.shape)}, expected {(N, classes)}")
    with torch.cuda.device(dev):
        _capi.call("stgcn_altformer_head_forward", _dev_ptr(z, "z", dev), w, shape, c_float(eps_blocks), c_float(eps_head),
                   c_float(scale1), c_float(scale2), c_void_p(ws.data_ptr()), c_size_t(nbytes), _dev_ptr(logits, "logits", dev),
                   c_uint(fl1), c_uint(fl2), c_uint(hf), _stream(dev))
    return logits


# ---- AltFormer heads: training (stgcn_vit_*_backward, stgcn_vit_block_forward_train) ------------------------------------------
def vit_linear_backward_supported(M, K, Nout, math=MATH_F32) -> bool:
    return bool(_capi.lib().stgcn_vit_linear_backward_supported(M, K, Nout, math & _capi.MATH_MASK))


def vit_linear_backward_bf16_supported(M, K, Nout) -> bool:
    """What ``vit_linear_backward`` covers with ``VIT_TRAIN_BF16``."""
    return bool(_capi.lib().stgcn_vit_linear_backward_bf16_supported(M, K, Nout))


def vit_linear_backward(dy, a, weight, h_pre=None, dx_accumulate=None, need_dx=True, need_dw=True, need_db=True,
                        math=MATH_F32):
    """Backward of ``y = a W^T + b`` on the last axis: returns ``(dx, dW, db)`` (None where not asked for).
    ``dx = dy W``, multiplied by ``GELU'(h_pre)`` when ``h_pre`` (shape of ``a``) is given - the dgrad of the linear behind
    a GELU whose input was ``h_pre`` - and added onto ``dx_accumulate`` (in place, returned) when that is given.
    ``math | VIT_TRAIN_BF16``: both products on operands rounded to nearest-even bf16 (``db`` sums the unrounded ``dy``).
    ``math | VIT_WGRAD_SMALL``: the weight gradient picks its form and cut by the call's size (``vit_wgrad_plan``)."""
    dev = dy.device
    Nout, K = weight.shape
    M = dy.numel() // Nout
    dx = None
    if need_dx:
        dx = dx_accumulate if dx_accumulate is not None else torch.empty(dy.shape[:-1] + (K,), device=dev, dtype=torch.float32)
    dW = torch.empty_like(weight) if need_dw else None
    db = torch.empty(Nout, device=dev, dtype=torch.float32) if need_dw and need_db else None
    if math & _capi.VIT_WGRAD_SMALL:     # its own cut of the tokens, its own size; without the bit the query every call has used
        nbytes = _capi.lib().stgcn_vit_linear_backward_small_ws_bytes(M, K, Nout, _capi.VIT_WGRAD_SMALL)
    else:
        nbytes = _capi.lib().stgcn_vit_linear_backward_ws_bytes(M, K, Nout)
    ws = _bytes(dev, nbytes)
    fl = (math & (_capi.MATH_MASK | _capi.VIT_TILE_MASK | _capi.VIT_TRAIN_BF16 | _capi.VIT_WGRAD_SMALL)) \
        | (_capi.VIT_DGELU if h_pre is not None and need_dx else 0) | (_capi.VIT_ACCUMULATE if dx_accumulate is not None else 0)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_linear_backward", _dev_ptr(dy, "dy", dev), _dev_ptr(a if need_dw else None, "a", dev),
                   _dev_ptr(weight, "weight", dev), _dev_ptr(h_pre if need_dx else None, "h_pre", dev), _dev_ptr(dx, "dx", dev),
                   _dev_ptr(dW, "dW"), _dev_ptr(db, "db"), c_void_p(ws.data_ptr()), c_size_t(nbytes), c_int(M), c_int(K),
                   c_int(Nout), c_uint(fl), _stream(dev))
    return dx, dW, db


def vit_attention_backward_supported(L, heads, head_dim) -> bool:
    """The resident backward's coverage (L <= 256)."""
    return bool(_capi.lib().stgcn_vit_attention_backward_supported(L, heads, head_dim))


def vit_attention_backward_stream_supported(L, heads, head_dim) -> bool:
    """The streaming backward's coverage (L <= 4096)."""
    return bool(_capi.lib().stgcn_vit_attention_backward_stream_supported(L, heads, head_dim))


def _vit_attention_backward(stream, qkv, out, dout, heads, scale):
    dev = qkv.device
    B, L, D3 = qkv.shape
    hd = D3 // 3 // heads
    if hd * heads * 3 != D3 or out.shape != (B, L, D3 // 3) or dout.shape != out.shape:
        raise ValueError(f"qkv {tuple(qkv.shape)}, out {tuple(out.shape)}, dout {tuple(dout.shape)} with {heads} heads")
    dqkv = torch.empty_like(qkv)
    ptrs = [_dev_ptr(qkv, "qkv", dev), _dev_ptr(out, "out", dev), _dev_ptr(dout, "dout", dev), _dev_ptr(dqkv, "dqkv")]
    dims = [c_int(B), c_int(L), c_int(heads), c_int(hd), c_float(hd ** -0.5 if scale is None else scale), _stream(dev)]
    with torch.cuda.device(dev):
        if stream == "bf16":
            _capi.call("stgcn_vit_attention_backward_bf16", *ptrs, *dims)
        elif stream:
            nbytes = _capi.lib().stgcn_vit_attention_backward_stream_ws_bytes(B, L, heads)
            ws = _bytes(dev, nbytes)
            _capi.call("stgcn_vit_attention_backward_stream", *ptrs, c_void_p(ws.data_ptr()), c_size_t(nbytes), *dims)
        else:
            _capi.call("stgcn_vit_attention_backward", *ptrs, *dims)
    return dqkv


def vit_attention_backward(qkv, out, dout, heads, scale=None) -> torch.Tensor:
    """Gradient of the packed qkv (B, L, 3*D) from the forward's output ``out`` and its gradient ``dout`` (B, L, D).
    Sequences of up to 256 tokens run the resident kernel, longer ones (up to 4096) the streaming kernels."""
    L, hd = qkv.shape[1], qkv.shape[2] // 3 // heads
    stream = not vit_attention_backward_supported(L, heads, hd) and vit_attention_backward_stream_supported(L, heads, hd)
    return _vit_attention_backward(stream, qkv, out, dout, heads, scale)


def vit_attention_backward_stream(qkv, out, dout, heads, scale=None) -> torch.Tensor:
    """``vit_attention_backward`` on the streaming kernels (a query kernel for the soft-max statistics and dq, a key kernel
    for dk and dv, their workspace allocated here) at every covered length, the short ones included: the same result up to
    the summation order."""
    return _vit_attention_backward(True, qkv, out, dout, heads, scale)


def vit_attention_backward_bf16(qkv, out, dout, heads, scale=None) -> torch.Tensor:
    """``vit_attention_backward`` in the arithmetic of ``VIT_TRAIN_ATTN_BF16`` (L <= 256): the scores recomputed as in
    ``vit_attention_train_bf16``, every other product on operands rounded to bf16, delta = sum P dP (``out`` is not read)."""
    return _vit_attention_backward("bf16", qkv, out, dout, heads, scale)


def vit_layernorm_backward(x, dn, weight, eps, dres=None):
    """LayerNorm backward over the last axis: ``(dx (+ dres), dweight, dbias)`` from ``dn``, the gradient of its output."""
    dev = x.device
    D = x.shape[-1]
    M = x.numel() // D
    dx = torch.empty_like(x)
    dw = torch.empty(D, device=dev, dtype=torch.float32)
    db = torch.empty(D, device=dev, dtype=torch.float32)
    nbytes = _capi.lib().stgcn_vit_layernorm_backward_ws_bytes(M, D)
    ws = _bytes(dev, nbytes)
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_layernorm_backward", _dev_ptr(x, "x", dev), _dev_ptr(dn, "dn", dev), _dev_ptr(weight, "weight", dev),
                   c_float(eps), _dev_ptr(dres, "dres", dev), _dev_ptr(dx, "dx"), _dev_ptr(dw, "dweight"), _dev_ptr(db, "dbias"),
                   c_void_p(ws.data_ptr()), c_size_t(nbytes), c_int(M), c_int(D), _stream(dev))
    return dx, dw, db


def vit_block_train_supported(L, D, heads, hidden) -> bool:
    """Coverage of the resident form of the training entry points (L <= 256)."""
    return bool(_capi.lib().stgcn_vit_block_train_supported(L, D, heads, hidden))


def vit_block_train_long_supported(L, D, heads, hidden) -> bool:
    """What ``vit_block_forward_train`` / ``vit_block_backward`` run: the resident coverage plus 256 < L <= 4096 on the
    streaming attention kernels."""
    return bool(_capi.lib().stgcn_vit_block_train_long_supported(L, D, heads, hidden))


def vit_block_train_bf16_supported(L, D, heads, hidden) -> bool:
    """What ``vit_block_forward_train`` / ``vit_block_backward`` cover with ``VIT_TRAIN_BF16``: both ranges of
    ``vit_block_train_long_supported``."""
    return bool(_capi.lib().stgcn_vit_block_train_bf16_supported(L, D, heads, hidden))


def vit_block_train_attn_bf16_supported(L, D, heads, hidden) -> bool:
    """Whether ``vit_block_forward_train`` / ``vit_block_backward`` with ``VIT_TRAIN_ATTN_BF16`` run the bf16 attention
    kernels: covered shapes with L <= 256 (longer sequences run the fp32 streaming kernels whatever the bit says)."""
    return bool(_capi.lib().stgcn_vit_block_train_attn_bf16_supported(L, D, heads, hidden))


def _vit_block_train_bytes(B, L, D, heads, hidden):
    """(saved bytes, workspace bytes) of the training entry points.  The resident form's queries where they answer (L <= 256),
    the ``_long`` queries, which cover both ranges and answer the same there, for what those leave at 0."""
    lib = _capi.lib()
    saved = lib.stgcn_vit_block_saved_bytes(B, L, D, hidden) or lib.stgcn_vit_block_train_long_saved_bytes(B, L, D, hidden)
    ws = lib.stgcn_vit_block_backward_ws_bytes(B, L, D, hidden) or lib.stgcn_vit_block_train_long_ws_bytes(B, L, D, heads, hidden)
    return saved, ws


VIT_BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "norm2.weight",
                    "norm2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def vit_block_train_drop_supported(L, D, heads, hidden) -> bool:
    """What ``vit_block_forward_train`` / ``vit_block_backward`` cover with ``drop``: ``vit_block_train_long_supported``."""
    return bool(_capi.lib().stgcn_vit_block_train_drop_supported(L, D, heads, hidden))


def _drop_struct(drop, x, hidden):
    """``drop`` = (m_proj, m_act, m_fc2), each None or contiguous fp32 of (B, L, D) / (B, L, hidden) / (B, L, D), as the C struct."""
    if len(drop) != 3:
        raise ValueError("drop is (m_proj, m_act, m_fc2)")
    B, L, D = x.shape
    masks = _capi.VitDropMasks()
    for (field, _), m, width in zip(_capi.VitDropMasks._fields_, drop, (D, hidden, D)):
        if m is not None and (tuple(m.shape) != (B, L, width) or not m.is_contiguous()):
            raise ValueError(f"{field}: expected a contiguous ({B}, {L}, {width}) tensor, got {tuple(m.shape)}")
        setattr(masks, field, _dev_ptr(m, field, x.device, align=0 if field == "m_act" else ALIGN_LISTED))
    return masks


def vit_block_forward_train(x, params, heads, eps, scale, math=MATH_F32, scale1=None, scale2=None, drop=None):
    """Training forward of one Block on x (B, L, D): returns ``(y, saved)``.  ``params``: the twelve tensors in the order of
    ``VIT_BLOCK_PARAMS`` (qkv.bias may be None).  ``scale1`` / ``scale2`` (B,): stochastic depth's per-sequence factors of the
    attention and the MLP branch (None = 1).  ``saved`` is an opaque buffer for ``vit_block_backward``.
    ``math``: MATH_F32 or MATH_BF16X3, optionally | VIT_QKV_F32, optionally | VIT_TRAIN_BF16 (every linear product but the qkv
    forward on operands rounded to bf16), optionally | VIT_TRAIN_ATTN_BF16 (the attention forward and backward on bf16 operands
    where L <= 256).  Hand the same value to ``vit_block_backward``.
    ``drop`` = (m_proj, m_act, m_fc2): per-element dropout factors (0 or 1 / (1 - p), fp32, None = 1) behind the projection
    (B, L, D), behind the GELU (B, L, hidden) and behind the second MLP linear (B, L, D).  With ``drop`` (a tuple, even of three
    Nones) the call is ``stgcn_vit_block_forward_train_drop``, which also takes a VIT_TILE_* field in ``math`` (the tile form of
    its linears; same result bit for bit); without, the older entry point, which refuses one."""
    dev = x.device
    B, L, D = x.shape
    hidden = params[8].shape[0]
    nbytes, _ = _vit_block_train_bytes(B, L, D, heads, hidden)
    saved = _bytes(dev, nbytes)
    y = torch.empty_like(x)
    if drop is not None:
        masks, weights = _drop_struct(drop, x, hidden), _block_structs([params], dev)
        with torch.cuda.device(dev):
            _capi.call("stgcn_vit_block_forward_train_drop", _dev_ptr(x, "x", dev), weights, _dev_ptr(scale1, "scale1", dev),
                       _dev_ptr(scale2, "scale2", dev), ctypes.byref(masks), c_float(eps), c_float(scale),
                       c_void_p(saved.data_ptr()), c_size_t(nbytes), _dev_ptr(y, "y"), c_int(B), c_int(L), c_int(D), c_int(heads),
                       c_int(hidden), c_uint(_vit_train_flags(math, small=True)), _stream(dev))
        return y, saved
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_block_forward_train", _dev_ptr(x, "x", dev),
                   *[_dev_ptr(p, n, dev) for n, p in zip(VIT_BLOCK_PARAMS, params)],
                   _dev_ptr(scale1, "scale1", dev), _dev_ptr(scale2, "scale2", dev), c_float(eps), c_float(scale),
                   c_void_p(saved.data_ptr()), c_size_t(nbytes), _dev_ptr(y, "y"), c_int(B), c_int(L), c_int(D), c_int(heads),
                   c_int(hidden), c_uint(_vit_train_flags(math)), _stream(dev))
    return y, saved


def vit_block_backward(x, params, saved, dy, heads, eps, scale, math=MATH_F32, scale1=None, scale2=None, drop=None) -> dict:
    """Backward of ``vit_block_forward_train`` (same arguments, ``drop`` included): ``{"x": dx, "norm1.weight": ..., ...}`` with a
    gradient for ``x`` and for every entry of ``VIT_BLOCK_PARAMS`` (``qkv.bias``: None when the block has none)."""
    dev = x.device
    B, L, D = x.shape
    hidden = params[8].shape[0]
    sbytes, nbytes = _vit_block_train_bytes(B, L, D, heads, hidden)
    if saved.numel() * saved.element_size() < sbytes:
        raise ValueError("saved does not come from vit_block_forward_train of these shapes")
    if drop is not None:
        if math & _capi.VIT_WGRAD_SMALL:
            nbytes = _capi.lib().stgcn_vit_block_train_small_ws_bytes(B, L, D, heads, hidden, _capi.VIT_WGRAD_SMALL)
        else:
            nbytes = _capi.lib().stgcn_vit_block_train_drop_ws_bytes(B, L, D, heads, hidden)
    ws = _bytes(dev, nbytes)
    grads = {"x": torch.empty_like(x)}
    for n, p in zip(VIT_BLOCK_PARAMS, params):
        grads[n] = None if p is None else torch.empty_like(p)
    if drop is not None:
        masks, weights = _drop_struct(drop, x, hidden), _block_structs([params], dev)
        gs = _capi.VitBlockGrads()
        for (field, _), n in zip(_capi.VitBlockGrads._fields_, VIT_BLOCK_PARAMS):
            setattr(gs, field, _dev_ptr(grads[n], "d" + n))
        with torch.cuda.device(dev):
            _capi.call("stgcn_vit_block_backward_drop", _dev_ptr(x, "x", dev), weights, _dev_ptr(scale1, "scale1", dev),
                       _dev_ptr(scale2, "scale2", dev), ctypes.byref(masks), c_void_p(saved.data_ptr()), c_size_t(sbytes),
                       _dev_ptr(dy, "dy", dev, align=ALIGN_LISTED if drop[0] is not None or drop[2] is not None else 0),
                       _dev_ptr(grads["x"], "dx"), ctypes.byref(gs), c_float(eps), c_float(scale),
                       c_void_p(ws.data_ptr()), c_size_t(nbytes), c_int(B), c_int(L), c_int(D), c_int(heads), c_int(hidden),
                       c_uint(_vit_train_flags(math, small=True)), _stream(dev))
        return grads
    w = dict(zip(VIT_BLOCK_PARAMS, params))
    with torch.cuda.device(dev):
        _capi.call("stgcn_vit_block_backward", _dev_ptr(x, "x", dev),
                   *[_dev_ptr(w[n], n, dev) for n in ("norm1.weight", "norm1.bias", "qkv.weight", "proj.weight", "norm2.weight",
                                                      "norm2.bias", "fc1.weight", "fc2.weight")],
                   _dev_ptr(scale1, "scale1", dev), _dev_ptr(scale2, "scale2", dev), c_void_p(saved.data_ptr()), c_size_t(sbytes),
                   _dev_ptr(dy, "dy", dev), _dev_ptr(grads["x"], "dx"), *[_dev_ptr(grads[n], "d" + n) for n in VIT_BLOCK_PARAMS],
                   c_float(eps), c_float(scale), c_void_p(ws.data_ptr()), c_size_t(nbytes), c_int(B), c_int(L), c_int(D),
                   c_int(heads), c_int(hidden), c_uint(_vit_train_flags(math)), _stream(dev))
    return grads
