"""nn.Module mirror of ST-TR's spatial self-attention unit, running on libstgcn_hip.so.

``gcn_unit_attention`` <- model/ST_TR/gcn_attention.py:25-156 and its ``attention_conv``, ``spatial_attention`` <-
model/ST_TR/spatial_transformer.py:17-80 of the reference: same constructor arguments, sub-module / parameter names (so
``.pth`` files load strictly), construction order (a seeded construction gives the reference's initial weights) and RNG use.

Only the configuration the reference's scripts build is implemented (only_attention, data_normalization, skip_conn,
bn_flag, kernel_size = stride = 1, with or without drop_connect); every other option value raises NotImplementedError at
construction.  There is no torch-op implementation of the math in this package.

Drop-connect draws ONE ``torch.bernoulli`` of N*T*Nh*V elements per training forward, as the reference does
(spatial_transformer.py:131-135), so the torch generator advances exactly as under the reference and the Dropout layers
after this unit draw the same numbers.  The reference draws on the default ``cuda`` device; this module draws on x's device
(the same device on one GPU; under nn.DataParallel each replica draws on its own device's generator).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import functional as F
from ._capi import MATH_BF16X3, MATH_F32
from .modules import _check_input, _master, _slot, _versions, _wants_grad

# arithmetic of the unit's two 1x1 projections and of their two input gradients (everything else is fp32 either way)
ST_ATTENTION_MATH = {"f32": MATH_F32, "bf16x3": MATH_BF16X3}
DEFAULT_ST_ATTENTION_MATH = "f32"


def _math_name(mode) -> str:
    if not isinstance(mode, str) or mode.lower() not in ST_ATTENTION_MATH:
        raise ValueError(f"gcn_unit_attention arithmetic {mode!r}: expected 'f32' or 'bf16x3'")
    return mode.lower()


def _default_math() -> str:
    return _math_name(os.environ.get("STGCN_ST_ATTENTION_MATH", DEFAULT_ST_ATTENTION_MATH))


def set_st_attention_math(module: nn.Module, mode) -> None:
    """Arithmetic of the two 1x1 projections (and, in training, of their two input gradients) of every
    ``gcn_unit_attention`` below: 'f32' (the fp32 matrix cores, the default) | 'bf16x3' (both operands split into bf16
    hi + lo, three bf16 matrix-core products, fp32 sums; opt-in, holds the fp32 gate of 1e-4).  Anything else raises
    ValueError.  The weight gradients, the V x V attention and the BatchNorms stay fp32.  Env ``STGCN_ST_ATTENTION_MATH``
    sets the default of newly built units.  Nothing but these units is touched."""
    name = _math_name(mode)
    for sub in module.modules():
        if isinstance(sub, gcn_unit_attention):
            sub.math_mode = name


class spatial_attention(nn.Module):
    """The ``attention_conv`` sub-module: holds ``qkv_conv`` and ``attn_out`` and the attention's settings.  Its math runs
    inside gcn_unit_attention's HIP kernels; it is not callable on its own."""

    def __init__(self, in_channels, kernel_size, dk, dv, Nh, complete, relative, layer, A, more_channels, drop_connect,
                 adjacency, num, num_point, shape=25, stride=1, last_graph=False, data_normalization=True, skip_conn=True,
                 visualization=True):
        super().__init__()
        for name, val in (("relative", relative), ("adjacency", adjacency), ("more_channels", more_channels)):
            if val:
                raise NotImplementedError(f"spatial_attention: {name}=True is not implemented by the HIP unit "
                                          "(no reference script builds it)")
        if stride != 1:
            raise NotImplementedError(f"spatial_attention: stride={stride} is not implemented by the HIP unit (only 1)")
        self.in_channels = in_channels
        self.complete = complete
        self.kernel_size = 1
        self.dk = dk
        self.dv = dv
        self.num = num
        self.layer = layer
        self.more_channels = more_channels
        self.drop_connect = drop_connect
        self.visualization = visualization
        self.data_normalization = data_normalization
        self.skip_conn = skip_conn
        self.adjacency = adjacency
        self.Nh = Nh
        self.num_point = num_point
        self.A = A[0] + A[1] + A[2]            # plain attribute, as in the reference (not a buffer, not in state_dict)
        self.shape = shape
        self.relative = relative
        self.last_graph = last_graph
        self.stride = stride
        self.padding = (self.kernel_size - 1) // 2
        assert self.Nh != 0, "integer division or modulo by zero, Nh >= 1"
        assert self.dk % self.Nh == 0, "dk should be divided by Nh. (example: out_channels: 20, dk: 40, Nh: 4)"
        assert self.dv % self.Nh == 0, "dv should be divided by Nh. (example: out_channels: 20, dv: 4, Nh: 4)"
        self.qkv_conv = nn.Conv2d(self.in_channels, 2 * self.dk + self.dv, kernel_size=self.kernel_size, stride=stride,
                                  padding=self.padding)
        self.attn_out = nn.Conv2d(self.dv, self.dv, kernel_size=1, stride=1)

    def forward(self, x):
        raise RuntimeError("spatial_attention runs inside gcn_unit_attention's HIP kernels; call the gcn_unit_attention")


class _StAttentionTrainFn(torch.autograd.Function):
    """gcn_unit_attention.forward with the HIP forward and backward: batch statistics in .train(), running statistics
    (``frozen``: constants of the backward) in .eval() under autograd."""

    @staticmethod
    def forward(ctx, mod, x, mask, *params):         # `params` = mod._weights(): graph edges only, values via _staged
        st = mod._staged(x.device)
        dbn, bn = mod.data_bn, mod.bn
        frozen = not mod._bn_training()
        xd = x.detach()
        y, sv = F.st_attention_forward_train(
            xd, (dbn.weight.detach(), dbn.bias.detach(), dbn.running_mean, dbn.running_var), st["Wqkv"], st["bqkv"],
            st["Wout"], st["bout"], (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var), mask,
            mod._dk, mod._heads, mod._momentum(), bn.eps, frozen=frozen, math=mod._math_flags)
        ctx.save_for_backward(xd, dbn.weight.detach(), dbn.bias.detach(), st["Wqkv"], st["Wout"], bn.weight.detach(),
                              bn.bias.detach(), mask, sv["qkv"], sv["o"], sv["z"], sv["rowstats"], sv["stats"])
        ctx.meta = (mod._dk, mod._heads, frozen, tuple(params[2].shape), tuple(params[4].shape), mod._math_flags)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, dbw, dbb, Wqkv, Wout, bw, bb, mask, qkv, o, z, rowstats, stats = ctx.saved_tensors
        dk, heads, frozen, qshape, oshape, math = ctx.meta
        saved = {"qkv": qkv, "o": o, "z": z, "rowstats": rowstats, "stats": stats}
        g = F.st_attention_backward(x, dbw, dbb, Wqkv, Wout, bw, bb, mask, saved, dy.contiguous(), dk, heads,
                                    need_dx=ctx.needs_input_grad[1], frozen=frozen, math=math)
        return (None, g["dx"], None, g["ddbn_weight"], g["ddbn_bias"], g["dWqkv"].view(qshape), g["dbqkv"],
                g["dWout"].view(oshape), g["dbout"], g["dbn_weight"], g["dbn_bias"])


class gcn_unit_attention(nn.Module):
    """Spatial self-attention unit of ST-TR; signature, attributes and state_dict of model/ST_TR/gcn_attention.py:25-93.

    State: ``data_bn.*`` (BatchNorm1d over in_channels*num_point), ``bn.*`` (BatchNorm2d(out_channels)),
    ``attention_conv.qkv_conv.{weight,bias}`` and ``attention_conv.attn_out.{weight,bias}``; ``incidence`` is a plain
    attribute as in the reference.  Covered by the kernels: out_channels in {128, 256, 512} with the reference's
    dk_factor = 0.25 and Nh = 8 (any per-head split with (dk/Nh, dv/Nh) in {(4,16), (8,32), (16,64)}), any in_channels,
    num_point <= 64; other shapes raise StgcnError (STGCN_ERR_UNSUPPORTED) at the first forward.  Batch statistics of a
    single frame (N*T == 1) raise ValueError, as the reference's data_bn does.

    ``math_mode`` ('f32' default | 'bf16x3'; ``set_st_attention_math``, env ``STGCN_ST_ATTENTION_MATH`` for new units) is
    the arithmetic of the two projections and their input gradients; an nn.DataParallel replica reads its master's.
    """

    def __init__(self, in_channels, out_channels, incidence, num, dv_factor, dk_factor, Nh, complete, relative,
                 only_attention, layer, more_channels, drop_connect, data_normalization, skip_conn, adjacency, num_point,
                 padding=0, kernel_size=1, stride=1, bn_flag=True, t_dilation=1, last_graph=False, visualization=True):
        super().__init__()
        refused = [("only_attention", not only_attention, "False"), ("relative", relative, "True"),
                   ("adjacency", adjacency, "True"), ("more_channels", more_channels, "True"),
                   ("data_normalization", not data_normalization, "False"), ("skip_conn", not skip_conn, "False"),
                   ("bn_flag", not bn_flag, "False"), ("kernel_size", kernel_size != 1, str(kernel_size)),
                   ("stride", stride != 1, str(stride))]
        for name, bad, val in refused:
            if bad:
                raise NotImplementedError(f"gcn_unit_attention: {name}={val} is not implemented by the HIP unit (the "
                                          "reference's scripts build only_attention=True, relative=False, adjacency=False, "
                                          "more_channels=False, data_normalization=True, skip_conn=True, bn_flag=True, "
                                          "kernel_size=1, stride=1)")
        self._math_mode = _default_math()
        self.incidence = incidence
        self.relu = nn.ReLU()
        self.visualization = visualization
        self.in_channels = in_channels
        self.more_channels = more_channels
        self.drop_connect = drop_connect
        self.data_normalization = data_normalization
        self.skip_conn = skip_conn
        self.num_point = num_point
        self.adjacency = adjacency
        self.last_graph = last_graph
        self.out_channels = out_channels
        self.data_bn = nn.BatchNorm1d(self.in_channels * self.num_point)
        self.bn = nn.BatchNorm2d(out_channels)
        self.only_attention = only_attention
        self.bn_flag = bn_flag
        self.layer = layer
        self.incidence = incidence.detach().clone().view(-1, incidence.size()[-1], incidence.size()[-1])
        self.attention_conv = spatial_attention(in_channels=self.in_channels, kernel_size=1,
                                                dk=int(out_channels * dk_factor), dv=int(out_channels), Nh=Nh,
                                                complete=complete, relative=relative, stride=stride,
                                                last_graph=self.last_graph, layer=self.layer, A=self.incidence, num=num,
                                                more_channels=self.more_channels, drop_connect=self.drop_connect,
                                                data_normalization=self.data_normalization, skip_conn=self.skip_conn,
                                                adjacency=self.adjacency, visualization=self.visualization,
                                                num_point=self.num_point)

    @property
    def _dk(self):
        return self.attention_conv.dk

    @property
    def _heads(self):
        return self.attention_conv.Nh

    @property
    def math_mode(self) -> str:
        """'f32' | 'bf16x3'; a replica answers for its master (a unit pickled before the setting existed: 'f32')."""
        return _master(self).__dict__.get("_math_mode", DEFAULT_ST_ATTENTION_MATH)

    @math_mode.setter
    def math_mode(self, mode):
        object.__setattr__(_master(self), "_math_mode", _math_name(mode))

    @property
    def _math_flags(self) -> int:
        return ST_ATTENTION_MATH[self.math_mode]

    def _replicate_for_data_parallel(self):
        replica = super()._replicate_for_data_parallel()
        object.__setattr__(replica, "_dp_master", _master(self))     # (not a sub-module: no Module.__setattr__)
        return replica

    def _weights(self):
        """The parameters by attribute (an nn.DataParallel replica has no ``parameters()``), in the order
        _StAttentionTrainFn.backward returns their gradients."""
        a = self.attention_conv
        yield self.data_bn.weight
        yield self.data_bn.bias
        yield a.qkv_conv.weight
        yield a.qkv_conv.bias
        yield a.attn_out.weight
        yield a.attn_out.bias
        yield self.bn.weight
        yield self.bn.bias

    def _cache_key(self, device):
        return (device, _versions(_master(self)))

    def _staged(self, device):
        """Projection weights as (rows, columns) device tensors, cached per device on the master module until any
        parameter or buffer changes; the folded running-statistics BatchNorms are added on first eval use."""
        key = self._cache_key(device)
        slot = _slot(self, device)
        with slot.lock:
            st = slot.get("st")
            if st is None or st["key"] != key:
                a = self.attention_conv
                with torch.no_grad():
                    on = lambda t: t.to(device=device, dtype=torch.float32).contiguous()   # noqa: E731
                    st = slot["st"] = {
                        "key": key,
                        "Wqkv": on(a.qkv_conv.weight.reshape(a.qkv_conv.out_channels, a.qkv_conv.in_channels)),
                        "bqkv": on(a.qkv_conv.bias), "Wout": on(a.attn_out.weight.reshape(a.dv, a.dv)),
                        "bout": on(a.attn_out.bias), "folded": None}
            return st

    def _folded(self, st):
        with _slot(self, st["key"][0]).lock, torch.no_grad():
            if st["folded"] is None:
                d, b = self.data_bn, self.bn
                st["folded"] = F.bn_fold(d.weight, d.bias, d.running_mean, d.running_var, None, d.eps) + \
                    F.bn_fold(b.weight, b.bias, b.running_mean, b.running_var, None, b.eps)
        return st["folded"]

    def _bn_training(self) -> bool:
        """Batch or running statistics, decided by the two BatchNorm sub-modules as in the reference; mixed modes are
        refused."""
        if self.data_bn.training != self.bn.training:
            raise NotImplementedError("gcn_unit_attention: data_bn and bn are in different modes (one .train(), one "
                                      ".eval()); the HIP path normalises both with the same kind of statistics")
        return self.bn.training

    def _momentum(self) -> float:
        d, b = self.data_bn, self.bn
        if d.momentum != b.momentum or d.eps != b.eps:
            raise NotImplementedError("gcn_unit_attention: data_bn and bn need the same momentum and eps on the HIP path")
        return b.momentum

    def _drop_mask(self, x):
        """The reference's drop-connect draw (spatial_transformer.py:131-132): one bernoulli per (frame, head, key)."""
        a = self.attention_conv
        if not (a.drop_connect and a.training):
            return None
        N, _, T, V = x.shape
        return torch.bernoulli(0.5 * torch.ones(N * T * a.Nh * V, device=x.device))

    def forward(self, x):
        bn_training = self._bn_training()
        _check_input(self, x, backward_ok=True, bn_training=bn_training)
        N, C, T, V = x.shape
        if C != self.in_channels:
            raise RuntimeError(f"gcn_unit_attention: expected {self.in_channels} input channels, got {C}")
        if V != self.num_point:
            raise RuntimeError(f"gcn_unit_attention: input has {V} joints, the unit was built for {self.num_point}")
        if bn_training and N * T == 1:
            # the reference's data_bn (BatchNorm1d over the (N, C*V, T) view) refuses one value per channel; the batch
            # variance would be 0.  Raised before the drop-connect draw and before any buffer is touched.
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[N, C * V, T]}")
        x = x.contiguous()
        st = self._staged(x.device)
        mask = self._drop_mask(x)
        wants = _wants_grad(self, x)
        if bn_training or wants or mask is not None:
            bn, dbn = self.bn, self.data_bn
            if bn_training and (bn.momentum is None or not bn.track_running_stats or not dbn.track_running_stats):
                raise NotImplementedError("gcn_unit_attention: training-mode BatchNorm needs momentum and running statistics")
            if not bn_training and not (bn.track_running_stats and dbn.track_running_stats):
                raise NotImplementedError("gcn_unit_attention: eval-mode BatchNorm without running statistics is not covered")
            if wants:
                y = _StAttentionTrainFn.apply(self, x, mask, *self._weights())
            else:
                y, _ = F.st_attention_forward_train(
                    x, (dbn.weight, dbn.bias, dbn.running_mean, dbn.running_var), st["Wqkv"], st["bqkv"], st["Wout"],
                    st["bout"], (bn.weight, bn.bias, bn.running_mean, bn.running_var), mask, self._dk, self._heads,
                    self._momentum(), bn.eps, frozen=not bn_training, math=self._math_flags)
            if bn_training:
                with torch.no_grad():
                    torch._foreach_add_([dbn.num_batches_tracked, bn.num_batches_tracked], 1)
            return y
        dscale, dshift, bscale, bshift = self._folded(st)
        return F.st_attention_forward(x, dscale, dshift, st["Wqkv"], st["bqkv"], st["Wout"], st["bout"], bscale, bshift,
                                      self._dk, self._heads, math=self._math_flags)
