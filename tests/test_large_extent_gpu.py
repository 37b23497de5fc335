"""GPU tests of the HIP entry points on extents no other test reaches (tests/large_extent.py has the method and the tables).

Table A: results of more than 2^31 elements - past 2^31 bytes, 2^32 bytes and 2^31 elements of one tensor, where a hand-written
offset of the wrong width wraps.  Table B: the clip limit - 65535 clips (kMaxGridClips: the clip index rides in a 16-bit grid
axis) on the smallest clips, 65536 refused with STGCN_ERR_UNSUPPORTED before anything is launched, and past it where an entry point
puts its sequences on grid.x (the heads) or documents that it takes more (the training forward of the temporal conv).

Every result is compared whole, on the device, with the fp64 reference of a 7-clip batch that the large batch repeats
(large_extent.gate_tiled), at the tolerance of the entry point's own test.  Results come from poisoned (NaN), guard-banded
``torch.empty`` (tests/_util.py::hostile_allocations): an element that is never written fails the gate.  A case is skipped only if
the device has less free memory than it needs (at most 48 GiB) plus 2 GiB; every case gives its memory back.

Reductions over the whole batch (parameter gradients, batch statistics) sum ~1.7e7 terms per channel; their rows name the bound
they hold and where it comes from."""
import functools

import pytest
import torch

import altformer_ref as ar
import altformer_train_ref as tr
import entry_points as ep
import large_extent as le
from _util import MATH_GATES, hostile_allocations
from entry_points import STEM_KERNELS, TCN_KERNELS, _stem_kernel, _tcn_mode, hipF as _F, math_flag as _math
from large_extent import GIB, Extent, gate_small, gate_tiled

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
BF16_OUT_GATE = 4e-3          # test_large_tile_temporal_conv_kernel: half an ulp of the stored bf16 value, max-norm criterion
NAN_FILL = 0xFF
UNSUPPORTED = -2              # STGCN_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


class Row:
    """``run(ext, dev)`` calls the entry point under the NaN-filling allocator and gates every result; ``tensors(ext)``: the bytes
    its inputs, results and workspaces hold at the peak (large_extent.need_bytes adds the gate's)."""

    def __init__(self, id, ext, run, tensors):
        self.id, self.ext, self.run, self.tensors = id, ext, run, int(tensors)


TABLE_A, TABLE_B = [], []
_A = le.table_a()


def poisoned():
    return hostile_allocations(NAN_FILL)


def sync_and_check(h):
    torch.cuda.synchronize()
    h.check()
    assert h.records, "no allocation went through torch.empty - the case would test nothing"


# ---- the fused stem ---------------------------------------------------------------------------------------------------------------
def run_stem(math, C, T, V, in_layout, out_layout, bf16, ext, dev):
    s = ep.stem(ext.n0, T, V, C)
    xt, ref = le.tiled(s, ext.R, dev, ext.N)
    staged = s.on(dev)
    mode = _math(math)
    prep = staged.prepare(mode)
    with poisoned() as h:
        out, P = staged.forward(xt, prep, mode, in_layout, out_layout, bf16)
        sync_and_check(h)
    assert out.shape == (ext.N, C, T, V) and out.dtype == ext.dtype and out.numel() == ext.result
    rel, strict = (max(MATH_GATES[math][0], BF16_OUT_GATE), False) if bf16 else MATH_GATES[math]
    print(ext.N, "clips: out", gate_tiled(out, ref["out"], rel, strict, "out"), "P", gate_tiled(P, ref["P"], 1e-4, True, "P"))


def stem_bytes(ext, C, T, V):
    x = ext.N * 3 * T * V * 4
    return ext.bytes() + 3 * x + ext.N * 3 * V * V * 4 + 2 * GIB       # x, its channels-last copy and the workspace's, P, fragments


for _r in le.A_STEM:
    TABLE_A.append(Row(le.stem_id(_r), _A[le.stem_id(_r)], functools.partial(run_stem, *_r[:7]), stem_bytes(_A[le.stem_id(_r)], *_r[1:4])))


def test_stem_rows_reach_every_kernel():
    F = _F()
    for math, C, T, V, _, _, _, kernel in le.A_STEM:
        assert F.stem_supported(3, C, T, V, 9, 3, _math(math)) and _stem_kernel((1, T, V, C), math) == kernel, (math, C, T, V)
    assert {r[7] for r in le.A_STEM} == STEM_KERNELS


# ---- the graph conv ---------------------------------------------------------------------------------------------------------------
def run_agcn(cin, cout, T, V, ext, dev):
    s = ep.agcn(ext.n0, cin, cout, T, V)
    xt, ref = le.tiled(s, ext.R, dev, ext.N)
    run = s.on(dev)
    with poisoned() as h:
        o = run(xt)
        sync_and_check(h)
    assert o["y"].numel() == ext.result
    print(ext.N, "clips:", {k: gate_tiled(o[k], ref[k], 1e-4, True, k) for k in ("y", "P", "P_attention")})


_id = "agcn_forward-" + "x".join(map(str, le.A_AGCN))
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_agcn, *le.A_AGCN), _A[_id].bytes() + GIB))


# ---- the temporal conv ------------------------------------------------------------------------------------------------------------
def run_tcn(cin, cout, K, stride, T, V, math, out_bf16, along_v, ext, dev):
    s = ep.tcn(cin, cout, K, stride, T, V, ext.n0, math, out_bf16, along_v)
    xt, ref = le.tiled(s, ext.R, dev, ext.N)
    run = s.on(dev)
    with poisoned() as h:
        o = run(xt)                                # tcn_forward_packed and, along the frames, the one-shot tcn_forward
        sync_and_check(h)
    rel, strict = (BF16_OUT_GATE, False) if out_bf16 else MATH_GATES[math]
    for k, y in o.items():
        assert y.numel() == ext.result and y.dtype == ext.dtype
        print(ext.N, "clips:", k, gate_tiled(y, ref[k], rel, strict, k))


def tcn_bytes(ext, cin, T, V, along_v):
    return ext.N * cin * T * V * 4 + (1 if along_v else 2) * ext.bytes()


for _r in le.A_TCN:
    TABLE_A.append(Row(le.tcn_id(_r), _A[le.tcn_id(_r)], functools.partial(run_tcn, *_r[:9]),
                       tcn_bytes(_A[le.tcn_id(_r)], _r[0], _r[4], _r[5], _r[8])))


def test_tcn_rows_reach_every_kernel():
    for cin, cout, K, stride, T, V, math, _, along_v, kernel in le.A_TCN:
        assert _tcn_mode(cin, cout, K, stride, T, V, math, along_v)[1] == kernel, (cin, cout, K, stride, T, V, math)
    assert {r[9] for r in le.A_TCN} == TCN_KERNELS


# ---- the heads: linear, attention, block ------------------------------------------------------------------------------------------
def run_vit_linear(math, epilogue, residual, ext, dev, K=le.LINEAR_K, Nout=le.LINEAR_NOUT, group=le.LINEAR_GROUP):
    """y (M, Nout) of M = N * group rows; the reference is that of the setup's n0 * group rows."""
    F = _F()
    M0 = ext.n0 * group
    s = ep.vit_linear(M0, K, Nout, "f32" if math == "bf16" else math)
    x64, W64, b64, R64 = (t.double() for t in (s.x, s.W, s.b, s.R))
    a = ar.layer_norm64(x64, s.ln[0].double(), s.ln[1].double()) if epilogue else x64
    want = a @ W64.T
    if epilogue:
        want = torch.nn.functional.gelu(want + b64)
    if residual:
        want = want + R64
    M = ext.N * group
    xt = s.x.to(dev).repeat(ext.R, 1)[:M].contiguous()
    Rt = s.R.to(dev).repeat(ext.R, 1)[:M].contiguous() if residual else None
    Wd, bd = s.W.to(dev), s.b.to(dev)
    kw = dict(ln=(s.ln[0].to(dev), s.ln[1].to(dev), ar.EPS), gelu=True) if epilogue else {}
    with poisoned() as h:
        if math == "bf16":
            y = F.vit_linear_bf16(xt, Wd, bd if epilogue else None, residual=Rt, **kw)
        else:
            assert F.vit_linear_supported(M, K, Nout, _math(math))
            y = F.vit_linear(xt, Wd, bd if epilogue else None, residual=Rt, math=_math(math), **kw)
        sync_and_check(h)
    assert y.shape == (M, Nout) and y.numel() == ext.result
    rel, strict = MATH_GATES[math]
    print(M, "rows:", gate_tiled(y.view(ext.N, group, Nout), want.view(ext.n0, group, Nout), rel, strict, "y"))


for _math_name, _epi, _res in le.A_LINEAR:
    _id = f"vit_linear-{_math_name}" + ("-ln_gelu" if _epi else "") + ("-residual" if _res else "")
    TABLE_A.append(Row(_id, _A[_id], functools.partial(run_vit_linear, _math_name, _epi, _res),
                       _A[_id].bytes() * (2 if _res else 1) + GIB))


def run_vit_attention(form, L, hd, ext, dev):
    s = ep.vit_attention(form, ext.n0, L, hd)
    qt, ref = le.tiled(s, ext.R, dev, ext.N)
    run = s.on(dev)
    with poisoned() as h:
        o = run(qt)
        sync_and_check(h)
    assert o["out"].numel() == ext.result
    print(ext.N, "sequences:", gate_tiled(o["out"], ref["out"], REL, True, "out"))


for _form, _L, _hd in le.A_ATTENTION:
    _id = f"vit_attention-{_form}-L{_L}-hd{_hd}"
    TABLE_A.append(Row(_id, _A[_id], functools.partial(run_vit_attention, _form, _L, _hd), 4 * _A[_id].bytes() + 2 * GIB))


def run_vit_block(L, D, heads, hidden, ext, dev):
    assert _F().vit_block_forward_supported(L, D, heads, hidden)
    s = ep.vit_block(ext.n0, L, D, heads, hidden, "f32")
    xt, ref = le.tiled(s, ext.R, dev, ext.N)
    run = s.on(dev)
    with poisoned() as h:
        o = run(xt)
        sync_and_check(h)
    assert o["y"].numel() == ext.result
    print(ext.N, "sequences:", gate_tiled(o["y"], ref["y"], REL, True, "y"))


_id = "vit_block_forward-" + "x".join(map(str, le.A_BLOCK))
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_vit_block, *le.A_BLOCK), 2 * _A[_id].bytes() + GIB))


# ---- training: the temporal conv ----------------------------------------------------------------------------------------------------
def tiled_running_var(rv_small, rv0, momentum, n_small, n_large):
    """The fp64 running variance after one step on the tiled batch, from the small batch's: the biased batch variance is the
    same, the unbiased one that the update takes differs by count / (count - 1)."""
    var_b = (rv_small - (1 - momentum) * rv0) / momentum * ((n_small - 1) / n_small)
    return (1 - momentum) * rv0 + momentum * var_b * (n_large / (n_large - 1))


def run_tcn_train(cin, cout, K, stride, T, V, math, ext, dev, grad_rel=1e-4):
    """tcn_forward_train + tcn_backward_train through the functional pair (the module's autograd would hold the product and the
    expanded cotangent as well: two more tensors of the result's size).  The forward's workspace and result are released before
    the backward allocates its own."""
    F = _F()
    s = ep.tcn_train(cin, cout, K, stride, ext.n0, T, V, math, kink_free=True)
    xt, ref = le.tiled(s, ext.R, dev, ext.N)
    m = s.module.to(dev)
    mode = _math(math)
    W = m.conv.weight.detach().reshape(cout, cin, K).contiguous()
    bn = m.bn
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    rv0 = rv.double().cpu()
    with poisoned() as h:
        y, z, mean, invstd = F.tcn_forward_train(xt, W, m.conv.bias.detach(), (bn.weight.detach(), bn.bias.detach(), rm, rv), stride,
                                                 mode, bn.momentum, bn.eps, save=True)
        sync_and_check(h)
    del h
    Tout = F.tcn_out_frames(T, K, stride)
    n_small, n_large = ext.n0 * Tout * V, ext.N * Tout * V
    print(ext.N, "clips: y", gate_tiled(y, ref["y"], 1e-4, True, "y"))
    del y
    le.release()
    # the saved statistics against the fp64 batch statistics of the small batch (= those of the tiled one)
    z64 = torch.nn.functional.conv2d(s.x.double(), m.conv.weight.detach().double().cpu(), m.conv.bias.detach().double().cpu(),
                                     stride=(stride, 1), padding=((K - 1) // 2, 0))
    mean64, var64 = z64.mean((0, 2, 3)), z64.var((0, 2, 3), unbiased=False)
    print("mean", gate_small(mean, mean64, 1e-4, "saved mean", True), "invstd",
          gate_small(invstd, (var64 + bn.eps).rsqrt(), 1e-4, "saved invstd", True))
    print("running_mean", gate_small(rm, ref["running_mean"], 1e-4, "running_mean", True), "running_var",
          gate_small(rv, tiled_running_var(ref["running_var"], rv0, bn.momentum, n_small, n_large), 1e-4, "running_var", True))
    dy = s.cotangent[0].to(dev).repeat(ext.R, 1, 1, 1)
    with poisoned() as h:
        dx, dW, dbias, dgamma, dbeta = F.tcn_backward_train(xt, W, z, bn.weight.detach(), bn.bias.detach(), mean, invstd, dy, stride, mode)
        sync_and_check(h)
    del h, dy, z
    le.release()
    print("dx", gate_tiled(dx, ref["dx"], 1e-4, False, "dx"))
    for k, g in (("dW", dW), ("dgamma", dgamma), ("dbeta", dbeta)):
        print(k, gate_small(g, ref[k] * ext.R, grad_rel, k))
    # analytically zero behind a batch-statistics BatchNorm: rounding noise, at the scale of the R-fold dbeta
    assert dbias.abs().max().item() <= 1e-3 * (ref["dbeta"] * ext.R).abs().max().item(), "dbias"


_id = "tcn_train-" + "x".join(map(str, le.A_TCN_TRAIN))
# the backward is the peak: x, z, dy, dx and a workspace that holds dz (the forward: x, y, z and a workspace that holds z)
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_tcn_train, *le.A_TCN_TRAIN), 5 * _A[_id].bytes() + GIB - le.GATE_BYTES))


# ---- training: the graph conv -------------------------------------------------------------------------------------------------------
def run_agcn_train(cin, cout, T, V, ext, dev, want_dx=False, grad_rel=1e-4):
    """unit_agcn's training step through the module.  Without ``want_dx`` the stem class (3 input channels, Cout of 64 / 128 /
    256) runs its moment form: the first layer needs no dx.  With it the call takes the GEMM chain (agcn_backward_generic.hip:
    the expansion recomputed, both pre-BatchNorm branches and their gradients in the workspace) and dx is gated too.  The
    statistics the forward saves for the backward are caught on their way out of agcn_forward_train."""
    F = _F()
    s = ep.agcn_train(cin, cout, ext.n0, T, V, want_dx=want_dx, kink_free=True)
    bns = {"bn": s.module.bn, "down": s.module.down[1]}
    rm0 = {k: b.running_mean.detach().double().cpu().clone() for k, b in bns.items()}
    rv0 = {k: b.running_var.detach().double().cpu().clone() for k, b in bns.items()}
    momentum, eps = s.module.bn.momentum, s.module.bn.eps
    xt, ref = le.tiled(s, ext.R, dev, ext.N)
    run = s.on(dev, fresh=True, tile=ext.R)
    saved, real = [], F.agcn_forward_train

    def catching(*args, **kw):
        out = real(*args, **kw)
        saved.append(out[4])
        return out
    F.agcn_forward_train = catching
    try:
        with poisoned() as h:
            o = run(xt)
            sync_and_check(h)
    finally:
        F.agcn_forward_train = real
    del h
    le.release()
    print(ext.N, "clips: y", gate_tiled(o["y"], ref["y"], 1e-4, True, "y"), "P", gate_tiled(o["P"], ref["P"], 1e-4, True, "P"))
    if want_dx:
        print("dx", gate_tiled(o["dx"], ref["dx"], 1e-4, False, "dx"))
    n_small, n_large = ext.n0 * T * V, ext.N * T * V
    assert len(saved) == 1 and saved[0] is not None, "the module's forward did not go through agcn_forward_train(save=...)"
    stats = saved[0][:4 * cout].double().cpu().view(4, cout)         # batch mean, invstd of bn; then of the down BatchNorm
    for i, k in enumerate(bns):
        want_rv = tiled_running_var(ref[k + ".running_var"], rv0[k], momentum, n_small, n_large)
        print(k, "running_mean", gate_small(o[k + ".running_mean"], ref[k + ".running_mean"], 1e-4, k + ".running_mean", True),
              "running_var", gate_small(o[k + ".running_var"], want_rv, 1e-4, k + ".running_var", True))
        # the fp64 batch statistics, out of the fp64 update of the small batch
        mean64 = (ref[k + ".running_mean"] - (1 - momentum) * rm0[k]) / momentum
        var64 = (ref[k + ".running_var"] - (1 - momentum) * rv0[k]) / momentum * ((n_small - 1) / n_small)
        print(k, "saved mean", gate_small(stats[2 * i], mean64, 1e-4, k + " saved mean", True),
              "saved invstd", gate_small(stats[2 * i + 1], (var64 + eps).rsqrt(), 1e-4, k + " saved invstd", True))
    ep.agcn_compare_grads({k: o["d" + k] for k in s.leaves}, {k: ref["d" + k] * ext.R for k in s.leaves}, grad_rel)


_id = "agcn_train-" + "x".join(map(str, le.A_AGCN_TRAIN))
# y, the cotangent, their product and its gradient (the setup's loss is (y * G).sum()), P, the moment form's workspace
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_agcn_train, *le.A_AGCN_TRAIN), 4 * _A[_id].bytes() + 2 * GIB))


# ---- ST-TR's attention unit ---------------------------------------------------------------------------------------------------------
def st_forward(n0, cin, cout, T, V, dev):
    """entry_points.st_attention's input and reference (the state of seed 7) and the functional call on the module's staged,
    folded parameters: ``run(x, math)`` -> {"y"}."""
    import st_attention_ref as R
    F = _F()
    s = ep.st_attention(n0, cin, cout, T, V)
    m = ep.st_unit(cin, cout, V, R.make_state(cin, cout, V, 7)).eval()
    st = m._staged(dev)
    ds, dsh, bs, bsh = m._folded(st)
    return s, lambda x, math: {"y": F.st_attention_forward(x, ds, dsh, st["Wqkv"], st["bqkv"], st["Wout"], st["bout"], bs, bsh, m._dk,
                                                           m._heads, math)}


def run_st_attention(cin, cout, T, V, math, ext, dev):
    """gcn_unit_attention's eval forward (st_attention_forward; with bf16x3 st_attention_forward_math, whose projections are
    stgcn_wx_product launches)."""
    s, run = st_forward(ext.n0, cin, cout, T, V, dev)
    xt, ref = le.tiled(s, ext.R, dev, ext.N)
    with poisoned() as h:
        o = run(xt, _math(math or "f32"))
        sync_and_check(h)
    assert o["y"].numel() == ext.result
    print(ext.N, "clips: y", gate_tiled(o["y"], ref["y"], 1e-4, True, "y"))


for _r in le.A_ST_ATTENTION:
    _id = "st_attention_forward-" + "x".join(map(str, _r[:4])) + "-" + (_r[4] or "f32")
    TABLE_A.append(Row(_id, _A[_id], functools.partial(run_st_attention, *_r), _A[_id].bytes() + 22 * GIB))     # y, a 20 GiB workspace


# ---- training: one block of the heads -------------------------------------------------------------------------------------------------
def run_vit_block_train(L, D, heads, hidden, ext, dev):
    """vit_block_forward_train + vit_block_backward (which run vit_layernorm_backward's and vit_linear_backward's kernels), fp32.
    y and dx are periodic; a parameter gradient is the small batch's times the whole tilings plus that of the clips left over."""
    F = _F()
    assert F.vit_block_train_supported(L, D, heads, hidden)
    x0, sd = ep.block_inputs(ext.n0, L, D, hidden)
    dy0 = torch.randn(ext.n0, L, D, generator=torch.Generator().manual_seed(L + D + 1))
    scale = (D // heads) ** -0.5
    want_y, want = tr.grads64(x0, sd, dy0, heads=heads, scale=scale)
    whole, left = divmod(ext.N, ext.n0)
    rest = tr.grads64(x0[:left], sd, dy0[:left], heads=heads, scale=scale)[1] if left else None
    xt = x0.to(dev).repeat(ext.R, 1, 1)[:ext.N].contiguous()
    dyt = dy0.to(dev).repeat(ext.R, 1, 1)[:ext.N].contiguous()
    flat = [t for pair in ep.block_params(sd, dev) for t in pair]
    with poisoned() as h:
        y, saved = F.vit_block_forward_train(xt, flat, heads, ar.EPS, scale, F.MATH_F32)
        g = F.vit_block_backward(xt, flat, saved, dyt, heads, ar.EPS, scale, F.MATH_F32)
        sync_and_check(h)
    del h, saved
    le.release()
    strict = ep.TRAIN_STRICT["f32"]
    print(ext.N, "sequences: y", gate_tiled(y, want_y, REL, strict, "y"), "dx", gate_tiled(g["x"], want["x"], REL, strict, "dx"))
    for k, name in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS):
        print(k, gate_small(g[name], want[k] * whole + (rest[k] if left else 0), REL, "d" + k, strict))


_id = "vit_block_train-" + "x".join(map(str, le.A_BLOCK_TRAIN))
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_vit_block_train, *le.A_BLOCK_TRAIN), 4 * _A[_id].bytes() + 22 * GIB - le.GATE_BYTES))


# ---- a whole head, the ST-ViT ends ----------------------------------------------------------------------------------------------------
def whole_head(T, V, dev):
    """entry_points.small_head for (T, V), its fp64 copy on the CPU and the keyword arguments of altformer_head_forward."""
    import copy
    import stgcn_amd
    head = ep.small_head(dev, "ST", num_frame=T, num_joints=V)
    head64 = copy.deepcopy(head).cpu().double().eval()
    stgcn_amd.set_whole_head(head)
    z0 = torch.relu(torch.randn(le.N0, 128, T, V, generator=torch.Generator().manual_seed(5)))      # the stem ends in a ReLU
    with torch.no_grad():
        want = head64(z0.double())
        plan = head._whole_plan(z0[:2].to(dev))          # (under no_grad: autograd must record nothing that concerns the head)
    assert plan is not None, "the small head does not take the one-call path"
    return z0, want, plan


def run_head(T, V, ext, dev):
    F = _F()
    z0, want, plan = whole_head(T, V, dev)
    zt = z0.to(dev).repeat(ext.R, 1, 1, 1)[:ext.N].contiguous()
    with poisoned() as h:
        logits = F.altformer_head_forward(zt, **plan)
        sync_and_check(h)
    print(ext.N, "clips: logits", gate_tiled(logits, want, REL, True, "logits"))


_id = "altformer_head_forward-%dx%d" % le.A_HEAD
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_head, *le.A_HEAD), _A[_id].N * 128 * le.A_HEAD[0] * le.A_HEAD[1] * 4 + 20 * GIB))


def run_vit_patch_embed(C, T, V, p1, p2, E, ext, dev):
    import stvit_ref as sr
    F = _F()
    K, n = p1 * p2 * C, (T // p1) * (V // p2)
    g = torch.Generator().manual_seed(5000 + K + n)
    z0 = sr.make_input(ext.n0, C, T, V, seed=5001 + n)
    W, bias = (torch.rand(E, K, generator=g) * 2 - 1) / K ** 0.5, (torch.rand(E, generator=g) * 2 - 1) / K ** 0.5
    cls, pos = torch.randn(E, generator=g), 0.5 * torch.randn(n + 1, E, generator=g)
    want = sr.embed64(z0, W, bias, cls, pos, p1, p2)
    assert F.vit_patch_embed_supported(ext.N, C, T, V, p1, p2, E)
    zt = z0.to(dev).repeat(ext.R, 1, 1, 1)[:ext.N].contiguous()
    assert zt.numel() == ext.named[1]
    Wd, bd, cd, pd = (t.to(dev) for t in (W, bias, cls, pos))
    with poisoned() as h:
        x = F.vit_patch_embed(zt, Wd, bd, cd, pd, p1, p2)
        sync_and_check(h)
    assert x.numel() == ext.result
    print(ext.N, "clips: x", gate_tiled(x, want, REL, True, "x"))


_id = "vit_patch_embed-" + "x".join(map(str, le.A_PATCH))
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_vit_patch_embed, *le.A_PATCH), _A[_id].named[1] * 4 + 2 * _A[_id].bytes() + 2 * GIB))


def run_vit_pool_classify(L, D, classes, ext, dev, modes=("max", "mean", "cls")):
    F = _F()
    g = torch.Generator().manual_seed(L + D + classes)
    x0 = torch.randn(ext.n0, L, D, generator=g) * 2 + 0.5
    lw, lb = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, b = torch.randn(classes, D, generator=g) / D ** 0.5, 0.1 * torch.randn(classes, generator=g)
    assert F.vit_pool_classify_supported(ext.N, L, D, classes)
    xt = x0.to(dev).repeat(ext.R, 1, 1)[:ext.N].contiguous()
    args = [t.to(dev) for t in (lw, lb)], [t.to(dev) for t in (W, b)]
    x64 = x0.double()
    for mode in modes:
        pooled = {"max": x64.max(1).values, "mean": x64.mean(1), "cls": x64[:, 0]}[mode]
        want = torch.nn.functional.layer_norm(pooled, (D,), lw.double(), lb.double(), 1e-5) @ W.double().T + b.double()
        with poisoned() as h:
            logits = F.vit_pool_classify(xt, *args[0], 1e-5, *args[1], mode=mode)
            sync_and_check(h)
        print(ext.N, "clips:", mode, gate_tiled(logits, want, REL, True, mode))
    return xt, args


_id = "vit_pool_classify-" + "x".join(map(str, le.A_POOL_CLASSIFY))
TABLE_A.append(Row(_id, _A[_id], functools.partial(run_vit_pool_classify, *le.A_POOL_CLASSIFY), _A[_id].named[1] * 4 + GIB))


# ---- Table B: the clip limit --------------------------------------------------------------------------------------------------------
LIMIT = le.MAX_CLIPS
SMALL = 2 * GIB               # what a Table B row holds: a few hundred MB


def refused(call, what, untouched=True):
    """``call`` raises the library's error with STGCN_ERR_UNSUPPORTED - not STGCN_ERR_HIP: a launch that HIP rejects means a guard
    is missing - and (``untouched``: a functional call, which stages nothing itself) has written nothing to what it allocated."""
    from stgcn_amd import StgcnError
    with poisoned() as h:
        with pytest.raises(StgcnError) as e:
            call()
        torch.cuda.synchronize()
        h.check()
        assert e.value.code == UNSUPPORTED, f"{what}: {e.value}"
        for i, (raw, nbytes, shape, dtype) in enumerate(h.records if untouched else ()):
            assert bool((raw == h.fill).all()), f"{what}: allocation #{i} (shape {shape}, {dtype}) was written by a refused call"


def at_the_limit(s, run, gates, dev, limit=LIMIT, over=True):
    """``run(x)`` -> {name: result}: correct everywhere at ``limit`` clips, refused at ``limit + 1`` (``over``), and correct on two
    clips afterwards - no error state is left behind.  ``gates``: {name: (rel, strict)}."""
    R = -(-(limit + 1) // len(s.x))
    xt, ref = le.tiled(s, R, dev, limit + 1)
    with poisoned() as h:
        o = run(xt[:limit].contiguous())
        sync_and_check(h)
    print(limit, "clips:", {k: gate_tiled(o[k], ref[k], *g, k) for k, g in gates.items()})
    del o, h
    if over:
        refused(lambda: run(xt), f"{limit + 1} clips")
        o = run(xt[:2].contiguous())
        torch.cuda.synchronize()
        for k, g in gates.items():
            gate_tiled(o[k], ref[k][:2], *g, f"{k} after the refusal")


def limit_stem(dev):
    s = ep.stem(le.N0, 1, 7, 128)
    staged = s.on(dev)
    mode = _math("bf16x3")
    prep = staged.prepare(mode)
    at_the_limit(s, lambda x: dict(zip(("out", "P"), staged.forward(x, prep, mode))), {"out": MATH_GATES["bf16x3"], "P": (1e-4, True)}, dev)


def limit_agcn(dev):
    """agcn_forward (which stops the setup's run at 65536) and agcn_attention on its own."""
    F = _F()
    s = ep.agcn(le.N0, 3, 64, 1, 7)
    run = s.on(dev)
    at_the_limit(s, run, {k: (1e-4, True) for k in ("y", "P", "P_attention")}, dev)
    st = s.module._staged(dev)
    at_the_limit(s, lambda x: {"P_attention": F.agcn_attention(x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"])},
                 {"P_attention": (1e-4, True)}, dev)


def limit_tcn(dev):
    s = ep.tcn(128, 128, 9, 1, 1, 7, le.N0, "bf16x3", False, False)
    at_the_limit(s, s.on(dev), {k: MATH_GATES["bf16x3"] for k in ("y_packed", "y_one_shot")}, dev)


def limit_patch_embed(dev):
    for order in ("ST", "TS"):
        s = ep.patch_embed(order, "nctv", N=le.N0, T=2, V=3)
        at_the_limit(s, s.on(dev), {"e": (1e-4, False), "e_no_pos": (1e-4, False)}, dev)


def limit_tcn_train(dev):
    """The training pair at 65535 = 5 * 13107 clips (a whole number of 5-clip batches: the batch statistics are the small batch's).
    The forward takes more - its one-wave convolution sums the statistics in a persistent kernel, no clip in its grid (tcn.hip),
    and the BatchNorm kernels walk the clips - so it runs at 65541 = 7 * 9363 clips (65537 is prime: no tiling has its
    statistics); the backward refuses 65536."""
    F = _F()
    cin, cout, K, stride, T, V, math = 128, 128, 9, 1, 1, 7, "bf16x3"
    run_tcn_train(cin, cout, K, stride, T, V, math, Extent(LIMIT, (cout, T, V), n0=5), dev)
    ext = Extent(65541, (cout, T, V))
    s = ep.tcn_train(cin, cout, K, stride, ext.n0, T, V, math, kink_free=True)
    xt, ref = le.tiled(s, ext.R, dev)
    m = s.module.to(dev)
    W = m.conv.weight.detach().reshape(cout, cin, K).contiguous()
    bn = (m.bn.weight.detach(), m.bn.bias.detach(), m.bn.running_mean.clone(), m.bn.running_var.clone())
    with poisoned() as h:
        y, z, mean, invstd = F.tcn_forward_train(xt, W, m.conv.bias.detach(), bn, stride, _math(math), save=True)
        sync_and_check(h)
    print(ext.N, "clips: y", gate_tiled(y, ref["y"], 1e-4, True, "y"))
    print("running_mean", gate_small(bn[2], ref["running_mean"], 1e-4, "running_mean", True))
    dy = torch.ones_like(y)
    n = LIMIT + 1
    refused(lambda: F.tcn_backward_train(xt[:n], W, z[:n], bn[0], bn[1], mean, invstd, dy[:n], stride, _math(math)), f"backward, {n} clips")
    del xt, y, z, dy
    run_tcn_train(cin, cout, K, stride, T, V, math, Extent(2, (cout, T, V), n0=2), dev)       # no error state is left behind


def limit_agcn_train(dev, want_dx=False):
    """The moment form: 65535 clips, 65536 refused (by the forward), 2 clips after.  With ``want_dx`` the GEMM chain
    (agcn_backward_generic.hip) and its input gradient: a batch entry per (clip, subset) pair on a 16-bit grid axis, so 21845 =
    65535 / 3 clips are its limit (5 * 4369: a whole number of 5-clip batches); 21846 are refused by the backward, before launch."""
    cin, cout, T, V = 3, 64, 1, 7
    limit = LIMIT // 3 if want_dx else LIMIT
    run_agcn_train(cin, cout, T, V, Extent(limit, (cout, T, V), n0=5), dev, want_dx)
    n0 = 6 if want_dx else 4
    s = ep.agcn_train(cin, cout, n0, T, V, want_dx=want_dx, kink_free=True)
    s.reference(s.x)
    R = (limit + 1) // n0
    run = s.on(dev, fresh=True, tile=R)
    xt = s.x.to(dev).repeat(R, 1, 1, 1)
    assert len(xt) == limit + 1
    refused(lambda: run(xt), f"{limit + 1} clips", untouched=False)      # (through the module, which stages its parameters)
    if want_dx:       # the entry point itself, on operands whose values do not matter: nothing it was given is written
        F = _F()
        st, bn, d = s.module._staged(dev), s.module.bn, s.module.down[1]
        zeros = lambda *shape: torch.zeros(*shape, device=dev)       # noqa: E731
        P, stats, dy = zeros(limit + 1, 3, V, V), zeros(4 * cout + 128), zeros(limit + 1, cout, T, V)
        refused(lambda: F.agcn_backward_train(xt, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"],
                                              st["bdown"], P, None, None, bn.weight.detach(), bn.bias.detach(), d.weight.detach(),
                                              d.bias.detach(), stats, dy, need_dx=True), f"agcn_backward_train, {limit + 1} clips")
    del xt
    run_agcn_train(cin, cout, T, V, Extent(2, (cout, T, V), n0=2), dev, want_dx)


# the heads put sequences on grid.x: 65537 of the shortest sequences each entry point takes
SEQS = LIMIT + 2


def limit_vit_linear(dev):
    run_vit_linear("f32", True, True, Extent(SEQS, (1, 64)), dev, K=32, Nout=64, group=1)
    run_vit_linear("bf16x3", False, False, Extent(SEQS, (1, 64)), dev, K=32, Nout=64, group=1)


def limit_vit_attention(dev):
    """L = 1 is the shortest sequence, but its soft-max is 1 whatever q and k hold (out = v): L = 2 with peaked scores makes the
    row feel a mis-addressed q or k too."""
    for form in ("resident", "stream", "split"):
        for L in (1, 2):
            run_vit_attention(form, L, 32, Extent(SEQS, (L, 256)), dev)


def limit_vit_block(dev):
    run_vit_block(1, 256, 8, 512, Extent(SEQS, (1, 256)), dev)


def limit_vit_pool(dev):
    F = _F()
    L, D = 2, 256
    assert F.vit_pool_supported(SEQS, L, D)
    x0 = torch.randn(le.N0, L, D, generator=torch.Generator().manual_seed(L + D))
    xt = x0.to(dev).repeat(-(-SEQS // le.N0), 1, 1)[:SEQS].contiguous()
    for mode, want in (("mean", x0.double().mean(1)), ("max", x0.double().max(1).values), ("cls", x0.double()[:, 0])):
        with poisoned() as h:
            out = F.vit_pool(xt, mode)
            sync_and_check(h)
        print(SEQS, "sequences:", mode, gate_tiled(out, want, REL, True, mode))


def limit_st_attention(dev):
    F = _F()
    s, run = st_forward(le.N0, 3, 128, 1, 2, dev)
    for math in (F.MATH_F32, F.MATH_BF16X3):
        at_the_limit(s, lambda x: run(x, math), {"y": (1e-4, True)}, dev)


def limit_head(dev):
    """altformer_head_forward: 65535 clips of 1 x 2 (its embeddings put the clip on a grid axis), 65536 refused."""
    F = _F()
    z0, want, plan = whole_head(1, 2, dev)
    s = ep.Setup(z0, lambda z: {"logits": want}, None)
    at_the_limit(s, lambda z: {"logits": F.altformer_head_forward(z, **plan)}, {"logits": (REL, True)}, dev)


def limit_vit_block_train(dev):
    run_vit_block_train(1, 64, 2, 64, Extent(SEQS, (1, 64)), dev)


def limit_vit_pool_classify(dev):
    """One workgroup of 1024 threads per clip: 2^22 - 1 clips are the most a launch holds; one more is refused."""
    F = _F()
    n = le.POOL_CLASSIFY_CLIPS
    xt, (ln, lin) = run_vit_pool_classify(1, 64, 14, Extent(n - 1, (14,)), dev, modes=("max",))
    more = torch.cat((xt, xt[:1]))
    assert not F.vit_pool_classify_supported(n, 1, 64, 14)
    refused(lambda: F.vit_pool_classify(more, *ln, 1e-5, *lin), f"{n} clips")
    del xt, more
    run_vit_pool_classify(1, 64, 14, Extent(2, (14,), n0=2), dev, modes=("max",))             # no error state is left behind


for _name, _run in (("st_attention_forward", limit_st_attention), ("altformer_head_forward", limit_head),
                    ("vit_block_train", limit_vit_block_train), ("vit_pool_classify", limit_vit_pool_classify)):
    TABLE_B.append(Row("limit-" + _name, None, _run, 2 * SMALL))


for _name, _run in (("stem", limit_stem), ("agcn_forward+agcn_attention", limit_agcn), ("tcn_forward_packed", limit_tcn),
                    ("patch_embed", limit_patch_embed), ("tcn_train", limit_tcn_train), ("agcn_train", limit_agcn_train),
                    ("agcn_train-dx-gemm_chain", functools.partial(limit_agcn_train, want_dx=True)), ("vit_linear", limit_vit_linear), ("vit_attention", limit_vit_attention), ("vit_block_forward", limit_vit_block),
                    ("vit_pool", limit_vit_pool)):
    TABLE_B.append(Row("limit-" + _name, None, _run, SMALL))


# ---- the tests over the tables ------------------------------------------------------------------------------------------------------
def test_every_row_of_table_a_is_large_and_alias_free():
    assert sorted(r.id for r in TABLE_A) == sorted(_A) and len(TABLE_A) == len(_A), "a row of large_extent.table_a() has no runner, or the other way round"
    for r in TABLE_A:
        r.ext.assert_large_and_alias_free(r.id)
        assert r.ext.N <= LIMIT or r.id.startswith("vit_"), f"{r.id}: {r.ext.N} clips ride on no 16-bit grid axis"
        le.need_bytes(r)


@pytest.mark.parametrize("row", TABLE_A, ids=lambda r: r.id)
def test_result_past_2_31_elements_matches_the_tiled_reference(row, dev):
    row.ext.assert_large_and_alias_free(row.id)
    le.skip_unless_it_fits(row)
    try:
        row.run(row.ext, dev)
    finally:
        le.release()


@pytest.mark.parametrize("row", TABLE_B, ids=lambda r: r.id)
def test_clip_limit(row, dev):
    le.skip_unless_it_fits(row)
    try:
        row.run(dev)
    finally:
        le.release()
