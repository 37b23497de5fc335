"""The case table, the planting helpers and the conditions of the non-finite contract: what the HIP paths must do
with an input that holds ONE non-finite value.  Shared by tests/test_nonfinite_host.py (the references make every case
meaningful, no GPU) and tests/test_nonfinite_gpu.py (the HIP paths meet the conditions).  Not a conftest.py: a plain module.

A case plants one value at one position of one input, runs the fp64 restatement the existing tests use for the entry point
(oracle.stgcn_oracle, altformer_ref, altformer_train_ref, st_attention_ref; the torch path in fp64 on the CPU for whole modules)
and the HIP path on the same planted input.  Against the reference OF THE PLANTED INPUT:

  (a) nothing hidden: wherever the reference is non-finite the HIP output is non-finite (NaN and Inf are not told apart) -
      every planted value, every arithmetic, every output (statistics, running buffers, gradients, bf16-stored outputs);
  (b) nothing leaked (planted NaN): wherever the reference is finite the HIP output is finite and passes the entry point's own
      gate there (tests/_util.py::MATH_GATES; the scale is max|ref| over the finite elements) - so the two masks are equal;
  (c) planted +-inf: the split arithmetics turn an Inf operand into NaN (bf16x3: lo = x - hi = inf - inf; bf16 and f16mx
      alike) where the reference's relu(-inf) = 0 is finite, so (b) holds as written for 'f32' and 'f32_valu' only; the other
      modes owe (a) plus (b) on the units the planted element cannot reach in the reference (the other clips / sequences /
      rows).  'f16mx' has no Inf cases: its scales follow the input magnitude (max|x| per clip), so an Inf input is outside
      what the mode defines.

Training with batch statistics owes (a) only: in the reference one NaN reaches everything.

Out of scope: non-finite PARAMETERS (the prepacked blobs and their restaging are a topic of their own) and the
eval-with-gradients backward."""
import functools
import math

import torch
import torch.nn.functional as TF

import altformer_ref as ar
import altformer_train_ref as tr
import st_attention_ref as R
from _util import MATH_GATES

BF16_OUT_GATE = 4e-3          # a bf16-stored output: half an ulp of the stored value on top of the arithmetic (max-norm)
SPLIT_MATHS = ("bf16x3", "bf16", "mixed")     # arithmetics that split or round their operands: an Inf operand becomes NaN


def _nan_all_ones():
    return torch.tensor([-1], dtype=torch.int32).view(torch.float32)[0]


# the canonical NaN; the NaN with an all-ones payload (0xFFFFFFFF, the hostile allocator's fill: a round-to-bf16 done by integer
# addition would wrap it to zero); the infinities
VALUES = {"nan": torch.tensor(float("nan")), "nan_ones": _nan_all_ones(), "+inf": torch.tensor(float("inf")),
          "-inf": torch.tensor(float("-inf"))}
assert VALUES["nan_ones"].view(torch.int32).item() == -1 and bool(torch.isnan(VALUES["nan_ones"]))


def plant(x, index, value):
    """A copy of ``x`` (fp32, CPU) with VALUES[value] - the exact bits - at ``index``."""
    y = x.clone()
    y.view(torch.int32)[tuple(index)] = VALUES[value].view(torch.int32)
    return y


# ---- positions --------------------------------------------------------------------------------------------------------------
def clip_positions(shape, K=9):
    """Where kernels over (N, C, T, V) go wrong: first / last element (clip 0, the last clip), joint V-1 beside the padded
    columns, the first frame of the second 128- and 256-pixel time tile (a frame of one tile that is the halo of its
    neighbour), joints 23 | 24 either side of the wide-frame kernel's split."""
    N, C, T, V = shape
    pos = [("first", (0, 0, 0, 0)), ("last", (N - 1, C - 1, T - 1, V - 1)), ("joint_V-1", (0, C // 2, T // 2, V - 1))]
    for pixels in (128, 256):
        t = max(1, pixels // V)
        if t < T - 1:
            pos.append((f"halo_t{t}", (N - 1, 0, t, V // 2)))
    if V == 46:
        pos += [("joint_23", (0, 0, T // 2, 23)), ("joint_24", (N - 1, C - 1, T // 2, 24))]
    return pos


def token_positions(shape):
    """(B, L, D) inputs of the heads: token 0 (LayerNorm centres on the row's first element), token L-1 (off the 32-key tile
    where L is), features 0 and D-1."""
    B, L, D = shape
    pos = [("first", (0, 0, 0)), ("last", (B - 1, L - 1, D - 1)), ("token_0", (B // 2, 0, D // 2)), ("token_L-1", (B // 2, L - 1, 1)),
           ("feature_0", (B - 1, L // 2, 0)), ("feature_D-1", (0, L // 2, D - 1))]
    return pos


def row_positions(shape):
    M, K = shape
    return [("first", (0, 0)), ("last", (M - 1, K - 1)), ("feature_0", (M // 2, 0)), ("feature_K-1", (M // 2, K - 1))]


# ---- the table --------------------------------------------------------------------------------------------------------------
class Prepared:
    """What ``Case.prepare()`` returns.  ``x``: the clean fp32 CPU input; ``positions``: [(label, index)]; ``reference(x)``:
    {name: fp64 tensor} on the CPU; ``device(dev)``: prepares the HIP side once and returns ``run(x) -> {name: tensor}`` with the
    same names.  Every output's axis 0 is the unit axis (clip, sequence or row) unless ``global_outputs`` names it (parameter
    gradients, statistics: no unit); the unit a planted element belongs to is ``index[0]``.  ``gates``: {name: (rel, strict)},
    ``gate`` for the rest."""

    def __init__(self, x, positions, reference, device, gate, gates=None, global_outputs=()):
        self.x, self.positions, self.reference, self.device = x, positions, reference, device
        self.gate, self.gates, self.global_outputs = gate, gates or {}, set(global_outputs)


class Case:
    """``math``: the arithmetic that decides what a planted Inf owes (c); ``training``: only (a) applies."""

    def __init__(self, id, prepare, math, training=False, kernel=None, without=()):
        self.id, self._prepare, self.math, self.training, self.kernel = id, prepare, math, training, kernel
        self.without = set(without) | ({"+inf", "-inf"} if math == "f16mx" else set())   # (c): f16mx defines no Inf input

    @functools.lru_cache(maxsize=None)
    def prepare(self):
        return self._prepare()

    def plants(self):
        """[(label, index, value)]: every position with the canonical NaN, the other values at the first and the last."""
        pos = self.prepare().positions
        out = [(label, idx, "nan") for label, idx in pos]
        for v in ("nan_ones", "+inf", "-inf"):
            if v in self.without:
                continue
            out += [(label, idx, v) for label, idx in pos if label in ("first", "last")]
        return out

    def owes(self, value):
        """'a' | 'units' | 'full' - see the module docstring."""
        if self.training:
            return "a"
        if value.endswith("inf") and self.math in SPLIT_MATHS:
            return "units"
        return "full"


CASES = []


def add(id, math, prepare, *args, training=False, kernel=None, without=()):
    CASES.append(Case(id, functools.partial(prepare, *args), math, training, kernel, without))


def nonfinite(t):
    return ~torch.isfinite(t.detach().double().cpu())


# ---- the conditions -----------------------------------------------------------------------------------------------------------
def check(case, prep, index, value, out, ref, what):
    """(a) - (c) for one plant; prints each figure before it asserts."""
    owes = case.owes(value)
    for name, r in ref.items():
        o = out[name]
        assert o is not None, f"{what}: output {name} is missing"
        o, r = o.detach().double().cpu().reshape(r.shape), r.detach().double()
        bad_r, bad_o = ~torch.isfinite(r), ~torch.isfinite(o)
        hidden = int((bad_r & ~bad_o).sum())
        print(f"{what} {name}: reference non-finite {int(bad_r.sum())}/{r.numel()}, HIP {int(bad_o.sum())}, hidden {hidden} [{owes}]")
        assert hidden == 0, f"{what} {name}: (a) {hidden} of {int(bad_r.sum())} non-finite reference elements came out finite"
        if owes == "a":
            continue
        if owes == "units":
            if name in prep.global_outputs:
                continue
            keep = torch.ones(r.shape[0], dtype=torch.bool)
            keep[index[0]] = False
            o, r, bad_o, bad_r = o[keep], r[keep], bad_o[keep], bad_r[keep]
        leaked = int((bad_o & ~bad_r).sum())
        assert leaked == 0, f"{what} {name}: (b) {leaked} elements are non-finite where the reference is finite"
        fin = ~bad_r
        if not bool(fin.any()):
            continue
        rel, strict = prep.gates.get(name, prep.gate)
        scale = r[fin].abs().max().item()
        err = (o[fin] - r[fin]).abs().max().item()
        print(f"{what} {name}: on the finite elements max|err| / max|ref| = {err / max(scale, 1e-30):.3e} (gate {rel:g})")
        assert err <= rel * max(scale, 1e-30), f"{what} {name}: (b) max abs err {err:.3e} > {rel:g} * max|ref| ({scale:.3e})"
        if strict:
            assert torch.allclose(o[fin], r[fin], rtol=rel, atol=rel * 0.1 * scale), f"{what} {name}: (b) allclose(rtol={rel}) failed"


def reference_makes_sense(case, prep, index, value, clean, ref, what):
    """The host file's three conditions on one plant."""
    for name, r in clean.items():
        assert bool(torch.isfinite(r).all()), f"{what}: the clean reference's {name} is not finite"
    assert any(bool(nonfinite(r).any()) for r in ref.values()), f"{what}: the planted value reaches no output of the reference"
    if case.owes(value) == "a":
        return
    ok = False
    for name, r in ref.items():
        if name in prep.global_outputs:
            continue
        fin = torch.isfinite(r).reshape(r.shape[0], -1)
        touched = fin[index[0]]
        ok = ok or (bool(touched.any()) and not bool(touched.all())) or bool(fin.all(dim=1).any())
    assert ok, f"{what}: claims (b), but no touched unit keeps a finite element and no unit is wholly finite"


# ---- eval forward: graph conv ---------------------------------------------------------------------------------------------------
def _F():
    from stgcn_amd import functional as F
    return F


def _math(name):
    F = _F()
    return {"f32": F.MATH_F32, "bf16x3": F.MATH_BF16X3, "bf16": F.MATH_BF16, "f32_valu": F.MATH_F32_VALU, "f16mx": F.MATH_F16MX}[name]


def _random_stem(V, seed, cin=3, c=128):
    from test_gpu_parity import _random_stem as rs
    return rs(V, None, seed, torch.device("cpu"), cin=cin, c=c)


def two_clips(shape):
    """A shape of the borrowed tables with a second clip where it has one: (b) across clips needs another clip."""
    return (max(shape[0], 2),) + tuple(shape[1:])


def prepare_agcn(N, cin, cout, T, V):
    from oracle import stgcn_oracle as so
    gcn, _, gp, _, gen = _random_stem(V, 3000 + cin + cout + T + V, cin=cin, c=cout)
    gp = gp.to(torch.float64)
    x = torch.randn(N, cin, T, V, generator=gen)

    def reference(x):
        aux = {}
        y = so.agcn_forward(x.double(), gp, aux=aux)
        return {"y": y, "P": aux["P"], "P_attention": aux["P"]}

    def device(dev):
        F = _F()
        gcn.to(dev).eval()
        st = gcn._staged(dev)
        gcn._folded(st)

        def run(x):
            xd = x.to(dev)
            y, P = F.agcn_forward(xd, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], st["Wd"], st["bd"], st["Wdown"], st["bdown"],
                                  st["bn_scale"], st["bn_shift"], st["down_scale"], st["down_shift"])
            return {"y": y, "P": P, "P_attention": F.agcn_attention(xd, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"])}
        return run
    return Prepared(x, clip_positions(x.shape), reference, device, MATH_GATES["f32"])


# ---- eval forward: temporal conv --------------------------------------------------------------------------------------------------
def prepare_tcn(cin, cout, K, stride, T, V, N, math, out_bf16, along_v):
    from stgcn_amd import Unit2D
    from oracle import stgcn_oracle as so
    gen = torch.Generator().manual_seed(cin + cout + K + T)
    torch.manual_seed(5)
    m = Unit2D(cin, cout, kernel_size=K, stride=stride, dim=3 if along_v else 2)
    with torch.no_grad():
        m.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
        m.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        m.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        m.bn.running_mean.copy_(torch.randn(cout, generator=gen) * 0.3)
        m.bn.running_var.copy_(torch.rand(cout, generator=gen) + 0.25)
    x = torch.randn(N, cin, T, V, generator=gen)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    if along_v:
        sd["conv.weight"] = sd["conv.weight"].permute(0, 1, 3, 2)
    tp = so.tcn_params_from_state(sd, stride=stride).to(torch.float64)

    def reference(x):
        y = so.tcn_forward(x.double().transpose(2, 3), tp).transpose(2, 3) if along_v else so.tcn_forward(x.double(), tp)
        return {"y_packed": y} if along_v else {"y_packed": y, "y_one_shot": y}

    def device(dev):
        from test_buffer_discipline_gpu import _tcn_mode
        F = _F()
        st = m.to(dev).eval()._staged(dev)
        mode, _ = _tcn_mode(cin, cout, K, stride, T, V, math, along_v)
        Wp = F.tcn_pack(st["W"], st["scale"], mode)

        def run(x):
            xd = x.to(dev)
            out = {"y_packed": F.tcn_forward_packed(xd, Wp, st["shift"], cout, K, stride, mode, out_bf16, along_v=along_v)}
            if not along_v:
                out["y_one_shot"] = F.tcn_forward(xd, st["W"], st["scale"], st["shift"], stride, mode, out_bf16)
            assert all(y.dtype == (torch.bfloat16 if out_bf16 else torch.float32) for y in out.values())
            return out
        return run
    return Prepared(x, clip_positions(x.shape, K), reference, device, (BF16_OUT_GATE, False) if out_bf16 else MATH_GATES[math])


def tcn_case_math(cin, cout, K, stride, T, V, math, along_v):
    """The arithmetic the call runs in (Unit2D's rule sends what the matrix-core kernels do not cover to the VALU kernel)."""
    from test_buffer_discipline_gpu import _tcn_mode
    F = _F()
    mode, kernel = _tcn_mode(cin, cout, K, stride, T, V, math, along_v)
    return ("f32_valu" if mode == F.MATH_F32_VALU else math), kernel


# ---- eval forward: the stem -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem_setup(N, T, V, C):
    gcn, tcn, gp, tp, gen = _random_stem(V, 100 + T + V, c=C)
    return gcn, tcn, gp.to(torch.float64), tp.to(torch.float64), torch.randn(N, 3, T, V, generator=gen)


def _stem_reference(gp, tp):
    from oracle import stgcn_oracle as so

    def reference(x):
        aux = {}
        ref = so.stem_forward(x.double(), gp, tp, aux=aux)
        return ref, aux["gcn"]["P"], aux["gcn_out"]
    return reference


STEM_VARIANTS = [("nctv", "nctv", False), ("nctv", "ntvc", False), ("ntvc", "nctv", False), ("ntvc", "ntvc", True), ("nctv", "nctv", True)]


def prepare_stem_fused(shape, math):
    """The fused kernels through F.stem_forward: (N,3,T,V) and (N,T,V,3) in, (N,C,T,V) and (N,T,V,C) out, fp32 and bf16 stored."""
    N, T, V, C = shape
    gcn, tcn, gp, tp, x = _stem_setup(N, T, V, C)
    full = _stem_reference(gp, tp)
    tag = lambda i, o, b: f"[{i}->{o},{'bf16' if b else 'f32'}]"       # noqa: E731

    def reference(x):
        ref, P, _ = full(x)
        out = {}
        for v in STEM_VARIANTS:
            out["out" + tag(*v)], out["P" + tag(*v)] = ref, P
        return out

    def device(dev):
        F = _F()
        mode = _math(math)
        gcn.to(dev).eval(), tcn.to(dev).eval()
        st, ts = gcn._staged(dev), tcn._staged(dev)
        gcn._folded(st)
        prep = F.stem_prepare(st["Wd"], st["bd"], st["Wdown"], st["bdown"], st["bn_scale"], st["bn_shift"], st["down_scale"],
                              st["down_shift"], ts["W"], ts["scale"], mode)

        def run(x):
            out = {}
            for i, o, b in STEM_VARIANTS:
                xd = x.to(dev)
                if i == "ntvc":
                    xd = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                out["out" + tag(i, o, b)], P = F.stem_forward(xd, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], prep, ts["shift"],
                                                              C, 9, mode, b, channels_last_out=o == "ntvc")
                out["P" + tag(i, o, b)] = P.clone()
            return out
        return run
    rel, strict = MATH_GATES[math]
    gates = {}
    for v in STEM_VARIANTS:
        gates["P" + tag(*v)] = MATH_GATES["f32"]
        if v[2]:
            gates["out" + tag(*v)] = (max(rel, BF16_OUT_GATE), False)
    return Prepared(x, clip_positions(x.shape), reference, device, (rel, strict), gates)


def prepare_stem_two_stage(shape, math):
    """tcn0(gcn0(x)) through the modules without fusion: the graph conv's expansion, then the temporal conv's kernel."""
    N, T, V, C = shape
    gcn, tcn, gp, tp, x = _stem_setup(N, T, V, C)
    full = _stem_reference(gp, tp)

    def reference(x):
        ref, P, y = full(x)
        return {"z": ref, "P": P, "gcn_out": y}

    def device(dev):
        from stgcn_amd import set_math_mode
        gcn.to(dev).eval(), tcn.to(dev).eval()
        set_math_mode(tcn, math)
        assert not getattr(gcn, "_fused_with", None)

        def run(x):
            with torch.no_grad():
                y = gcn(x.to(dev))
                z = tcn(y)
            return {"z": z, "P": gcn.last_attention, "gcn_out": y}
        return run
    return Prepared(x, clip_positions(x.shape), reference, device, MATH_GATES[math], {"P": MATH_GATES["f32"], "gcn_out": MATH_GATES["f32"]})


# ---- eval forward: patch embedding, ST-TR unit -----------------------------------------------------------------------------------
def prepare_patch_embed(order, layout):
    N, C, T, V, E = 2, 128, 9, 25, 256
    g = torch.Generator().manual_seed(61 + (order == "TS"))
    z = torch.randn(N, C, T, V, generator=g)
    W, b = torch.randn(E, C, generator=g) / C ** 0.5, torch.randn(E, generator=g) * 0.1
    pos = torch.randn(1, T if order == "TS" else V, E, generator=g) * 0.05
    L = V if order == "ST" else T

    def reference(z):
        tok = z.permute(0, 2, 3, 1).reshape(N * T, V, C) if order == "ST" else z.permute(0, 3, 2, 1).reshape(N * V, T, C)
        e = tok.double() @ W.double().T + b.double()
        return {"e": (e + pos.double()).reshape(N, -1, L, E), "e_no_pos": e.reshape(N, -1, L, E)}        # axis 0: the clip

    def device(dev):
        F = _F()
        Wd, bd, pd = W.to(dev), b.to(dev), pos.to(dev)

        def run(z):
            zd = z.to(dev)
            if layout == "ntvc":
                zd = zd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            return {"e": F.patch_embed(zd, Wd, bd, pd, order=order).reshape(N, -1, L, E),
                    "e_no_pos": F.patch_embed(zd, Wd, bd, None, order=order).reshape(N, -1, L, E)}
        return run
    return Prepared(z, clip_positions(z.shape), reference, device, (1e-4, False))


def _st_unit(cin, cout, V, sd, drop_connect=True):
    from test_st_attention_gpu import _unit
    return _unit(cin, cout, V, sd, drop_connect)


def prepare_st_attention(N, cin, cout, T, V):
    sd = R.make_state(cin, cout, V, 7)
    x = R.make_input(N, cin, T, V, 8)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}

    def reference(x):
        return {"y": R.forward64(sd64, x.double(), False)[0]}

    def device(dev):
        m = _st_unit(cin, cout, V, sd).eval()
        m._folded(m._staged(dev))

        def run(x):
            with torch.no_grad():
                return {"y": m(x.to(dev))}
        return run
    return Prepared(x, clip_positions(x.shape), reference, device, MATH_GATES["f32"])


# ---- heads, inference ---------------------------------------------------------------------------------------------------------
TILE_FORMS = {(128, 128): 0, (64, 64): 0x20000, (32, 64): 0x30000}


def prepare_vit_linear(M, K, Nout, math):
    g = torch.Generator().manual_seed(M + K + Nout)
    x = torch.randn(M, K, generator=g) * (0.25 + 3.75 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    W = (torch.rand(Nout, K, generator=g) * 2 - 1) / K ** 0.5
    b = torch.randn(Nout, generator=g) * 0.5
    Rr = torch.randn(M, Nout, generator=g)
    lw, lb = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)

    def reference(x):
        xn = ar.layer_norm64(x.double(), lw.double(), lb.double())
        on, off = TF.gelu(xn @ W.double().T + b.double()) + Rr.double(), x.double() @ W.double().T
        return {f"{k}{tile}": v for tile in TILE_FORMS for k, v in (("on", on), ("off", off))}

    def device(dev):
        F = _F()
        mode = _math(math)
        Wd, bd, Rd, lwd, lbd = (t.to(dev) for t in (W, b, Rr, lw, lb))

        def run(x):
            xd, out = x.to(dev), {}
            for tile, fl in TILE_FORMS.items():
                assert F.vit_linear_tile(M, K, Nout, mode | fl) == tile
                out[f"on{tile}"] = F.vit_linear(xd, Wd, bd, ln=(lwd, lbd, ar.EPS), residual=Rd, gelu=True, math=mode | fl)
                out[f"off{tile}"] = F.vit_linear(xd, Wd, None, math=mode | fl)
            return out
        return run
    return Prepared(x, row_positions(x.shape), reference, device, MATH_GATES[math])


def prepare_vit_attention(form, B, L, hd):
    from test_altformer_gpu import peaked_qkv
    heads = 8
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd)

    def reference(qkv):
        return {"out": ar.attention64(qkv, heads, hd ** -0.5)}

    def device(dev):
        F = _F()
        entry = {"resident": F.vit_attention, "stream": F.vit_attention_stream, "split": F.vit_attention_split}[form]
        if form == "stream":
            assert F.vit_attention_stream_supported(L, heads, hd)
        if form == "split":
            assert F.vit_attention_split_supported(L, heads, hd)
        return lambda qkv: {"out": entry(qkv.to(dev), heads)}
    return Prepared(qkv, token_positions(qkv.shape), reference, device, MATH_GATES["f32"])


def _block_inputs(B, L, D, hidden):
    sd = ar.random_block_state(D, hidden, True, seed=B + L + D)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    return x, sd


def _block_params(sd, dev):
    sdd = {k: v.to(dev) for k, v in sd.items()}
    pair = lambda n: (sdd[n + ".weight"], sdd[n + ".bias"])       # noqa: E731
    return (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))


def prepare_vit_block(B, L, D, heads, hidden, mode):
    x, sd = _block_inputs(B, L, D, hidden)

    def reference(x):
        return {"y": ar.block64(x, sd, heads=heads)[0]}

    def device(dev):
        from stgcn_amd.altformer import HEAD_MATH
        F = _F()
        params = _block_params(sd, dev)
        return lambda x: {"y": F.vit_block_forward(x.to(dev), *params, heads, ar.EPS, (D // heads) ** -0.5, HEAD_MATH[mode])}
    return Prepared(x, token_positions(x.shape), reference, device, MATH_GATES["bf16"] if mode == "bf16" else MATH_GATES["f32"])


def _pool_input(S, L, D):
    g = torch.Generator().manual_seed(S + L + D)
    return torch.randn(S, L, D, generator=g) * (0.25 + 3.75 * torch.rand(S, 1, D, generator=g)) + torch.randn(S, 1, 1, generator=g)


def prepare_vit_pool(S, L, D, mode):
    x = _pool_input(S, L, D)

    def reference(x):
        return {"out": x.double().max(dim=1).values if mode == "max" else x.double().mean(dim=1)}

    def device(dev):
        F = _F()
        return lambda x: {"out": F.vit_pool(x.to(dev), mode)}
    return Prepared(x, token_positions(x.shape), reference, device, MATH_GATES["f32"])


def prepare_vit_pool_classify(N, L, D, classes, mode):
    x = _pool_input(N, L, D)
    g = torch.Generator().manual_seed(N + L + D + classes)
    lw, lb = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, b = (torch.rand(classes, D, generator=g) * 2 - 1) / D ** 0.5, torch.randn(classes, generator=g) * 0.5

    def reference(x):
        pooled = x.double().max(dim=1).values if mode == "max" else x.double().mean(dim=1)
        return {"logits": TF.layer_norm(pooled, (D,), lw.double(), lb.double(), 1e-5) @ W.double().T + b.double()}

    def device(dev):
        F = _F()
        lwd, lbd, Wd, bd = (t.to(dev) for t in (lw, lb, W, b))
        return lambda x: {"logits": F.vit_pool_classify(x.to(dev), lwd, lbd, 1e-5, Wd, bd, mode=mode)}
    return Prepared(x, token_positions(x.shape), reference, device, MATH_GATES["f32"])


def _stem_output(N, T, V, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(N, 128, T, V, generator=g))        # the stem ends in a ReLU


def prepare_head(cls_name, setting):
    """A small head (tests/test_altformer_gpu.py::small_head) from the stem output to the logits; the reference is the same
    module's torch path in fp64 on the CPU.  ``setting``: 'per_block' | 'whole' | 'low_latency' | 'low_latency_split' | 'bf16'."""
    from test_altformer_gpu import small_head
    import copy
    head = small_head(torch.device("cpu"), cls_name)
    ref_head = copy.deepcopy(head).double()
    z = _stem_output(3, 40, 22)

    def reference(z):
        with torch.no_grad():
            return {"logits": ref_head(z.double())}

    def device(dev):
        import stgcn_amd
        from stgcn_amd.altformer import set_head_math, set_low_latency
        h = copy.deepcopy(head).to(dev).eval()
        stgcn_amd.set_hip_min_tokens(h, 0)
        if setting == "whole":
            stgcn_amd.set_whole_head(h)
        elif setting.startswith("low_latency"):
            set_low_latency(h, min_tokens=0, split_attention=setting.endswith("split"))
        elif setting == "bf16":
            set_head_math(h, "bf16")

        def run(z):
            zd = z.to(dev)
            with torch.no_grad():
                assert h.runs_whole(zd) == (setting == "whole")
                return {"logits": h(zd)}
        return run
    return Prepared(z, clip_positions(z.shape), reference, device, MATH_GATES["bf16"] if setting == "bf16" else MATH_GATES["f32"])


def prepare_model(style, setting):
    """ST_GCN_AltFormer, 3 clips at T = 20, one clip poisoned: its logits are non-finite, the others' meet the gate."""
    import copy
    import stgcn_amd
    torch.manual_seed(77)
    model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=20, num_joints=22, style=style, graph="graph.SHRE",
                                       graph_args={"labeling_mode": "spatial"}).eval()
    g = torch.Generator().manual_seed(78)
    with torch.no_grad():
        model.gcn0.PA.data = torch.randn(3, 22, 22, generator=g) * 0.05
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    from oracle import stgcn_oracle as so
    gp = so.agcn_params_from_state(model.gcn0.state_dict(), model.gcn0.A).to(torch.float64)
    tp = so.tcn_params_from_state(model.tcn0.state_dict()).to(torch.float64)
    ref_head = copy.deepcopy(model.modelA if style == "ST" else model.modelB).double()
    x = torch.randn(3, 20, 22, 3, generator=g)           # the loader's (N, T, V, C) batch

    def reference(x):                                    # the stem has no CPU path of its own: the oracle's, then the head's torch path
        with torch.no_grad():
            return {"logits": ref_head(so.stem_forward(x.permute(0, 3, 1, 2).double(), gp, tp))}

    def device(dev):
        from stgcn_amd.altformer import set_head_math, set_low_latency
        m = copy.deepcopy(model).to(dev).eval()
        stgcn_amd.set_hip_min_tokens(m, 0)
        if setting == "whole":
            stgcn_amd.set_whole_head(m)
        elif setting.startswith("low_latency"):
            set_low_latency(m, min_tokens=0, split_attention=setting.endswith("split"))
        elif setting == "bf16":
            set_head_math(m, "bf16")

        def run(x):
            with torch.no_grad():
                return {"logits": m(x.to(dev))}
        return run
    N, T, V, C = x.shape
    pos = [("first", (0, 0, 0, 0)), ("last", (N - 1, T - 1, V - 1, C - 1)), ("middle_clip", (1, T // 2, V - 1, 1))]
    return Prepared(x, pos, reference, device, MATH_GATES["bf16"] if setting == "bf16" else MATH_GATES["f32"])


# ---- training: only (a) ---------------------------------------------------------------------------------------------------------
def prepare_agcn_train(cin, cout, N, T, V, want_dx):
    """The training forward and backward of unit_agcn through the module, as test_unit_agcn_backward_vs_oracle (the moment form
    of the stem class) and test_unit_agcn_generic_backward_vs_oracle; the running buffers after the step included."""
    from oracle import stgcn_oracle as so
    from test_gpu_parity import _agcn_module_grads, _agcn_oracle_leaves
    import copy
    gcn, _, gp, _, gen = _random_stem(V, 2000 + cin + cout + T + V, cin=cin, c=cout)
    gp = gp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    names = sorted(leaves)
    x = torch.randn(N, cin, T, V, generator=gen)
    G = torch.randn(N, cout, T, V, generator=gen)

    def reference(x):
        xr = x.double().requires_grad_(True)
        aux = {}
        yr = so.agcn_forward(xr, gp, training=True, aux=aux)
        grads = torch.autograd.grad((yr * G.double()).sum(), [leaves[k] for k in names] + [xr])
        out = {"y": yr.detach(), "P": aux["P"].detach(), **{"d" + k: v for k, v in zip(names, grads[:-1])},
               "bn.running_mean": aux["bn"]["running_mean"].detach(), "bn.running_var": aux["bn"]["running_var"].detach()}
        if cin != cout:
            out["down.running_mean"], out["down.running_var"] = (aux["down_bn"][k].detach() for k in ("running_mean", "running_var"))
        if want_dx:
            out["dx"] = grads[-1]
        return out

    def device(dev):
        master = gcn.to(dev)

        def run(x):
            m = copy.deepcopy(master).train()
            m.A = master.A
            xg = x.to(dev).requires_grad_(want_dx)
            y = m(xg)
            (y * G.to(dev)).sum().backward()
            out = {"y": y.detach(), "P": m.last_attention, **{"d" + k: v for k, v in _agcn_module_grads(m).items()},
                   "bn.running_mean": m.bn.running_mean, "bn.running_var": m.bn.running_var}
            if cin != cout:
                out["down.running_mean"], out["down.running_var"] = m.down[1].running_mean, m.down[1].running_var
            if want_dx:
                out["dx"] = xg.grad
            return out
        return run
    return Prepared(x, clip_positions(x.shape), reference, device, MATH_GATES["f32"])


def prepare_tcn_train(cin, cout, K, stride, N, T, V, math):
    """Unit2D's training step through the module, as test_unit2d_backward_vs_oracle."""
    from stgcn_amd import Unit2D, set_math_mode
    from oracle import stgcn_oracle as so
    import copy
    torch.manual_seed(900 + cin + K + V)
    gen = torch.Generator().manual_seed(901 + cin + K + V)
    master = Unit2D(cin, cout, kernel_size=K, stride=stride)
    with torch.no_grad():
        master.bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        master.bn.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
        master.conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
    set_math_mode(master, math)
    tp = so.tcn_params_from_state(master.state_dict(), stride=stride).to(torch.float64)
    leaves = [tp.conv_w, tp.bn.weight, tp.bn.bias]
    for t in leaves:
        t.requires_grad_(True)
    x = torch.randn(N, cin, T, V, generator=gen)
    G = torch.randn(N, cout, _F().tcn_out_frames(T, K, stride), V, generator=gen)

    def reference(x):
        xr = x.double().requires_grad_(True)
        aux = {}
        yr = so.tcn_forward(xr, tp, training=True, aux=aux)
        g = torch.autograd.grad((yr * G.double()).sum(), leaves + [xr])
        return {"y": yr.detach(), "dW": g[0], "dgamma": g[1], "dbeta": g[2], "dx": g[3],
                "running_mean": aux["bn"]["running_mean"].detach(), "running_var": aux["bn"]["running_var"].detach()}

    def device(dev):
        def run(x):
            m = copy.deepcopy(master).to(dev).train()
            xd = x.to(dev).requires_grad_(True)
            y = m(xd)
            (y * G.to(dev)).sum().backward()
            return {"y": y.detach(), "dW": m.conv.weight.grad.reshape(cout, cin, K), "dgamma": m.bn.weight.grad, "dbeta": m.bn.bias.grad,
                    "dx": xd.grad, "running_mean": m.bn.running_mean, "running_var": m.bn.running_var}
        return run
    return Prepared(x, clip_positions(x.shape, K), reference, device, MATH_GATES[math])


def prepare_tcn_saved(cin, cout, K, stride, N, T, V, math):
    """stgcn_tcn_forward_train with save=True: the pre-BatchNorm branch z and the saved batch mean / inverse deviation the
    backward reads, and the running buffers it updates in place."""
    from oracle import stgcn_oracle as so
    g = torch.Generator().manual_seed(cin + cout + K + T + V)
    W, b = torch.randn(cout, cin, K, generator=g) * 0.05, torch.randn(cout, generator=g) * 0.1
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    x = torch.randn(N, cin, T, V, generator=g)

    def reference(x):
        z = so.temporal_conv(x.double(), W.double(), b.double(), stride)
        n = z.numel() / cout
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        invstd = torch.rsqrt(var + so.BN_EPS)
        y = torch.relu((z - mean.view(1, -1, 1, 1)) * (invstd * gamma.double()).view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1))
        return {"y": y, "z": z, "save_mean": mean, "save_invstd": invstd, "running_mean": so.BN_MOMENTUM * mean,
                "running_var": (1 - so.BN_MOMENTUM) + so.BN_MOMENTUM * var * (n / (n - 1))}

    def device(dev):
        F = _F()
        Wd, bd, gd, btd = (t.to(dev) for t in (W, b, gamma, beta))

        def run(x):
            rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
            y, z, mean, invstd = F.tcn_forward_train(x.to(dev), Wd, bd, (gd, btd, rm, rv), stride, _math(math), save=True)
            return {"y": y, "z": z, "save_mean": mean, "save_invstd": invstd, "running_mean": rm, "running_var": rv}
        return run
    return Prepared(x, clip_positions(x.shape, K), reference, device, MATH_GATES[math])


def prepare_stem_train(math):
    """loss.backward() through tcn0(gcn0(x)) in .train(), as test_stem_training_step_vs_oracle."""
    from stgcn_amd import set_math_mode
    from oracle import stgcn_oracle as so
    from test_gpu_parity import _agcn_module_grads, _agcn_oracle_leaves
    import copy
    gcn, tcn, gp, tp, gen = _random_stem(22, 1200)
    set_math_mode(tcn, math)
    gp, tp = gp.to(torch.float64), tp.to(torch.float64)
    leaves = _agcn_oracle_leaves(gp)
    tleaves = {"t_w": tp.conv_w, "t_bn_w": tp.bn.weight, "t_bn_b": tp.bn.bias}
    for t in tleaves.values():
        t.requires_grad_(True)
    leaves.update(tleaves)
    names = sorted(leaves)
    x = torch.randn(3, 3, 20, 22, generator=gen)
    G = torch.randn(3, 128, 20, 22, generator=gen)

    def reference(x):
        aux = {}
        zr = so.tcn_forward(so.agcn_forward(x.double(), gp, training=True), tp, training=True, aux=aux)
        grads = torch.autograd.grad((zr * G.double()).sum(), [leaves[k] for k in names])
        return {"z": zr.detach(), **{"d" + k: v for k, v in zip(names, grads)}, "tcn.running_mean": aux["bn"]["running_mean"].detach(),
                "tcn.running_var": aux["bn"]["running_var"].detach()}

    def device(dev):
        gm, tm = gcn.to(dev), tcn.to(dev)

        def run(x):
            g2, t2 = copy.deepcopy(gm).train(), copy.deepcopy(tm).train()
            g2.A = gm.A
            z = t2(g2(x.to(dev)))
            (z * G.to(dev)).sum().backward()
            got = {"d" + k: v for k, v in _agcn_module_grads(g2).items()}
            got.update({"dt_w": t2.conv.weight.grad.flatten(1).reshape(128, 128, 9), "dt_bn_w": t2.bn.weight.grad, "dt_bn_b": t2.bn.bias.grad})
            return {"z": z.detach(), **got, "tcn.running_mean": t2.bn.running_mean, "tcn.running_var": t2.bn.running_var}
        return run
    return Prepared(x, clip_positions(x.shape), reference, device, MATH_GATES[math])


def prepare_st_attention_train(N, cin, cout, T, V):
    """gcn_unit_attention's training step without drop-connect, through the module."""
    sd = R.make_state(cin, cout, V, 11)
    x = R.make_input(N, cin, T, V, 12)
    dy = torch.randn(N, cout, T, V, generator=torch.Generator().manual_seed(13))

    def reference(x):
        yr, new, g, dx = R.grads64(sd, x, dy, training=True, mask=None)
        return {"y": yr, "dx": dx, **{"d" + k: v for k, v in g.items()}, **new}

    def device(dev):
        m = _st_unit(cin, cout, V, sd, drop_connect=False).train()

        def run(x):
            m.load_state_dict(sd)                   # the running statistics of the previous plant
            for p in m.parameters():
                p.grad = None
            xg = x.to(dev).requires_grad_(True)
            y = m(xg)
            y.backward(dy.to(dev))
            return {"y": y.detach(), "dx": xg.grad, **{"d" + k: p.grad for k, p in m.named_parameters()},
                    **{k: v.clone() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}}
        return run
    return Prepared(x, clip_positions(x.shape), reference, device, MATH_GATES["f32"])


def prepare_vit_block_train(B, L, D, mode, attention_bf16=False):
    """One block's training forward and backward (vit_block_forward_train / vit_block_backward) against autograd through
    altformer_train_ref.block64."""
    heads, hidden = ar.HEADS, 2 * D
    x, sd = _block_inputs(B, L, D, hidden)
    dy = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L + D))

    def reference(x):
        y, g = tr.grads64(x, sd, dy, scale=(D // heads) ** -0.5)
        return {"y": y, **{"d" + k: v for k, v in g.items()}}

    def device(dev):
        from stgcn_amd import _capi
        from stgcn_amd.altformer import HEAD_TRAIN_MATH
        F = _F()
        ps = [sd[k].to(dev) for k in tr.PARAMS]
        math = HEAD_TRAIN_MATH[mode] | (_capi.VIT_TRAIN_ATTN_BF16 if attention_bf16 else 0)
        args = (heads, ar.EPS, (D // heads) ** -0.5, math)

        def run(x):
            xd = x.to(dev)
            y, saved = F.vit_block_forward_train(xd, ps, *args)
            g = F.vit_block_backward(xd, ps, saved, dy.to(dev), *args)
            return {"y": y, "dx": g["x"], **{"d" + k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS)}}
        return run
    return Prepared(x, token_positions(x.shape), reference, device, MATH_GATES["bf16" if mode == "bf16" or attention_bf16 else "f32"])


# ---- the rows of the table ------------------------------------------------------------------------------------------------------
def _build_table():
    from test_buffer_discipline_gpu import AGCN_SHAPES, STEM_MATHS, STEM_SHAPES, TCN_SHAPES, _stem_kernel
    F = _F()
    for s in AGCN_SHAPES + [(2, 16, 32, 5, 7)]:      # the last: the only one on agcn_expand_generic_kernel
        s = two_clips(s)
        add("agcn-" + "x".join(map(str, s)), "f32", prepare_agcn, *s)
    for ci, co, K, st, T, V, N, m, ob, av in TCN_SHAPES:
        eff, kernel = tcn_case_math(ci, co, K, st, T, V, m, av)
        add(f"tcn-{ci}x{co}x{K}x{st}x{T}x{V}x{N}-{m}" + ("-bf16out" if ob else "") + ("-alongV" if av else ""), eff, prepare_tcn,
            ci, co, K, st, T, V, N, m, ob, av, kernel=kernel)
    for s in STEM_SHAPES:
        for m in STEM_MATHS:
            if F.stem_supported(3, s[3], s[1], s[2], 9, 3, _math(m)):
                add("stem_fused-" + "x".join(map(str, two_clips(s))) + "-" + m, m, prepare_stem_fused, two_clips(s), m,
                    kernel=_stem_kernel(s, m))
    for s in [(3, 37, 22, 128), (2, 9, 46, 128), (2, 30, 64, 128)]:
        for m in ("f32", "bf16x3", "bf16"):
            add("stem_two_stage-" + "x".join(map(str, s)) + "-" + m, m, prepare_stem_two_stage, s, m)
    for o in ("ST", "TS"):
        for lay in ("nctv", "ntvc"):
            add(f"patch_embed-{o}-{lay}", "f32", prepare_patch_embed, o, lay)
    for s in [(2, 131, 128, 12, 22), (2, 256, 512, 3, 46)]:
        add("st_attention-" + "x".join(map(str, s)), "f32", prepare_st_attention, *s)
    for (M, K, Nout), m in [((129, 96, 100), "f32"), ((129, 96, 100), "bf16x3"), ((33, 256, 200), "bf16x3")]:
        add(f"vit_linear-{M}x{K}x{Nout}-{m}", m, prepare_vit_linear, M, K, Nout, m)
    for form, B, L, hd in [("resident", 3, 33, 32), ("resident", 3, 65, 64), ("resident", 2, 180, 32), ("stream", 2, 257, 32),
                           ("split", 2, 33, 32), ("split", 2, 180, 64)]:
        add(f"vit_attention-{form}-{B}x{L}-hd{hd}", "f32", prepare_vit_attention, form, B, L, hd)
    for mode in ("f32", "mixed", "bf16"):
        add(f"vit_block-3x33x256-{mode}", mode, prepare_vit_block, 3, 33, 256, 8, 512, mode)
    for mode in ("mean", "max"):
        lost = ("-inf",) if mode == "max" else ()      # a maximum over tokens drops one -inf in the reference too: nothing to keep
        for S, L, D in [(3, 33, 256), (2, 180, 64)]:
            add(f"vit_pool-{S}x{L}x{D}-{mode}", "f32", prepare_vit_pool, S, L, D, mode, without=lost)
        add(f"vit_pool_classify-3x65x256x14-{mode}", "f32", prepare_vit_pool_classify, 3, 65, 256, 14, mode, without=lost)
    for cls_name in ("ST", "TS"):
        add(f"head-{cls_name}-whole", "mixed", prepare_head, cls_name, "whole")
    for style in ("ST", "TS"):
        for setting in ("per_block", "whole", "low_latency", "low_latency_split", "bf16"):
            add(f"model-{style}-{setting}", "bf16" if setting == "bf16" else "mixed", prepare_model, style, setting)
    # training: only (a)
    add("agcn_train-moment_form-3x128-3x20x22", "f32", prepare_agcn_train, 3, 128, 3, 20, 22, False, training=True)
    add("agcn_train-generic-64x64-2x12x22-dx", "f32", prepare_agcn_train, 64, 64, 2, 12, 22, True, training=True)
    for (ci, co, K, st, N, T, V), m in [((64, 128, 9, 1, 2, 21, 22), "bf16x3"), ((64, 128, 9, 2, 2, 21, 22), "bf16x3"),
                                        ((32, 64, 2, 1, 2, 7, 22), "bf16x3"), ((32, 64, 9, 1, 2, 7, 22), "f32_valu")]:
        add(f"tcn_train-{ci}x{co}x{K}x{st}x{N}x{T}x{V}-{m}", m, prepare_tcn_train, ci, co, K, st, N, T, V, m, training=True)
    for m in ("bf16x3", "f32_valu"):
        add(f"tcn_saved-64x128x9x1x2x21x22-{m}", m, prepare_tcn_saved, 64, 128, 9, 1, 2, 21, 22, m, training=True)
    add("stem_train-bf16x3", "bf16x3", prepare_stem_train, "bf16x3", training=True)
    add("st_attention_train-2x131x128x12x22", "f32", prepare_st_attention_train, 2, 131, 128, 12, 22, training=True)
    for mode in ("f32", "bf16x3", "bf16"):
        add(f"vit_block_train-3x33x256-{mode}", mode, prepare_vit_block_train, 3, 33, 256, mode, training=True)
    add("vit_block_train-3x33x256-f32-attention_bf16", "f32", prepare_vit_block_train, 3, 33, 256, "f32", True, training=True)
    add("vit_block_train-2x257x256-f32-streaming", "f32", prepare_vit_block_train, 2, 257, 256, "f32", training=True)


_build_table()
assert len({c.id for c in CASES}) == len(CASES)
