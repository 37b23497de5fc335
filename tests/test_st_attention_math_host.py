"""Host side of the 'bf16x3' arithmetic of gcn_unit_attention (tests/test_st_attention_math_gpu.py runs it).  No GPU.

The ABI additions (declared, bound, exported; the two ``*_supported`` truth tables; kernel names), the Python setting
(default, setter, env, DataParallel replica), and the reference-only conditions: the inputs of the GPU tests are such that
the arithmetic ITSELF - emulated in fp64 sums, or restated with fp32 sums on the CPU - holds the GPU tests' gates with room, so
that a GPU failure points at the kernel."""
import os
import re
import subprocess
import sys

import pytest
import torch

import st_attention_math_ref as MR
import st_attention_ref as R
from _util import ZERO_GRAD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("stgcn_st_attention_math_supported", "stgcn_st_attention_forward_math", "stgcn_wx_product_supported",
       "stgcn_wx_product_kernel_name", "stgcn_wx_product_ws_bytes", "stgcn_wx_product")
QUARTER_GATE = 2.5e-5
F32, BF16X3, BF16, F32_VALU = 0, 1, 2, 3


def _lib():
    from stgcn_amd import _capi
    return _capi.lib()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from stgcn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    assert "#define STGCN_ABI_VERSION 11" in hdr and _capi.ABI_VERSION == 11
    handle = _lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in stgcn_hip.h"
        assert name in _capi.PROTOTYPES, f"{name} has no prototype in _capi.PROTOTYPES"
        fn = getattr(handle, name)
        assert fn.argtypes == _capi.PROTOTYPES[name][1] and fn.restype == _capi.PROTOTYPES[name][0]
    assert len(_capi.PROTOTYPES["stgcn_st_attention_forward_math"][1]) == len(_capi.PROTOTYPES["stgcn_st_attention_forward"][1]) + 1
    assert len(_capi.PROTOTYPES["stgcn_wx_product"][1]) == 14
    assert handle.stgcn_version() == 11
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("stgcn_st_attention_forward_math", "stgcn_st_attention_math_supported", "stgcn_wx_product"):
        assert name in table


COVERED = [(c["cin"], c["cout"], c["cout"] // 4, c["V"], c["nh"]) for c in R.EDGE_CASES] + \
          [(c["cin"], c["cout"], c["cout"] // 4, c["V"], R.NH) for c in MR.UNIT_CASES] + [(16, 128, 32, 9, 4), (16, 64, 16, 9, 4)]
REFUSED = [(16, 128, 32, 65, 8), (16, 64, 16, 9, 8), (16, 192, 48, 9, 8), (16, 128, 32, 0, 8), (0, 128, 32, 9, 8)]


def test_unit_supported_table_follows_the_f32_query_for_both_arithmetics():
    h = _lib()
    for shape in COVERED + REFUSED:
        base = h.stgcn_st_attention_supported(*shape)
        assert base == (1 if shape in COVERED else 0), shape
        for math in (F32, BF16X3, BF16X3 | 0x200):
            assert h.stgcn_st_attention_math_supported(*shape, math) == base, (shape, math)
        for math in (BF16, F32_VALU, 7):
            assert h.stgcn_st_attention_math_supported(*shape, math) == 0, (shape, math)


def test_product_supported_table_and_kernel_names():
    h = _lib()
    shapes = [(c["M"], c["K"], c["TV"]) for c in MR.PRODUCT_CASES] + [(1, 1, 1), (768, 512, 13800), (131, 768, 3450)]
    names = {}
    for M, K, TV in shapes:
        for math in (F32, BF16X3):
            assert h.stgcn_wx_product_supported(M, K, TV, math) == 1, (M, K, TV, math)
            name = h.stgcn_wx_product_kernel_name(M, K, TV, math).decode()
            assert name, (M, K, TV, math)
            names.setdefault(math, set()).add(name)
            assert h.stgcn_wx_product_kernel_name(M, K, TV, math).decode() == name          # stable
        for math in (BF16, F32_VALU, 7):
            assert h.stgcn_wx_product_supported(M, K, TV, math) == 0
            assert h.stgcn_wx_product_kernel_name(M, K, TV, math) == b""
        assert h.stgcn_wx_product_ws_bytes(M, K, BF16X3) <= 1 << 30
    assert not names[F32] & names[BF16X3], "the two arithmetics name the same kernel"
    for bad in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, 4, 1 << 40)]:
        for math in (F32, BF16X3):
            assert h.stgcn_wx_product_supported(*bad, math) == 0
            assert h.stgcn_wx_product_kernel_name(*bad, math) == b""
    # the half-height tile serves the M whose last 128-row tile would be less than half full
    assert h.stgcn_wx_product_kernel_name(192, 64, 3450, BF16X3) == h.stgcn_wx_product_kernel_name(131, 64, 3450, BF16X3)
    assert h.stgcn_wx_product_kernel_name(192, 64, 3450, BF16X3) != h.stgcn_wx_product_kernel_name(256, 64, 3450, BF16X3)


# ---- the Python setting ---------------------------------------------------------------------------------------------------------------
def _stack():
    import torch.nn as nn
    from stgcn_amd import Unit2D, gcn_unit_attention
    A = torch.zeros(3, 9, 9)
    return nn.Sequential(gcn_unit_attention(8, 128, A, **R.unit_kwargs(9)), Unit2D(128, 128, kernel_size=9),
                         nn.Sequential(gcn_unit_attention(128, 128, A, **R.unit_kwargs(9))))


def test_setter_default_reach_and_refusals():
    import stgcn_amd
    from stgcn_amd import Unit2D, gcn_unit_attention, set_math_mode, set_st_attention_math
    assert "set_st_attention_math" in stgcn_amd.__all__
    net = _stack()
    units = [m for m in net.modules() if isinstance(m, gcn_unit_attention)]
    tcn = next(m for m in net.modules() if isinstance(m, Unit2D))
    assert len(units) == 2 and all(u.math_mode == "f32" for u in units)
    tcn_mode = tcn.math_mode
    others = {id(m): dict(m.__dict__) for m in net.modules() if not isinstance(m, gcn_unit_attention)}
    set_st_attention_math(net, "bf16x3")
    assert all(u.math_mode == "bf16x3" for u in units)
    assert tcn.math_mode == tcn_mode
    for m in net.modules():
        if not isinstance(m, gcn_unit_attention):
            assert m.__dict__.keys() == others[id(m)].keys(), f"{type(m).__name__} gained an attribute"
    for bad in ("bf16", "f32_valu", "BF16X4", None, 1):
        with pytest.raises(ValueError, match="'f32' or 'bf16x3'"):
            set_st_attention_math(net, bad)
    assert all(u.math_mode == "bf16x3" for u in units)
    for mode in ("f32", "bf16x3", "bf16", "f32_valu"):                 # set_math_mode leaves the units alone
        set_math_mode(net, mode)
        assert all(u.math_mode == "bf16x3" for u in units)
    set_st_attention_math(net, "f32")
    assert all(u.math_mode == "f32" for u in units)
    assert "gcn_unit_attention" in set_math_mode.__doc__


def test_replica_reports_its_masters_setting():
    from stgcn_amd import gcn_unit_attention, set_st_attention_math
    u = gcn_unit_attention(8, 128, torch.zeros(3, 9, 9), **R.unit_kwargs(9))
    rep = u._replicate_for_data_parallel()
    assert rep.math_mode == "f32"
    set_st_attention_math(u, "bf16x3")
    assert rep.math_mode == "bf16x3" and rep._math_flags == 1          # read from the master, not copied at replication
    assert u._replicate_for_data_parallel().math_mode == "bf16x3"


@pytest.mark.parametrize("value,expect", [("BF16X3", "bf16x3"), (None, "f32"), ("bf16", "error")])
def test_env_sets_the_default_of_new_units(value, expect):
    code = (f"import sys; sys.path[:0] = {[os.path.join(ROOT, 'st-gcn-altformer_amd'), HERE]!r}\n"
            "import torch, st_attention_ref as R\n"
            "from stgcn_amd import gcn_unit_attention\n"
            "try:\n"
            "    print('MODE', gcn_unit_attention(8, 128, torch.zeros(3, 9, 9), **R.unit_kwargs(9)).math_mode)\n"
            "except ValueError as e:\n"
            "    print('MODE error', e)\n")
    env = {k: v for k, v in os.environ.items() if k != "STGCN_ST_ATTENTION_MATH"}
    if value is not None:
        env["STGCN_ST_ATTENTION_MATH"] = value
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert done.returncode == 0, done.stderr
    line = next(ln for ln in done.stdout.splitlines() if ln.startswith("MODE"))
    assert line.split()[1] == expect, line
    if expect == "error":
        assert "'f32' or 'bf16x3'" in line


# ---- reference-only conditions -----------------------------------------------------------------------------------------------------------
def _ratio(a, ref):
    return float((a.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


@pytest.mark.parametrize("name", [c["name"] for c in MR.UNIT_CASES])
def test_emulation_of_the_unit_is_within_a_quarter_of_the_gate(name):
    """y, dx and every parameter gradient of the three-term emulation lie within 2.5e-5 of max|fp64|, on the inputs and the
    cotangent the GPU test uses; y also holds the mixed allclose criterion of parity_gate."""
    from _util import parity_gate
    c, sd, x, dy, mask, (y, _, g, dx) = MR.unit_reference(name)
    training = c["mode"] == "train"
    ye, _, ge, dxe = MR.grads_emulated(sd, x, dy, training=training, mask=mask)
    fig = {"y": _ratio(ye, y), "dx": _ratio(dxe, dx)}
    for k in g:
        if not (k in ZERO_GRAD and training):
            fig[k] = _ratio(ge[k], g[k])
    worst = max(fig, key=fig.get)
    print(f"{name}: emulation y {fig['y']:.2e} dx {fig['dx']:.2e} worst {worst} {fig[worst]:.2e}")
    for k, v in fig.items():
        assert v <= QUARTER_GATE, f"{name}: the emulation of {k} is {v:.2e} of max|fp64| (> {QUARTER_GATE:g})"
    parity_gate(ye, y, what=f"{name} emulated y")


def test_emulation_of_the_frozen_case_is_within_a_quarter_of_the_gate():
    """``frozen_mask`` with its kink-free cotangent (st_attention_math_ref.frozen_reference says why)."""
    c, sd, x, dy, mask, (y, _, g, dx) = MR.frozen_reference()
    ye, _, ge, dxe = MR.grads_emulated(sd, x, dy, training=False, mask=mask)
    fig = {"y": _ratio(ye, y), "dx": _ratio(dxe, dx), **{k: _ratio(ge[k], g[k]) for k in g}}
    worst = max(fig, key=fig.get)
    print(f"frozen_mask: emulation y {fig['y']:.2e} dx {fig['dx']:.2e} worst {worst} {fig[worst]:.2e}")
    assert len(g) == 8 and float(dy.abs().max()) > 0
    for k, v in fig.items():
        assert v <= QUARTER_GATE, f"frozen_mask: the emulation of {k} is {v:.2e} of max|fp64| (> {QUARTER_GATE:g})"


@pytest.mark.parametrize("name", [c["name"] for c in MR.PRODUCT_CASES])
def test_cpu_restatement_of_the_product_holds_bound_and_separation(name):
    """Three-term arithmetic with fp32 sums on the CPU, in two summation orders: within the elementwise bound of emu3 and at
    least 4 x closer (rms) to emu3 than to the exact product; an exact-fp32 product gives the reverse."""
    ref = MR.product_reference(name)
    for order in (0, 1):
        C = MR.three_term_fp32(ref["Wmk"], ref["X"], order)
        for add in (None if ref["bias"] is None else ref["bias"].view(1, -1, 1), ref["R"]):
            if add is not None:
                C = C + add
        excess = float(((C.double() - ref["emu3"]).abs() - ref["bound"]).max())
        near, far = MR.rms(C.double() - ref["emu3"]), MR.rms(C.double() - ref["exact64"])
        print(f"{name} order {order}: rms to emu3 {near:.2e}, to exact {far:.2e} ({far / max(near, 1e-300):.0f} x)")
        assert excess <= 0, f"{name} order {order}: {excess:.2e} over the elementwise bound"
        assert near <= far / 4
    C32 = ref["Wmk"] @ ref["X"]
    for add in (None if ref["bias"] is None else ref["bias"].view(1, -1, 1), ref["R"]):
        if add is not None:
            C32 = C32 + add
    near, far = MR.rms(C32.double() - ref["exact64"]), MR.rms(C32.double() - ref["emu3"])
    print(f"{name} exact fp32: rms to exact {near:.2e}, to emu3 {far:.2e} ({far / max(near, 1e-300):.0f} x)")
    assert near <= far / 4
