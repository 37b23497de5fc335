"""ST-TR's attention unit decides in one plan (csrc/st_attention.hip, ``plan_st_attention``) and refuses before any launch.

* The six host queries against tests/golden/st_attention_dispatch.json, which the library of the commit before the plan wrote
  (tests/golden/make_st_attention_dispatch.py describes the grid): no answer moved.
* A call past the columns its arithmetic's product kernel covers - T = 65536 (TV = 65535*64 + 64) in f32, T = 131073
  (TV = 65535*128 + 192) in bf16x3, at V = 64 - answers STGCN_ERR_UNSUPPORTED from every entry point.  STGCN_ERR_HIP would
  mean that a launch was reached: the library before the plan got as far as the first product, the training forward with
  data_bn's running statistics already updated.
  Without a GPU the pointers are made-up addresses (a refused call reads none); with one they are real buffers of the sizes
  the header and the size query give.  The largest covered T gets past the plan: STGCN_ERR_HIP without a GPU, STGCN_OK with one.
* GPU: the functional training forward at the f32 shape raises, and the running statistics, y and the saved tensors hold
  what they held before.
"""
import ctypes
import json
import os

import pytest
import torch

from _util import GOLDEN, hostile_allocations

OK, UNSUPPORTED, HIP = 0, -2, -4
F32, BF16X3 = 0, 1
BASE = 0x7F0000001000                      # 4096-byte aligned, never dereferenced
SHAPE = dict(N=1, Cin=1, Cout=16, dk=4, V=64, heads=1)
# arithmetic -> (largest covered T, first refused T) at V = 64: the column tiles of the product ride on a 16-bit grid axis
EDGE = {F32: (65535, 65536), BF16X3: (131070, 131073)}      # 65535*64 / 64, 65535*128 / 64


def _lib():
    from stgcn_amd import _capi
    return _capi.lib()


def _fixture():
    with open(os.path.join(GOLDEN, "st_attention_dispatch.json")) as fh:
        return json.load(fh)


# ---- the queries ---------------------------------------------------------------------------------------------------------------------
def test_unit_queries_match_the_parent():
    fx, lib = _fixture(), _lib()
    maths = list(fx["maths"].values())
    bad = []
    for row in fx["unit"]:
        shape, want = row[:5], row[5:]
        got = [lib.stgcn_st_attention_supported(*shape)] + [lib.stgcn_st_attention_math_supported(*shape, m) for m in maths]
        if got != want:
            bad.append(f"{shape}: want {want} got {got}")
    assert len(fx["unit"]) >= 650 and {r[0] for r in fx["unit"]} >= set(range(1, 261)) and {r[3] for r in fx["unit"]} >= set(range(1, 71))
    assert not bad, f"{len(bad)} of {len(fx['unit'])} rows differ:\n" + "\n".join(bad[:20])


def test_workspace_sizes_match_the_parent():
    fx, lib = _fixture(), _lib()
    bad = []
    for row in fx["ws"]:
        shape, want = row[:7], row[7:]
        passes = (0, 1, 2) if want[2] is not None else (-1, 3)
        got = [lib.stgcn_st_attention_ws_bytes(*shape, p) for p in passes]
        if got != want[:len(passes)]:
            bad.append(f"{shape}: want {want} got {got}")
    assert len(fx["ws"]) >= 220
    assert not bad, f"{len(bad)} of {len(fx['ws'])} rows differ:\n" + "\n".join(bad[:20])


def test_product_queries_match_the_parent():
    fx, lib = _fixture(), _lib()
    maths = list(fx["maths"].values())
    bad = []
    for row in fx["product"]:
        (M, K, TV), want = row[:3], row[3:]
        got = []
        for m in maths:
            got += [lib.stgcn_wx_product_supported(M, K, TV, m), fx["kernels"].index(lib.stgcn_wx_product_kernel_name(M, K, TV, m).decode()),
                    lib.stgcn_wx_product_ws_bytes(M, K, m)]
        if got != want:
            bad.append(f"{(M, K, TV)}: want {want} got {got}")
    tvs = {r[2] for r in fx["product"]}
    assert {65535 * 64, 65535 * 64 + 1, 65535 * 128, 65535 * 128 + 1} <= tvs, "both column limits, from both sides"
    assert not bad, f"{len(bad)} of {len(fx['product'])} rows differ:\n" + "\n".join(bad[:20])


# ---- refusal before the first launch -------------------------------------------------------------------------------------------------
def _operand_floats(entry, T):
    """Element counts of the pointer operands of ``entry`` in the order of its arguments ("ws": the size query's bytes)."""
    N, Cin, Cout, dk, V, H = (SHAPE[k] for k in ("N", "Cin", "Cout", "dk", "V", "heads"))
    Cq, CV, TV = 2 * dk + Cout, Cin * V, T * V
    a = lambda C: N * C * TV                                                                      # noqa: E731
    weights = [Cq * Cin, Cq, Cout * Cout, Cout]                                                   # Wqkv, bqkv, Wout, bout
    saved = [a(Cq), a(Cout), a(Cout), 4 * N * T * H * V, 2 * CV + 2 * Cout]                       # qkv, o, z, rowstats, stats
    if entry == "stgcn_st_attention_forward_math":
        return [a(Cin), CV, CV] + weights + [Cout, Cout, "ws", a(Cout)]
    if entry == "stgcn_st_attention_forward_train":
        return [a(Cin)] + [CV] * 4 + weights + [Cout] * 4 + [N * T * H * V, "ws", a(Cout)] + saved
    assert entry == "stgcn_st_attention_backward"
    return [a(Cin), CV, CV, Cq * Cin, Cout * Cout, Cout, Cout, N * T * H * V] + saved + \
           [a(Cout), a(Cin), CV, CV, Cq * Cin, Cq, Cout * Cout, Cout, Cout, Cout, "ws"]


PASS = {"stgcn_st_attention_forward_math": 0, "stgcn_st_attention_forward_train": 1, "stgcn_st_attention_backward": 2}


def _call(entry, T, math):
    """The status of ``entry`` at SHAPE with T frames, and what it kept alive (real buffers where a GPU is visible)."""
    from stgcn_amd import _capi
    lib = _lib()
    _, argtypes = _capi.PROTOTYPES[entry]
    dims = [SHAPE["N"], SHAPE["Cin"], SHAPE["Cout"], SHAPE["dk"], T, SHAPE["V"], SHAPE["heads"]]
    ws_bytes = lib.stgcn_st_attention_ws_bytes(*dims, PASS[entry])
    assert ws_bytes > 0
    gpu = torch.cuda.is_available()
    sizes = _operand_floats(entry, T)
    assert len(sizes) == sum(t is ctypes.c_void_p for t in argtypes) - 1, "one size per pointer operand but the stream"
    keep, args, ints, ptrs = [], [], iter(dims), iter(sizes)
    for i, t in enumerate(argtypes):
        if t is ctypes.c_void_p and i == len(argtypes) - 1:
            args.append(ctypes.c_void_p(None))                                                    # the stream
        elif t is ctypes.c_void_p:
            n = next(ptrs)
            if gpu:
                keep.append(torch.zeros((ws_bytes + 7) // 8, dtype=torch.float64, device="cuda") if n == "ws" else
                            torch.zeros(n, dtype=torch.float32, device="cuda"))
                assert keep[-1].data_ptr() % 256 == 0
            args.append(ctypes.c_void_p(keep[-1].data_ptr() if gpu else BASE + 4096 * i))
        elif t is ctypes.c_size_t:
            args.append(ctypes.c_size_t(ws_bytes))
        elif t is ctypes.c_float:
            args.append(ctypes.c_float(0.1))
        elif t is ctypes.c_uint:
            args.append(ctypes.c_uint(math))
        else:
            args.append(t(next(ints)))
    rc = getattr(lib, entry)(*args)
    msg = lib.stgcn_last_error().decode() if rc else ""
    if gpu:
        torch.cuda.synchronize()
    return rc, msg, keep


@pytest.mark.parametrize("math", [F32, BF16X3], ids=["f32", "bf16x3"])
@pytest.mark.parametrize("entry", sorted(PASS, key=PASS.get))
def test_a_call_past_its_products_columns_is_refused_before_any_launch(entry, math):
    lib = _lib()
    q = (SHAPE["Cin"], SHAPE["Cout"], SHAPE["dk"], SHAPE["V"], SHAPE["heads"])
    assert lib.stgcn_st_attention_supported(*q) == 1 and lib.stgcn_st_attention_math_supported(*q, math) == 1
    last, over = EDGE[math]
    rc, msg, keep = _call(entry, over, math)
    print(entry, "T =", over, "->", rc, msg)
    assert rc == UNSUPPORTED, f"T={over}: status {rc} ({msg}); STGCN_ERR_HIP means that a launch was reached"
    for t in keep:
        assert not bool(t.count_nonzero()), "a refused call wrote to one of its operands"
    del keep
    rc, msg, keep = _call(entry, last, math)
    print(entry, "T =", last, "->", rc, msg)
    assert rc == (OK if torch.cuda.is_available() else HIP), f"T={last} is covered: status {rc} ({msg})"


@pytest.mark.gpu
def test_refused_training_forward_leaves_the_running_statistics_alone():
    """F.st_attention_forward_train, batch statistics, f32, T = 65536 at V = 64: STGCN_ERR_UNSUPPORTED, and data_bn's and bn's
    running statistics, y and every saved tensor (allocated poisoned by the call) hold what they held before."""
    from stgcn_amd import functional as F
    from stgcn_amd._capi import StgcnError
    dev = torch.device("cuda:0")
    N, Cin, Cout, dk, V, H = (SHAPE[k] for k in ("N", "Cin", "Cout", "dk", "V", "heads"))
    T = EDGE[F32][1]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, Cin, T, V, generator=g).to(dev)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)                                         # noqa: E731
    data_bn = [rnd(Cin * V), rnd(Cin * V), rnd(Cin * V), torch.rand(Cin * V, generator=g).to(dev) + 0.5]
    bn = [rnd(Cout), rnd(Cout), rnd(Cout), torch.rand(Cout, generator=g).to(dev) + 0.5]
    before = [t.clone() for t in data_bn[2:] + bn[2:]]
    Wqkv, bqkv, Wout, bout = rnd(2 * dk + Cout, Cin), rnd(2 * dk + Cout), rnd(Cout, Cout), rnd(Cout)
    with hostile_allocations(0xFF) as h:
        with pytest.raises(StgcnError, match="STGCN_ERR_UNSUPPORTED") as e:
            F.st_attention_forward_train(x, data_bn, Wqkv, bqkv, Wout, bout, bn, None, dk, H, frozen=False, math=F.MATH_F32)
        torch.cuda.synchronize()
        h.check()
        assert e.value.code == UNSUPPORTED
        assert len(h.records) >= 7, "the workspace, y and the five saved tensors"
        for i, (raw, nbytes, shape, dtype) in enumerate(h.records):
            assert bool((raw == h.fill).all()), f"allocation #{i} (shape {shape}, {dtype}) was written by the refused call"
    for name, was, now in zip(("data_bn.running_mean", "data_bn.running_var", "bn.running_mean", "bn.running_var"), before,
                              data_bn[2:] + bn[2:]):
        assert torch.equal(was, now), f"{name} was updated by a refused call"
