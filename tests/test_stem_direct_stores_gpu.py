"""The fused stem's narrow three-term kernel stores (N,C,T,V) results straight from its accumulators: with the operands of its
consumer MFMAs exchanged a lane holds four consecutive pixels of one channel, and the tile tail has no staging pass (csrc/kf6.h,
``PIXROWS``; csrc/kf6_tile.h).  (N,T,V,C) results still leave through the staged epilogue of the instantiation with the operands
in their old order.  So every shape is held to

* the CPU oracle in float64 at the gate of the other bf16x3 stem tests (1e-4 of max|ref|, ``MATH_GATES`` / ``parity_gate``), and
* the same call with a channels-last result, permuted, BIT FOR BIT: each element is the same sum of the same products in the
  same order in both kernels, so the new epilogue is held to the old one without a recorded digest.

Results are written into NaN-filled tensors between NaN-filled guard bands (``_util.skewed``): an element that no store reaches
stays NaN, a store outside the tensor breaks a guard.  The shapes visit the three forms of the tail (straight-line 16-byte
stores; element by element under bounds checks; the short tile's whole groups under a lane's predicate), both producer block
counts, two channel groups and a walk in which a workgroup crosses a clip boundary.  Two shapes of the list are served by
stem_bf16_v4_kernel (V = 25 and C = 256 at V = 22 do not fit KF6's LDS budget): they are held to the same conditions, and
(2, 37, 24, 128) / (2, 24, 20, 256) put the eight-block producer and two channel groups on this kernel."""
import ctypes
import functools

import pytest
import torch

import entry_points as ep
from _util import MATH_GATES, parity_gate, skewed

V6, V4 = "stem_bf16_v6_kernel", "stem_bf16_v4_kernel"
# (N, T, V, C): what it exercises, the kernel the plan names
SHAPES = [
    ((3, 24, 22, 128), V6),     # two full tiles plus a 16-pixel SHORT tile, aligned rows
    ((3, 20, 22, 128), V6),     # last tile of 184 pixels: the bounds-checked four-block form
    ((2, 25, 22, 128), V6),     # T V = 550, not a multiple of 4: the element form on every tile, SHORT included
    ((2, 35, 22, 128), V6),     # T V = 770: rows off 16 bytes with a partial last tile
    ((2, 24, 16, 128), V6),     # one joint half of the feature phase; a short tile of exactly 128 pixels
    ((2, 24, 25, 128), V4),     # two joint halves (this one: the older kernel)
    ((2, 37, 24, 128), V6),     # two joint halves, eight producer blocks per wave and chunk, a short tile of 120 pixels
    ((2, 24, 22, 256), V4),     # two channel groups (this one: the older kernel)
    ((2, 24, 20, 256), V6),     # two channel groups on this kernel: the second reads shift[128 ..]
]
BF16_SHAPES = [(3, 24, 22, 128), (2, 25, 22, 128)]
WALK_T, WALK_V = 24, 22


def _ids(rows):
    return ["x".join(map(str, r[0] if isinstance(r[0], tuple) else r)) for r in rows]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _setup(shape):
    """Seeded stem of a shape, its input and the float64 oracle's result: made once per shape, never modified."""
    s = ep.stem(*shape)
    return s, s.reference(s.x)["out"]


@functools.lru_cache(maxsize=None)
def _staged(shape, dev):
    s, _ = _setup(shape)
    staged = s.on(dev)
    return staged, staged.prepare(ep.math_flag("bf16x3"))


def _run(shape, dev, x=None, bf16=False, channels_last=False, skew=0):
    """F.stem_forward in bf16x3 into a NaN-filled tensor ``skew`` elements behind a 256-byte boundary; returns it shaped (N,C,T,V)."""
    s, _ = _setup(shape)
    staged, prep = _staged(shape, dev)
    x = (s.x if x is None else x).to(dev)
    N, C = x.shape[0], shape[3]
    T, V = shape[1], shape[2]
    dtype = torch.bfloat16 if bf16 else torch.float32
    target = skewed(torch.zeros((N, T, V, C) if channels_last else (N, C, T, V), device=dev, dtype=dtype), skew)
    target.fill_(float("nan"))
    st, ts = staged.st, staged.ts
    out, _ = ep.hipF().stem_forward(x, st["A_eff"], st["Wa"], st["ba"], st["Wb"], st["bb"], prep, ts["shift"], C, 9,
                                    ep.math_flag("bf16x3"), bf16, out=target, channels_last_out=channels_last)
    torch.cuda.synchronize()
    target.check()
    assert out.data_ptr() == target.data_ptr() and tuple(out.shape) == (N, C, T, V)
    assert not torch.isnan(out).any(), f"{shape}: elements that no store reached"
    return out


def _walk_crosses_a_clip(N, T, V, ncu):
    """Does some workgroup of the launch walk tiles of more than one clip (the library's own walk)?"""
    from stgcn_amd import _capi
    lib = _capi.lib()
    tpc = -(-T * V // 256)
    short = 1 if lib.stgcn_stem_short_tile_blocks(128, T, V, 9) > 0 else 0
    G = min(N * tpc, ncu)
    first, end = ctypes.c_int(), ctypes.c_int()
    for b in range(G):
        assert lib.stgcn_stem_walk_run(b, G, N, tpc, short, ctypes.byref(first), ctypes.byref(end)) == 0
        if end.value > first.value and first.value // tpc != (end.value - 1) // tpc:
            return True
    return False


def _smallest_crossing_n(T, V, ncu):
    return next(N for N in range(1, 65536) if _walk_crosses_a_clip(N, T, V, ncu))


def test_the_plan_names_the_kernel_and_the_walk_crosses_where_it_says():
    """Host only.  The kernel's name does not carry its template arguments: these shapes are answered as before."""
    from stgcn_amd import _capi
    lib = _capi.lib()
    for (N, T, V, C), name in SHAPES + [((40, WALK_T, WALK_V, 128), V6)]:
        for fl in (1, 1 | _capi.OUT_NTVC):
            assert lib.stgcn_stem_kernel_name(3, C, T, V, 9, 3, fl).decode() == name, (N, T, V, C, fl)
    # on 256 workgroups 40 clips of 24 x 22 are 120 tiles, one each; up to 128 clips the balanced runs stay inside a clip (two
    # workgroups share one), the first launch in which a run crosses a clip boundary has 129
    assert not _walk_crosses_a_clip(40, WALK_T, WALK_V, 256)
    assert _smallest_crossing_n(WALK_T, WALK_V, 256) == 129


@pytest.mark.gpu
@pytest.mark.parametrize("shape,name", SHAPES, ids=_ids(SHAPES))
def test_direct_stores_match_the_oracle_and_the_staged_epilogue(shape, name, dev):
    _, ref = _setup(shape)
    out = _run(shape, dev)
    gate, strict = MATH_GATES["bf16x3"]
    err = parity_gate(out, ref, gate, f"fused stem {shape} bf16x3 nctv", strict=strict)
    print(f"{shape} bf16x3 nctv: max|err|/max|ref| = {err:.2e}")
    out_cl = _run(shape, dev, channels_last=True)
    assert out_cl.stride() != out.stride() and torch.equal(out, out_cl), f"{shape}: (N,C,T,V) and permuted (N,T,V,C) results differ"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BF16_SHAPES, ids=_ids(BF16_SHAPES))
def test_direct_stores_bf16_output(shape, dev):
    """bf16 results: one 8-byte store of two packed pairs in the straight-line form, element stores in the others."""
    _, ref = _setup(shape)
    out = _run(shape, dev, bf16=True)
    assert out.dtype == torch.bfloat16
    parity_gate(out.float(), ref, 1e-2, f"fused stem {shape} bf16x3, bf16 output", strict=False)
    out_cl = _run(shape, dev, bf16=True, channels_last=True)
    assert torch.equal(out, out_cl), f"{shape}: bf16 (N,C,T,V) and permuted (N,T,V,C) results differ"
    # ... and it is the fp32 result rounded once
    assert torch.equal(out, _run(shape, dev).bfloat16())


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_a_result_one_element_off_16_bytes(bf16, dev):
    """Rows that are aligned by their indices in a tensor that is not: the kernel sees the address and takes the element form."""
    shape = SHAPES[0][0]
    want = _run(shape, dev, bf16=bf16)
    got = _run(shape, dev, bf16=bf16, skew=1)
    assert got.data_ptr() % 16 == got.element_size()
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_a_workgroup_walks_more_than_one_clip(dev):
    """The smallest launch of 24 x 22 clips in which a workgroup's run crosses a clip boundary (129 clips on 256 workgroups).  The
    clips repeat three inputs, so the oracle is asked for three."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    N = _smallest_crossing_n(WALK_T, WALK_V, ncu)
    assert N > 40 and not _walk_crosses_a_clip(40, WALK_T, WALK_V, ncu)
    shape = (3, WALK_T, WALK_V, 128)
    s, ref3 = _setup(shape)
    idx = torch.arange(N) % 3
    x = s.x[idx]
    out = _run(shape, dev, x=x)
    gate, strict = MATH_GATES["bf16x3"]
    parity_gate(out, ref3[idx], gate, f"fused stem {N} clips of {WALK_T} x {WALK_V}", strict=strict)
    assert torch.equal(out, _run(shape, dev, x=x, channels_last=True))
    assert torch.equal(out[:3], _run(shape, dev)), "a clip's result depends on the workgroup that walked it"
