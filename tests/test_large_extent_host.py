"""Large extents, host side (no GPU): the tiled gate of tests/large_extent.py fails when it must, every row of its tables meets
the no-aliasing condition, and the size queries do not wrap at the extents the GPU rows run at."""
import pytest
import torch

import large_extent as le
from large_extent import Extent, gate_tiled

CHUNK = 300                   # elements per compared piece here: the 60-element clips below fall into many pieces
REL = 1e-4


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


# ---- gate_tiled ---------------------------------------------------------------------------------------------------------------------
def _tiling(N=40, n0=7, unit=(5, 4, 3), seed=0):
    ref = torch.randn(n0, *unit, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    out = ref.repeat(-(-N // n0), 1, 1, 1)[:N].float()
    assert out.numel() > 5 * CHUNK
    return out, ref


def test_gate_passes_on_an_exact_tiling():
    out, ref = _tiling()
    assert gate_tiled(out, ref, REL, True, "exact", chunk=CHUNK) <= 1e-7
    # a whole number of batches or not, a strided view (the stem's channels-last result), a clip above the chunk, bf16 storage
    out, ref = _tiling(N=42)
    gate_tiled(out, ref, REL, True, "whole", chunk=CHUNK)
    gate_tiled(out.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), ref, REL, True, "view", chunk=CHUNK)
    gate_tiled(out, ref, REL, True, "clip above the chunk", chunk=7)
    gate_tiled(out.bfloat16(), ref, 4e-3, False, "bf16", chunk=CHUNK)


@pytest.mark.parametrize("where", ["first", "last"])
def test_gate_fails_on_one_wrong_element(where):
    out, ref = _tiling()
    flat = 11 if where == "first" else out.numel() - 2
    assert (flat < CHUNK) == (where == "first") and (flat >= out.numel() - CHUNK) == (where == "last")
    out.view(-1)[flat] += 0.01
    with pytest.raises(AssertionError, match=rf"max abs err .* flat index {flat} "):
        gate_tiled(out, ref, REL, True, where, chunk=CHUNK)
    # small next to max|ref| but not next to the element: the second criterion alone
    out, ref = _tiling()
    ref.view(-1)[flat % ref.numel()] = 1e-3
    out = ref.repeat(6, 1, 1, 1)[:40].float()
    out.view(-1)[flat] += 5e-5 * ref.abs().max().item()
    gate_tiled(out, ref, REL, False, where, chunk=CHUNK)
    with pytest.raises(AssertionError, match=rf"allclose.* flat index {flat} "):
        gate_tiled(out, ref, REL, True, where, chunk=CHUNK)


def test_gate_fails_when_a_clip_is_stored_one_period_remainder_off():
    """The miniature of an offset wrap: the threshold 2^9 leaves 512 % 420 = 92 modulo the period and 32 modulo the clip, so
    the clip that should start at 25 * 60 lands 92 elements early and keeps the right values - in the wrong place."""
    out, ref = _tiling()
    clip, period = 60, 7 * 60
    assert not [t for t in (512,) if t % clip == 0 or t % period == 0]
    good = out.clone().view(-1)
    at = 25 * clip
    out.view(-1)[at - 512 % period:at - 512 % period + clip] = good[at:at + clip]
    with pytest.raises(AssertionError, match="max abs err"):
        gate_tiled(out, ref, REL, True, "offset clip", chunk=CHUNK)
    # the same store one whole period off is what the shape condition excludes: it cannot be seen
    out2 = good.clone()
    out2[at - period:at - period + clip] = good[at:at + clip]
    gate_tiled(out2.view(40, 5, 4, 3), ref, REL, True, "a period off", chunk=CHUNK)


def test_gate_fails_on_an_unwritten_element():
    out, ref = _tiling()
    out.view(-1)[1234] = float("nan")
    with pytest.raises(AssertionError, match="non-finite output at flat index 1234 "):
        gate_tiled(out, ref, REL, False, "nan", chunk=CHUNK)


def test_a_failure_names_the_largest_threshold_passed():
    assert "past 2^31 elements, 2^33 bytes" in le._fmt_threshold((1 << 31) + 5, 4)
    assert "past 2^30 elements, 2^31 bytes" in le._fmt_threshold((1 << 30) + 5, 2)
    assert "past no threshold" in le._fmt_threshold(17, 4)


# ---- the shape condition ------------------------------------------------------------------------------------------------------------
def test_every_row_of_table_a_meets_the_shape_condition():
    table = le.table_a()
    assert len(table) >= 25
    for name, ext in table.items():
        ext.assert_large_and_alias_free(name)
        for t in le.THRESHOLDS[ext.dtype]:
            assert t % ext.clip and t % (ext.n0 * ext.clip), (name, t)
        assert ext.N % ext.n0 == 0 and ext.result == ext.N * ext.clip
        # the fewest tilings: one fewer stays at or below 2^31 (the patch embedding's result: 2^30, the most its plan takes twice)
        if name.startswith("vit_patch_embed"):
            assert 1 << 30 < ext.result < 1 << 31 and ext.clip * (ext.N - ext.n0) <= 1 << 30, name
        else:
            assert (ext.named[1] // ext.N) * (ext.N - ext.n0) <= 1 << 31, name
    # the example of the issue: 128 x 12 x 22 clips
    assert le.aliasing_thresholds(33792, 7) == [] and (1 << 29) % (7 * 33792) == 152576 and (1 << 31) % 33792 == 2048
    assert le.aliasing_thresholds(1024, 7) == [1 << 29, 1 << 30, 1 << 31], "one row of a 1024-wide linear would alias"
    with pytest.raises(AssertionError):
        Extent.past((1, 1024)).assert_large_and_alias_free("a row of 1024")
    with pytest.raises(AssertionError):
        Extent(7 * 100, (128, 12, 22)).assert_large_and_alias_free("small")


def test_no_row_needs_more_than_48_gib():
    class Case:
        id, tensors = "x", 42 * le.GIB
    assert le.need_bytes(Case) == 48 * le.GIB
    Case.tensors += 1
    with pytest.raises(AssertionError):
        le.need_bytes(Case)


# ---- the size queries ---------------------------------------------------------------------------------------------------------------
FULL = (300, 25)              # (T, V) of a full-size clip
A_CLIPS = le.table_a()["tcn-128x128x9x1x12x22-f32"].N


def _non_decreasing(f, Ns):
    got = [f(n) for n in Ns]
    assert all(g > 0 for g in got), got
    assert got == sorted(got), got
    return got


CLIPS = [(1, 2, 7, 4096, le.MAX_CLIPS), FULL], [(1, 7, 4096, A_CLIPS, le.MAX_CLIPS), (12, 22)]


@pytest.mark.parametrize("Ns,tv", CLIPS, ids=["full-size", "table A"])
def test_clip_queries_do_not_wrap(Ns, tv, lib):
    from stgcn_amd import functional as F
    T, V = tv
    fl = F._flags(F.MATH_BF16X3, False)
    for N, got in zip(Ns, _non_decreasing(lambda n: lib.stgcn_stem_ws_bytes(n, 3, 128, T, V, 9, 3, fl), Ns)):
        assert got >= N * 3 * V * V * 4, "P (N,S,V,V) floats sit at the head of the stem's workspace"
    plane = 128 * T * V * 4
    for N, got in zip(Ns, _non_decreasing(lambda n: lib.stgcn_agcn_train_ws_bytes(n, 3, 128, T, V, 3, 1), Ns)):
        assert got >= 2 * N * plane, "materialise = 1: room for the two pre-BatchNorm branches"
    _non_decreasing(lambda n: lib.stgcn_agcn_train_ws_bytes(n, 3, 128, T, V, 3, 0), Ns)
    for N, got in zip(Ns, _non_decreasing(lambda n: lib.stgcn_agcn_backward_ws_bytes(n, 3, 128, T, V, 3, 3), Ns)):
        assert got >= 2 * N * plane, "recompute bits 0 and 1: the generic path rebuilds both branches in the workspace"
    _non_decreasing(lambda n: lib.stgcn_agcn_backward_ws_bytes(n, 3, 128, T, V, 3, 1), Ns)
    for N, got in zip(Ns, _non_decreasing(lambda n: lib.stgcn_tcn_train_ws_bytes(n, 128, 128, T, V, 9, 1, fl), Ns)):
        assert got >= N * plane, "the raw convolution z (N,Cout,T_out,V)"
    for N, got in zip(Ns, _non_decreasing(lambda n: lib.stgcn_tcn_backward_ws_bytes(n, 128, 128, T, V, 9, 1, fl), Ns)):
        assert got >= N * plane, "the gradient before the BatchNorm, dz (N,Cout,T_out,V)"
    for pass_, cin, cout in [(p, ci, co) for p in (0, 1, 2) for ci, co in ((3, 128), (64, 128), (128, 256))]:
        got = _non_decreasing(lambda n: lib.stgcn_st_attention_ws_bytes(n, cin, cout, cout // 4, T, V, 8, pass_), Ns)
        # (the header names no tensor inside this workspace; the eval forward and the backward keep q, k, v of every frame)
        if pass_ != 1:
            assert got[-1] >= Ns[-1] * (cout // 2 + cout) * T * V * 4, (pass_, cin, cout)
    assert lib.stgcn_tcn_train_ws_bytes(le.MAX_CLIPS, 128, 128, *FULL, 9, 1, fl) > 1 << 37      # 251 GB: size_t all the way


def test_sequence_queries_do_not_wrap(lib):
    blk = le.table_a()["vit_block_forward-" + "x".join(map(str, le.A_BLOCK))]
    L, D, heads, hidden = le.A_BLOCK
    Bs = (1, 7, 10923, blk.N, 4 * blk.N)
    ws = _non_decreasing(lambda b: lib.stgcn_vit_block_ws_bytes(b, L, D, hidden), Bs)
    assert ws[-1] == ws[-2] == ws[-3], "bounded by a slab of whole sequences"
    for B, got in zip(Bs, _non_decreasing(lambda b: lib.stgcn_vit_block_saved_bytes(b, L, D, hidden), Bs)):
        assert got >= B * L * hidden * 4, "the saved activations hold at least the hidden layer's"
    assert lib.stgcn_vit_block_saved_bytes(blk.N, L, D, hidden) > 1 << 33
    _non_decreasing(lambda b: lib.stgcn_vit_block_backward_ws_bytes(b, L, D, hidden), Bs)
    # 65537 sequences of one token, and the full-size heads: 256 clips of 300 frames are 76800 stage-1 sequences
    for L1, D1, h1 in ((1, 256, 512), (25, 256, 512), (300, 512, 1024)):
        for q in (lib.stgcn_vit_block_ws_bytes, lib.stgcn_vit_block_saved_bytes, lib.stgcn_vit_block_backward_ws_bytes):
            if L1 <= 256 or q is lib.stgcn_vit_block_ws_bytes:          # (the last two describe the resident form: L <= 256)
                _non_decreasing(lambda b: q(b, L1, D1, h1), (1, 65535, 65536, 65537, 76800, 1 << 24))


def test_coverage_queries_know_the_2_32_work_items_of_a_launch(lib):
    """gridDim.x * blockDim.x stays below 2^32 (csrc/common.h: grid_fits): the queries answer for it."""
    from stgcn_amd import functional as F
    n = le.POOL_CLASSIFY_CLIPS                                     # one workgroup of 1024 threads per clip
    assert F.vit_pool_classify_supported(n - 1, 1, 64, 14) and not F.vit_pool_classify_supported(n, 1, 64, 14)
    assert F.vit_pool_classify_supported(le.table_a()["vit_pool_classify-" + "x".join(map(str, le.A_POOL_CLASSIFY))].N, 9, 64, 14)
    assert F.vit_pool_supported((1 << 24) - 1, 2, 256) and not F.vit_pool_supported(1 << 24, 2, 256)      # 256 threads, one chunk
    assert not F.vit_pool_supported(1 << 23, 2, 512)               # two chunks of 64 float4 columns per sequence
    C, T, V, p1, p2, E = le.A_PATCH
    ext = le.table_a()["vit_patch_embed-" + "x".join(map(str, le.A_PATCH))]
    assert F.vit_patch_embed_supported(ext.N, C, T, V, p1, p2, E)
    past = le.N0 * le.tiles_past(1 << 31, ext.clip)
    assert not F.vit_patch_embed_supported(past, C, T, V, p1, p2, E), "a result of 2^31 elements is refused by the plan"


def test_head_query_does_not_wrap(lib):
    from stgcn_amd import functional as F
    flags = F._vit_flags(F.MATH_F32)

    for (T, V), order in [((40, 22), "ST"), ((6, 22), "ST"), (FULL, "ST"), (FULL, "TS")]:      # the small head, Table A's, full size
        def ws(n):
            shape = F._head_shape(n, T, V, 128, 256, 512, 8, 512, 1024, 2, 2, 14)
            return lib.stgcn_altformer_head_ws_bytes(shape, flags, flags, F._head_flags(order))
        Ns = [n for n in (1, 2, 256, 8192, le.MAX_CLIPS)
              if F.altformer_head_supported(n, T, V, 128, 256, 512, 8, 512, 1024, 2, 2, 14, order=order)]
        assert len(Ns) >= 3 and ((T, V) == FULL or Ns[-1] == le.MAX_CLIPS), (T, V, order, Ns)
        _non_decreasing(ws, Ns)
        # what a stage hands to the next: the stage-1 tokens (N, T, V, E1) stay in the workspace
        assert ws(Ns[-1]) >= Ns[-1] * T * V * 256 * 4, (T, V, order)
