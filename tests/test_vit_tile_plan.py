"""CPU tests of the token-major linear's tile plan (csrc/vit.h ``linear_tile``, read through ``stgcn_vit_linear_tile``) and of
the module switch that turns it on (``Block.small_tiles``, ``set_low_latency``).  No GPU: the plan is a host function of the
shape and the flags, it never asks the device."""
import itertools

import torch.nn as nn

MS = (1, 22, 180, 704, 3960, 4096, 32768, 126720)
KS = (256, 512, 1024)
NOUTS = (256, 512, 768, 1536)
T128, T64, T32 = (128 << 16) | 128, (64 << 16) | 64, (32 << 16) | 64


def _lib():
    from stgcn_amd import _capi
    return _capi, _capi.lib()


def _area(t):
    return (t >> 16) * (t & 0xFFFF)


def test_flag_values_match_the_header():
    import os
    import re
    capi, _ = _lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stgcn_hip.h")).read()
    for name, value in (("TILE_MASK", 0x30000), ("TILE_AUTO", 0x10000), ("TILE_64", 0x20000), ("TILE_32", 0x30000)):
        assert getattr(capi, "VIT_" + name) == value
        assert re.search(rf"#define\s+STGCN_VIT_{name}\s+0x{value:x}u", hdr), name
    assert capi.VIT_TILE_MASK & (capi.MATH_MASK | capi.VIT_GELU | capi.VIT_QKV_F32 | capi.VIT_DGELU | capi.VIT_ACCUMULATE) == 0


def test_field_zero_is_the_128_tile_everywhere():
    capi, lib = _lib()
    for M, K, Nout in itertools.product(MS, KS, NOUTS):
        for math in (capi.MATH_F32, capi.MATH_BF16X3):
            assert lib.stgcn_vit_linear_tile(M, K, Nout, math) == T128, (M, K, Nout, math)


def test_forced_forms_return_themselves():
    capi, lib = _lib()
    for M, K, Nout in itertools.product(MS, KS, NOUTS):
        assert lib.stgcn_vit_linear_tile(M, K, Nout, capi.VIT_TILE_64) == T64, (M, K, Nout)
        assert lib.stgcn_vit_linear_tile(M, K, Nout, capi.VIT_TILE_32 | capi.MATH_BF16X3) == T32, (M, K, Nout)


def test_auto_keeps_128_for_large_calls():
    capi, lib = _lib()
    for M, K, Nout in itertools.product((32768, 126720), KS, NOUTS):
        assert lib.stgcn_vit_linear_tile(M, K, Nout, capi.VIT_TILE_AUTO) == T128, (M, K, Nout)


def test_auto_goes_below_128_at_the_one_clip_shapes():
    capi, lib = _lib()
    for shape in ((3960, 256, 768), (3960, 256, 256), (180, 512, 1536), (704, 512, 1536)):
        t = lib.stgcn_vit_linear_tile(*shape, capi.VIT_TILE_AUTO)
        assert t in (T64, T32), (shape, hex(t))


def test_auto_area_does_not_decrease_with_m():
    capi, lib = _lib()
    for K, Nout in itertools.product(KS, NOUTS):
        areas = [_area(lib.stgcn_vit_linear_tile(M, K, Nout, capi.VIT_TILE_AUTO)) for M in sorted(set(MS) | set(range(1, 40000, 97)))]
        assert all(a > 0 for a in areas) and areas == sorted(areas), (K, Nout)
        assert {areas[0], areas[-1]} == {32 * 64, 128 * 128}, (K, Nout)        # the smallest form at M = 1, the largest at the end


def test_unsupported_linear_has_no_tile():
    capi, lib = _lib()
    for fl in (0, capi.VIT_TILE_AUTO, capi.VIT_TILE_64, capi.VIT_TILE_32):
        assert lib.stgcn_vit_linear_tile(180, 48, 256, fl) == 0                 # K % 32 != 0
        assert lib.stgcn_vit_linear_tile(180, 256, 256, fl | capi.MATH_BF16) == 0  # an arithmetic the linear does not have
        assert lib.stgcn_vit_linear_tile(0, 256, 256, fl) == 0


def test_functional_query_unpacks_the_tile():
    from stgcn_amd import functional as F
    capi, _ = _lib()
    assert F.vit_linear_tile(180, 512, 1536) == (128, 128)
    assert F.vit_linear_tile(180, 512, 1536, capi.VIT_TILE_32 | capi.MATH_BF16X3) == (32, 64)
    assert F.vit_linear_tile(180, 512, 1536, capi.VIT_TILE_AUTO) in ((64, 64), (32, 64))
    assert F.vit_linear_tile(180, 48, 1536) is None


def test_block_defaults_are_unchanged():
    from stgcn_amd import altformer
    blk = altformer.Block(256, 8, mlp_ratio=2.)
    assert blk.small_tiles is False
    assert blk.hip_min_tokens == 4096 == altformer.HIP_MIN_TOKENS
    assert blk.hip_train_min_tokens == altformer.HIP_TRAIN_MIN_TOKENS


def test_set_low_latency_round_trip():
    import stgcn_amd
    from stgcn_amd import altformer
    m = nn.Sequential(altformer.Block(256, 8, mlp_ratio=2.), nn.Sequential(altformer.Block(512, 8, mlp_ratio=2.)))
    blocks = [b for b in m.modules() if isinstance(b, altformer.Block)]
    assert len(blocks) == 2
    blocks[1].hip_train_min_tokens = 777
    train = [b.hip_train_min_tokens for b in blocks]
    stgcn_amd.set_low_latency(m)
    assert all(b.small_tiles is True and b.hip_min_tokens == altformer.LOW_LATENCY_MIN_TOKENS for b in blocks)
    assert [b.hip_train_min_tokens for b in blocks] == train
    stgcn_amd.set_low_latency(m, min_tokens=100)
    assert all(b.small_tiles is True and b.hip_min_tokens == 100 for b in blocks)
    assert [b.hip_train_min_tokens for b in blocks] == train
    stgcn_amd.set_low_latency(m, False)
    assert all(b.small_tiles is False and b.hip_min_tokens == altformer.HIP_MIN_TOKENS == 4096 for b in blocks)
    assert [b.hip_train_min_tokens for b in blocks] == train
    assert 0 <= altformer.LOW_LATENCY_MIN_TOKENS <= altformer.HIP_MIN_TOKENS
