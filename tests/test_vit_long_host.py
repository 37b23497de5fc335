"""Long sequences (256 < L <= 4096) of the AltFormer heads' blocks, host side (no GPU): the answers of the new queries next to
the unchanged old ones, the workspace size against the carve written out by hand, the argument checks of the streaming
attention entry point, and the module's routing on the CPU."""
import ctypes

import pytest
import torch

SLAB = 32768          # tokens per slab of stgcn_vit_block_forward (vit.h: kSlabRows)
MAX_L = 4096          # STGCN_VIT_MAX_STREAM_L


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


def test_header_binding_and_constant():
    import os
    import re
    from stgcn_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "stgcn_hip.h")).read()
    assert re.search(rf"#define\s+STGCN_VIT_MAX_STREAM_L\s+{MAX_L}\b", hdr)
    for n in ("stgcn_vit_attention_stream_supported", "stgcn_vit_attention_stream", "stgcn_vit_block_forward_supported"):
        assert re.search(rf"\b{n}\s*\(", hdr) and n in _capi.PROTOTYPES, n
    assert _capi.ABI_VERSION == 11 and _capi.lib().stgcn_version() == 11, "additive: the ABI version stays"


@pytest.mark.parametrize("L", [1, 256, 257, 500, 4096])
def test_new_queries_cover_every_length_up_to_the_cap(L, lib):
    from stgcn_amd import functional as F
    for hd in (32, 64):
        assert lib.stgcn_vit_attention_stream_supported(L, 8, hd) == 1
        assert F.vit_attention_stream_supported(L, 8, hd)
    for D, hidden in ((256, 512), (512, 1024), (512, 512)):
        assert lib.stgcn_vit_block_forward_supported(L, D, 8, hidden) == 1
        assert F.vit_block_forward_supported(L, D, 8, hidden)


def test_new_queries_refuse_what_is_not_covered(lib):
    for L in (4097, 0, -3):
        assert lib.stgcn_vit_attention_stream_supported(L, 8, 32) == 0
        assert lib.stgcn_vit_block_forward_supported(L, 256, 8, 512) == 0
    for L in (22, 500):
        assert lib.stgcn_vit_attention_stream_supported(L, 8, 48) == 0          # head_dim 48
        assert lib.stgcn_vit_attention_stream_supported(L, 0, 32) == 0
        assert lib.stgcn_vit_block_forward_supported(L, 384, 8, 768) == 0        # head_dim 48
        assert lib.stgcn_vit_block_forward_supported(L, 256, 8, 500) == 0        # hidden not a multiple of 64
        assert lib.stgcn_vit_block_forward_supported(L, 256, 7, 512) == 0        # D % heads


def test_old_and_training_queries_keep_their_answers(lib):
    for D, hidden, hd in ((256, 512, 32), (512, 1024, 64)):
        assert lib.stgcn_vit_block_supported(256, D, 8, hidden) == 1 and lib.stgcn_vit_block_supported(257, D, 8, hidden) == 0
        assert lib.stgcn_vit_attention_supported(256, 8, hd) == 1 and lib.stgcn_vit_attention_supported(257, 8, hd) == 0
        assert lib.stgcn_vit_block_train_supported(256, D, 8, hidden) == 1
        assert lib.stgcn_vit_block_train_supported(257, D, 8, hidden) == 0
        assert lib.stgcn_vit_attention_backward_supported(256, 8, hd) == 1
        assert lib.stgcn_vit_attention_backward_supported(257, 8, hd) == 0
        assert lib.stgcn_vit_block_saved_bytes(4, 257, D, hidden) == 0
        assert lib.stgcn_vit_block_backward_ws_bytes(4, 257, D, hidden) == 0
        assert lib.stgcn_vit_block_saved_bytes(4, 256, D, hidden) > 0


def carve(B, L, D, hidden):
    """BlockStore by hand: qkv, attention output, first residual and hidden activations of one slab of whole sequences, each piece
    padded to 256 bytes."""
    rows = min(B, max(1, SLAB // L)) * L
    up = lambda n: (n + 255) // 256 * 256     # noqa: E731
    return sum(up(rows * w * 4) for w in (3 * D, D, D, hidden))


def test_workspace_is_bounded_by_a_slab_and_is_what_the_carve_takes(lib):
    a, b = lib.stgcn_vit_block_ws_bytes(200, 500, 512, 1024), lib.stgcn_vit_block_ws_bytes(400, 500, 512, 1024)
    assert a > 0 and a == b == carve(200, 500, 512, 1024)                       # 65 sequences of 500 per slab
    for B, L, D, hidden in [(1, 4096, 512, 1024), (8, 4096, 512, 1024), (9, 4096, 512, 1024), (100, 4096, 256, 512),
                            (3, 4096, 4096, 4096), (70, 500, 256, 512), (66, 500, 256, 512), (5, 257, 256, 512), (3, 300, 512, 1024)]:
        got = lib.stgcn_vit_block_ws_bytes(B, L, D, hidden)
        assert got == carve(B, L, D, hidden), (B, L, D, hidden)
    # a slab of 8 sequences of 4096 is exactly the slab's 32768 tokens; the short last slab (B = 9: one sequence) uses a prefix
    assert lib.stgcn_vit_block_ws_bytes(9, 4096, 512, 1024) == lib.stgcn_vit_block_ws_bytes(8, 4096, 512, 1024) \
        == SLAB * (5 * 512 + 1024) * 4
    assert lib.stgcn_vit_block_ws_bytes(1, 4096, 512, 1024) == 4096 * (5 * 512 + 1024) * 4
    assert lib.stgcn_vit_block_ws_bytes(8, 4096, 4096, 4096) == SLAB * 6 * 4096 * 4 > 2 ** 31      # size_t, not int


def test_argument_errors_come_before_any_device_work(lib):
    """No GPU in this test: an answer at all means that nothing was launched."""
    rc = lib.stgcn_vit_attention_stream(None, None, 2, 500, 8, 32, 0.1, None)
    assert rc == -1 and b"null" in lib.stgcn_last_error().lower()
    host = (ctypes.c_float * 4)()             # non-null addresses that are never dereferenced
    p = ctypes.cast(host, ctypes.c_void_p)
    assert lib.stgcn_vit_attention_stream(p, None, 2, 500, 8, 32, 0.1, None) == -1
    for B, L, heads in ((0, 500, 8), (2, 0, 8), (2, 500, 0)):
        assert lib.stgcn_vit_attention_stream(p, p, B, L, heads, 32, 0.1, None) == -1, (B, L, heads)
    assert lib.stgcn_vit_attention_stream(p, p, 2, 4097, 8, 32, 0.1, None) == -2
    assert b"4097" in lib.stgcn_last_error()
    assert lib.stgcn_vit_attention_stream(p, p, 2, 500, 8, 48, 0.1, None) == -2
    assert lib.stgcn_vit_attention(p, p, 2, 257, 8, 32, 0.1, None) == -2, "the resident entry point still refuses L > 256"
    other = (ctypes.c_float * 4)()
    y = ctypes.cast(other, ctypes.c_void_p)
    rc = lib.stgcn_vit_block_forward(*([p] * 13), 1e-6, 0.1, p, 0, y, 2, 4097, 256, 8, 512, 0, None)
    assert rc == -2
    rc = lib.stgcn_vit_block_forward(*([p] * 13), 1e-6, 0.1, p, 0, y, 2, 500, 256, 8, 512, 0, None)
    assert rc == -3, "L = 500 is covered now: the next check is the workspace size"


def test_a_long_block_on_the_cpu_takes_the_torch_path():
    from stgcn_amd.altformer import Block
    torch.manual_seed(0)
    blk = Block(256, 8, mlp_ratio=2., qkv_bias=True).eval()
    x = torch.randn(2, 300, 256)
    with torch.no_grad():
        assert not blk.hip_applies(x) and not blk.uses_hip(x) and not blk.trains_on_hip(x)
        y = blk(x)
    assert y.shape == (2, 300, 256) and torch.isfinite(y).all()
    assert not blk.trains_on_hip(x.requires_grad_())
