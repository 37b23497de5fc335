"""Training the AltFormer heads' blocks on long sequences (256 < L <= 4096), host side (no GPU): the six new symbols next to
the unchanged resident queries, the sizes of `saved` and of the workspace against the carves written out by hand, the
argument checks of the streaming attention backward and of the block backward, and the module's opt-in on the CPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ABI = ["stgcn_vit_attention_backward_stream_supported", "stgcn_vit_attention_backward_stream_ws_bytes",
           "stgcn_vit_attention_backward_stream", "stgcn_vit_block_train_long_supported",
           "stgcn_vit_block_train_long_saved_bytes", "stgcn_vit_block_train_long_ws_bytes"]
SLAB = 32768          # tokens per slab of the block entry points (vit.h: kSlabRows)


def up256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


def test_six_symbols_declared_bound_and_exported(lib):
    from stgcn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    for n in NEW_ABI:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(lib, n), n
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr)
    assert _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11, "additive: the ABI version stays"


@pytest.mark.parametrize("L", [1, 256, 257, 500, 4096])
def test_long_queries_cover_every_length_up_to_the_cap(L, lib):
    from stgcn_amd import functional as F
    for hd in (32, 64):
        assert lib.stgcn_vit_attention_backward_stream_supported(L, 8, hd) == 1
        assert F.vit_attention_backward_stream_supported(L, 8, hd)
    for D, hidden in ((256, 512), (512, 1024)):
        assert lib.stgcn_vit_block_train_long_supported(L, D, 8, hidden) == 1
        assert F.vit_block_train_long_supported(L, D, 8, hidden)
        assert lib.stgcn_vit_block_train_long_saved_bytes(4, L, D, hidden) > 0
        assert lib.stgcn_vit_block_train_long_ws_bytes(4, L, D, 8, hidden) > 0


def test_long_queries_refuse_what_is_not_covered(lib):
    for L in (4097, 0):
        assert lib.stgcn_vit_attention_backward_stream_supported(L, 8, 32) == 0
        assert lib.stgcn_vit_attention_backward_stream_ws_bytes(2, L, 8) == 0
        assert lib.stgcn_vit_block_train_long_supported(L, 256, 8, 512) == 0
        assert lib.stgcn_vit_block_train_long_saved_bytes(4, L, 256, 512) == 0
        assert lib.stgcn_vit_block_train_long_ws_bytes(4, L, 256, 8, 512) == 0
    for L in (22, 500):
        assert lib.stgcn_vit_attention_backward_stream_supported(L, 8, 48) == 0     # head_dim 48
        assert lib.stgcn_vit_block_train_long_supported(L, 384, 8, 768) == 0         # head_dim 48
        assert lib.stgcn_vit_block_train_long_supported(L, 256, 8, 500) == 0         # hidden not a multiple of 64
        assert lib.stgcn_vit_block_train_long_supported(L, 256, 7, 512) == 0         # D % heads
        assert lib.stgcn_vit_block_train_long_ws_bytes(4, L, 384, 8, 768) == 0
        assert lib.stgcn_vit_block_train_long_ws_bytes(4, L, 256, 8, 500) == 0
        assert lib.stgcn_vit_block_train_long_saved_bytes(4, L, 256, 500) == 0
        assert lib.stgcn_vit_block_train_long_saved_bytes(0, L, 256, 512) == 0


@pytest.mark.parametrize("L", [22, 180, 256])
def test_short_lengths_answer_what_the_resident_queries_answer(L, lib):
    for B in (1, 32, 5000):
        for D, hidden in ((256, 512), (512, 1024)):
            assert lib.stgcn_vit_block_train_long_saved_bytes(B, L, D, hidden) == lib.stgcn_vit_block_saved_bytes(B, L, D, hidden) > 0
            assert lib.stgcn_vit_block_train_long_ws_bytes(B, L, D, 8, hidden) == lib.stgcn_vit_block_backward_ws_bytes(B, L, D, hidden) > 0


def test_saved_is_the_unchanged_carve(lib):
    B, L, D, hidden = 4, 300, 256, 512
    rows = B * L
    assert lib.stgcn_vit_block_train_long_saved_bytes(B, L, D, hidden) == sum(up256(rows * w * 4) for w in (3 * D, D, D, hidden, hidden))


def test_workspace_is_bounded_by_a_slab_and_adds_only_the_statistics(lib):
    a, b = (lib.stgcn_vit_block_train_long_ws_bytes(B, 500, 256, 8, 512) for B in (200, 400))
    assert a > 0 and a == b, "65 sequences of 500 per slab, whatever B"
    assert lib.stgcn_vit_block_train_long_ws_bytes(70, 500, 256, 8, 512) == a
    assert lib.stgcn_vit_block_train_long_ws_bytes(2, 500, 256, 8, 512) < a
    # 6 sequences of 300 are the tokens of 12 sequences of 150, which the resident carve sizes: the difference is the
    # statistics of the slab, (m, 1 / l, delta, pad) per (sequence, head, query), padded to 256 bytes
    for B, D, heads, hidden in ((6, 256, 8, 512), (6, 512, 8, 1024), (6, 256, 4, 512), (1000, 256, 8, 512)):
        seqs = min(B, SLAB // 300)
        resident = lib.stgcn_vit_block_backward_ws_bytes(2 * seqs, 150, D, hidden)
        assert resident > 0
        assert lib.stgcn_vit_block_train_long_ws_bytes(B, 300, D, heads, hidden) - resident == up256(seqs * heads * 300 * 4 * 4)
    assert lib.stgcn_vit_attention_backward_stream_ws_bytes(3, 257, 8) == up256(3 * 8 * 257 * 16)
    assert lib.stgcn_vit_attention_backward_stream_ws_bytes(1, 1, 1) == 256


def test_resident_queries_keep_their_answers(lib):
    for D, hidden, hd in ((256, 512, 32), (512, 1024, 64)):
        assert lib.stgcn_vit_block_train_supported(256, D, 8, hidden) == 1
        assert lib.stgcn_vit_block_train_supported(257, D, 8, hidden) == 0
        assert lib.stgcn_vit_attention_backward_supported(256, 8, hd) == 1
        assert lib.stgcn_vit_attention_backward_supported(257, 8, hd) == 0
        assert lib.stgcn_vit_block_saved_bytes(4, 257, D, hidden) == 0
        assert lib.stgcn_vit_block_backward_ws_bytes(4, 257, D, hidden) == 0


def test_argument_errors_come_before_any_device_work(lib):
    """No GPU in this test: an answer at all means that nothing was launched."""
    host = (ctypes.c_float * 4)()             # non-null addresses that are never dereferenced
    p = ctypes.cast(host, ctypes.c_void_p)
    big = 1 << 40
    rc = lib.stgcn_vit_attention_backward_stream(None, None, None, None, None, 0, 2, 500, 8, 32, 0.1, None)
    assert rc == -1 and b"null" in lib.stgcn_last_error().lower()
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert lib.stgcn_vit_attention_backward_stream(*args, big, 2, 500, 8, 32, 0.1, None) == -1
    for B, L, heads in ((0, 500, 8), (2, 0, 8), (2, 500, 0)):
        assert lib.stgcn_vit_attention_backward_stream(p, p, p, p, p, big, B, L, heads, 32, 0.1, None) == -1, (B, L, heads)
    assert lib.stgcn_vit_attention_backward_stream(p, p, p, p, p, big, 2, 4097, 8, 32, 0.1, None) == -2
    assert b"4097" in lib.stgcn_last_error()
    assert lib.stgcn_vit_attention_backward_stream(p, p, p, p, p, big, 2, 500, 8, 48, 0.1, None) == -2
    assert b"48" in lib.stgcn_last_error()
    assert lib.stgcn_vit_attention_backward_stream(p, p, p, p, p, 0, 2, 500, 8, 32, 0.1, None) == -3
    need = lib.stgcn_vit_attention_backward_stream_ws_bytes(2, 500, 8)
    assert lib.stgcn_vit_attention_backward_stream(p, p, p, p, p, need - 1, 2, 500, 8, 32, 0.1, None) == -3
    assert lib.stgcn_vit_attention_backward(p, p, p, p, 2, 257, 8, 32, 0.1, None) == -2, "the resident entry point still refuses L > 256"

    # the block entry points: L = 500 is covered now, so the next check is the buffer size; 4097 is not
    others = [ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p) for _ in range(2)]
    dy, dx = others

    def backward(L, saved_bytes, ws_bytes):
        return lib.stgcn_vit_block_backward(*([p] * 11), p, saved_bytes, dy, dx, *([p] * 12), 1e-6, 0.1, p, ws_bytes, 2, L, 256, 8,
                                            512, 0, None)

    saved = lib.stgcn_vit_block_train_long_saved_bytes(2, 500, 256, 512)
    ws = lib.stgcn_vit_block_train_long_ws_bytes(2, 500, 256, 8, 512)
    assert backward(500, saved, ws - 8) == -3, "a short workspace at L = 500: -3, not -2"
    assert b"workspace" in lib.stgcn_last_error()
    assert backward(500, saved - 8, ws) == -3
    assert backward(500, saved, lib.stgcn_vit_block_train_long_ws_bytes(2, 250, 256, 8, 512)) == -3, \
        "the resident carve of as many tokens is short by the statistics"
    assert backward(4097, big, big) == -2 and b"4097" in lib.stgcn_last_error()
    y = others[0]
    rc = lib.stgcn_vit_block_forward_train(*([p] * 15), 1e-6, 0.1, p, 0, y, 2, 500, 256, 8, 512, 0, None)
    assert rc == -3, "the training forward takes L = 500: the next check is the size of `saved`"
    rc = lib.stgcn_vit_block_forward_train(*([p] * 15), 1e-6, 0.1, p, big, y, 2, 4097, 256, 8, 512, 0, None)
    assert rc == -2 and b"4097" in lib.stgcn_last_error()


def test_long_training_is_opt_in_and_independent_of_the_token_thresholds():
    from stgcn_amd import Block, set_hip_min_tokens, set_hip_train_min_tokens, set_long_training
    from stgcn_amd.altformer import HIP_TRAIN_MIN_TOKENS
    torch.manual_seed(0)
    net = torch.nn.Sequential(Block(256, 8, mlp_ratio=2., qkv_bias=True), Block(256, 8, mlp_ratio=2., qkv_bias=True))
    assert [b.hip_train_max_len for b in net] == [256, 256]
    set_long_training(net)
    assert [b.hip_train_max_len for b in net] == [4096, 4096]
    assert [b.hip_train_min_tokens for b in net] == [HIP_TRAIN_MIN_TOKENS] * 2, "the token threshold is not touched"
    set_hip_min_tokens(net, 0)
    set_hip_train_min_tokens(net, 7)
    assert [b.hip_train_max_len for b in net] == [4096, 4096], "the thresholds do not touch the length"
    x = torch.randn(2, 300, 256, requires_grad=True)
    assert not net[0].trains_on_hip(x), "a CPU tensor trains on torch ops whatever the length allows"
    net(x).sum().backward()
    assert x.grad is not None and all(q.grad is not None for q in net.parameters())
    set_long_training(net, False)
    assert [b.hip_train_max_len for b in net] == [256, 256]
    assert [b.hip_train_min_tokens for b in net] == [7, 7]
