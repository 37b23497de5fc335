"""Host tests (no GPU) of training the ST-ViT head's two ends on HIP: the C ABI of ``stgcn_vit_patch_embed_backward`` and
``stgcn_vit_pool_classify_backward`` and their queries, the order of their answers for the errors that need no GPU, and the two
predicates of ``ViT`` on the CPU."""
import ctypes
import os
import re

import pytest
import torch

import stvit_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
NEW_NAMES = ("stgcn_vit_patch_embed_backward", "stgcn_vit_patch_embed_backward_supported", "stgcn_vit_patch_embed_backward_ws_bytes",
             "stgcn_vit_patch_embed_backward_cut", "stgcn_vit_pool_classify_backward", "stgcn_vit_pool_classify_backward_supported",
             "stgcn_vit_pool_classify_backward_ws_bytes")
IN_NTVC, BF16X3, POOL_MAX, POOL_CLS = 0x40, 1, 0x4000000, 0x8000000


@pytest.fixture(scope="module")
def lib():
    import stgcn_amd
    return stgcn_amd.lib()


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_is_still_11(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    handle = ctypes.CDLL(build())
    for n in NEW_NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
        assert n in open(os.path.join(ROOT, "INTEGRATION.md")).read(), n
    for n in ("vit_patch_embed_backward", "vit_patch_embed_backward_supported", "vit_pool_classify_backward",
              "vit_pool_classify_backward_supported"):
        assert callable(getattr(F, n)), n
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11


def test_embedding_queries_are_host_functions_that_follow_the_forward(lib):
    from stgcn_amd import functional as F
    splits, ragged = [], []
    for name, case in sr.EMBED_CASES.items():
        N, C, T, V, p1, p2, E = case
        for fl in (0, BF16X3, IN_NTVC, IN_NTVC | BF16X3):
            assert lib.stgcn_vit_patch_embed_backward_supported(*case, fl) == lib.stgcn_vit_patch_embed_supported(*case, fl) == 1, name
            ws = lib.stgcn_vit_patch_embed_backward_ws_bytes(*case, fl)
            K, M = p1 * p2 * C, N * (T // p1) * (V // p2)
            cut = lib.stgcn_vit_patch_embed_backward_cut(*case, fl)
            rps, parts = cut >> 16, cut & 0xFFFF
            assert rps % 32 == 0 and (parts - 1) * rps < M <= parts * rps, (name, rps, parts)
            # the transposed weight and the slabs; (N, C, T, V) input: one buffer of z's size for the other layout; never more
            floor = 4 * (K * E + parts * (E * K + E)) + (0 if fl & IN_NTVC else 4 * N * C * T * V)
            assert floor <= ws <= floor + 5 * 256, (name, fl, ws, floor)
        assert F.vit_patch_embed_backward_supported(*case) and F.vit_patch_embed_backward_ws_bytes(*case, channels_last=True) == \
            lib.stgcn_vit_patch_embed_backward_ws_bytes(*case, IN_NTVC)
        assert F.vit_patch_embed_backward_cut(*case) == (rps, parts)
        splits.append(parts)
        ragged.append((M - (parts - 1) * rps) % 32)
    assert max(splits) > 1 and any(ragged), "a case with more than one token split and one with a ragged last chunk"
    # (p2 C) % 32 != 0, E % 4 != 0, ragged patches, a flag bit of another entry point, the bf16 arithmetic
    for case, fl in (((2, 24, 8, 6, 4, 2, 64), 0), ((2, 32, 8, 6, 4, 2, 66), 0), ((2, 32, 9, 6, 4, 2, 64), 0),
                     ((2, 32, 8, 6, 4, 2, 64), 0x100), ((2, 32, 8, 6, 4, 2, 64), 2), ((0, 32, 8, 6, 4, 2, 64), 0)):
        assert lib.stgcn_vit_patch_embed_backward_supported(*case, fl) == 0, (case, fl)
        assert lib.stgcn_vit_patch_embed_backward_ws_bytes(*case, fl) == 0 and lib.stgcn_vit_patch_embed_backward_cut(*case, fl) == 0
    assert lib.stgcn_vit_patch_embed_supported(2, 24, 8, 6, 4, 2, 64, 0) == 0, "the forward refuses (p2 C) % 32 != 0 too"


def test_classifier_queries_are_host_functions_that_follow_the_forward(lib):
    from stgcn_amd import functional as F
    for N, L, D, classes in ((3, 7, 192, 14), (2, 100, 512, 14), (1, 1, 64, 1), (2, 5, 96, 3), (2, 5, 8192, 3), (0, 5, 64, 3)):
        fwd = lib.stgcn_vit_pool_classify_supported(N, L, D, classes)
        for fl in (0, POOL_CLS):
            assert lib.stgcn_vit_pool_classify_backward_supported(N, L, D, classes, fl) == fwd
            ws = lib.stgcn_vit_pool_classify_backward_ws_bytes(N, L, D, classes, fl)
            assert (ws >= 12 * N * D and ws <= 12 * N * D + 3 * 256) if fwd else ws == 0
        for fl in (POOL_MAX, POOL_MAX | POOL_CLS, 0x40):
            assert lib.stgcn_vit_pool_classify_backward_supported(N, L, D, classes, fl) == 0
            assert lib.stgcn_vit_pool_classify_backward_ws_bytes(N, L, D, classes, fl) == 0
    assert F.vit_pool_classify_backward_supported(2, 100, 512, 14, "cls") and F.vit_pool_classify_backward_supported(2, 100, 512, 14, "mean")
    assert not F.vit_pool_classify_backward_supported(2, 100, 512, 14, "max")


def _host():
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    p = ctypes.c_void_p(addr + (-addr) % 16)          # 16-byte aligned, never touched
    return buf, p, ctypes.c_void_p(p.value + 16), ctypes.c_void_p(p.value + 4)


def test_embedding_backward_answers_in_the_documented_order(lib):
    buf, p, q, odd = _host()
    dims = (2, 128, 180, 22, 20, 2, 512)
    ws = lib.stgcn_vit_patch_embed_backward_ws_bytes(*dims, 0)

    def call(z=p, W=p, dx=p, dz=q, dims=dims, wsp=p, nbytes=ws, fl=0):
        return lib.stgcn_vit_patch_embed_backward(z, W, dx, q, q, q, q, dz, *dims, wsp, nbytes, fl, None)
    name = b"stgcn_vit_patch_embed_backward:"
    # 1. flags, before the pointers are looked at
    assert call(z=None, fl=0x100) == ERR_ARG and b"STGCN_IN_NTVC" in lib.stgcn_last_error() and name in lib.stgcn_last_error()
    # 2. pointers, dimensions, alignment - before coverage (the bf16 arithmetic is not covered)
    for kw in (dict(z=None), dict(W=None), dict(dx=None), dict(wsp=None)):
        assert call(fl=2, **kw) == ERR_ARG and b"NULL" in lib.stgcn_last_error(), kw
    assert call(fl=2, dims=(2, 128, 181, 22, 20, 2, 512)) == ERR_ARG and b"whole patches" in lib.stgcn_last_error()
    for kw in (dict(z=odd), dict(W=odd), dict(dx=odd), dict(wsp=odd)):
        assert call(fl=2, **kw) == ERR_ARG and b"16-byte" in lib.stgcn_last_error(), kw
    assert call(fl=2, dz=p) == ERR_ARG and b"alias" in lib.stgcn_last_error()
    # 3. coverage - before the workspace
    assert call(fl=2, nbytes=0) == ERR_UNSUPPORTED and b"math" in lib.stgcn_last_error()
    assert call(dims=(2, 24, 8, 6, 4, 2, 64), nbytes=0) == ERR_UNSUPPORTED
    # 4. the workspace
    for fl in (0, BF16X3, IN_NTVC):
        need = lib.stgcn_vit_patch_embed_backward_ws_bytes(*dims, fl)
        assert call(fl=fl, nbytes=need - 1) == ERR_WORKSPACE and f"< {need} bytes".encode() in lib.stgcn_last_error()


def test_classifier_backward_answers_in_the_documented_order(lib):
    buf, p, q, odd = _host()
    dims = (2, 100, 512, 14)
    ws = lib.stgcn_vit_pool_classify_backward_ws_bytes(*dims, POOL_CLS)

    def call(x=p, lnw=p, lnb=p, W=p, dl=p, dx=q, dims=dims, wsp=p, nbytes=ws, fl=POOL_CLS):
        return lib.stgcn_vit_pool_classify_backward(x, lnw, lnb, 1e-5, W, dl, dx, q, q, q, q, *dims, wsp, nbytes, fl, None)
    name = b"stgcn_vit_pool_classify_backward:"
    assert call(x=None, fl=0x40) == ERR_ARG and b"unknown flag" in lib.stgcn_last_error() and name in lib.stgcn_last_error()
    assert call(x=None, fl=POOL_MAX | POOL_CLS) == ERR_ARG and b"exclude each other" in lib.stgcn_last_error()
    for kw in (dict(x=None), dict(lnw=None), dict(lnb=None), dict(W=None), dict(dl=None), dict(wsp=None)):
        assert call(fl=POOL_MAX, **kw) == ERR_ARG and b"NULL" in lib.stgcn_last_error(), kw
    for kw in (dict(x=odd), dict(dx=odd), dict(wsp=odd)):
        assert call(fl=POOL_MAX, **kw) == ERR_ARG and b"16-byte" in lib.stgcn_last_error(), kw
    assert call(fl=POOL_MAX, nbytes=0) == ERR_UNSUPPORTED and b"STGCN_VIT_POOL_MAX" in lib.stgcn_last_error()
    assert call(dims=(2, 100, 96, 14), nbytes=0) == ERR_UNSUPPORTED
    for fl in (0, POOL_CLS):
        assert call(fl=fl, nbytes=ws - 1) == ERR_WORKSPACE and f"< {ws} bytes".encode() in lib.stgcn_last_error()


def test_the_ends_do_not_train_on_hip_on_the_cpu_when_switched_off_with_dropout_or_under_the_threshold(monkeypatch):
    from stgcn_amd import set_hip_min_tokens
    from stgcn_amd.vit import VIT_HIP_TRAIN_MIN_TOKENS, ViT
    for k in ("STGCN_VIT_TRAIN", "STGCN_VIT_TRAIN_ENDS"):
        monkeypatch.delenv(k, raising=False)
    torch.manual_seed(0)
    vit = ViT(time_len=8, joint=6, p1=4, p2=2, num_classes=5, dim=64, depth=1, heads=2, mlp_dim=64, channels=32, dim_head=32, emb_dropout=0.5)
    assert vit.hip_train_min_tokens == ViT.DEFAULT_HIP_TRAIN_MIN_TOKENS >= VIT_HIP_TRAIN_MIN_TOKENS
    set_hip_min_tokens(vit, 0)
    z = torch.randn(3, 32, 8, 6, requires_grad=True)
    x = torch.randn(3, 7, 64, requires_grad=True)
    assert not vit.embed_trains_on_hip(z) and not vit.head_trains_on_hip(x), "CPU tensors"
    vit(z).sum().backward()
    assert z.grad is not None and all(p.grad is not None for p in vit.parameters())

    # the remaining conditions, with the device check answered for a GPU: what is left is host logic
    class OnGpu(torch.Tensor):
        is_cuda = True
    zg, xg = z.detach().as_subclass(OnGpu).requires_grad_(), x.detach().as_subclass(OnGpu).requires_grad_()
    vit.eval()                                         # emb_dropout inactive
    assert vit.embed_trains_on_hip(zg) and vit.head_trains_on_hip(xg)
    with torch.no_grad():
        assert not vit.embed_trains_on_hip(zg) and not vit.head_trains_on_hip(xg), "nothing recorded"
    vit.train()
    assert not vit.embed_trains_on_hip(zg) and vit.head_trains_on_hip(xg), "an active emb_dropout keeps the embedding on torch ops"
    vit.dropout.p = 0.0
    assert vit.embed_trains_on_hip(zg)
    vit.hip_train_min_tokens = 22
    assert not vit.embed_trains_on_hip(zg) and not vit.head_trains_on_hip(xg), "21 tokens under a threshold of 22"
    vit.hip_train_min_tokens = 21
    assert vit.embed_trains_on_hip(zg) and vit.head_trains_on_hip(xg)
    for key in ("STGCN_VIT_TRAIN_ENDS", "STGCN_VIT_TRAIN"):
        monkeypatch.setenv(key, "0")
        assert not vit.embed_trains_on_hip(zg) and not vit.head_trains_on_hip(xg), key
        monkeypatch.delenv(key)
    assert vit.embed_trains_on_hip(zg) and vit.head_trains_on_hip(xg)
    vit.force_torch = True
    assert not vit.embed_trains_on_hip(zg) and not vit.head_trains_on_hip(xg)
