"""The whole AltFormer head in one call (``stgcn_altformer_head_forward``, ``stgcn_vit_pool``, ``stgcn_vit_pool_classify``), host
side (no GPU): the additive C ABI (one flag bit, three structs, seven symbols, ABI 11 unchanged), the plan's answers through
the two queries, the argument errors reached before any launch, and the Python switch (``set_whole_head``)."""
import ctypes
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["stgcn_vit_pool_supported", "stgcn_vit_pool", "stgcn_vit_pool_classify_supported", "stgcn_vit_pool_classify",
             "stgcn_altformer_head_supported", "stgcn_altformer_head_ws_bytes", "stgcn_altformer_head_forward"]
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
EMBED_TS, IN_NTVC, POOL_MAX = 0x100, 0x40, 0x4000000
# (T, V) of SHREC, DHG and LMDHG
DATASETS = {"shrec": (180, 22), "dhg": (150, 22), "lmdhg": (200, 46)}


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


def shape(N=1, T=180, V=22, C=128, E1=256, E2=512, heads=8, hidden1=None, hidden2=None, depth1=6, depth2=6, classes=14):
    from stgcn_amd import _capi
    return _capi.AltformerHeadShape(N, T, V, C, E1, E2, heads, hidden1 or 2 * E1, hidden2 or 2 * E2, depth1, depth2, classes)


def test_header_binding_and_library_agree(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.build import SOURCES, build
    assert "vit_head.hip" in SOURCES
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    assert re.search(r"#define\s+STGCN_VIT_POOL_MAX\s+\(0x4000000u\)", hdr)
    defs = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(STGCN_\w+)\s+\(?0x([0-9A-Fa-f]+)u\b", hdr)}
    assert defs["STGCN_VIT_POOL_MAX"] == POOL_MAX == _capi.VIT_POOL_MAX
    assert all(POOL_MAX & v == 0 for k, v in defs.items() if k != "STGCN_VIT_POOL_MAX"), "collides with a flag of the header"
    assert POOL_MAX & (0x400000 | 0x1000000) == 0, "the two bits that host tests use as unknown ones stay unassigned"
    assert defs["STGCN_EMBED_TS"] == EMBED_TS == _capi.EMBED_TS and defs["STGCN_IN_NTVC"] == IN_NTVC == _capi.IN_NTVC
    handle = ctypes.CDLL(build())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW_NAMES:
        assert re.search(rf"\b(int|size_t)\s+{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
        assert n in integration, n
    P, I, Fl, U, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint, ctypes.c_size_t
    SP, WP = ctypes.POINTER(_capi.AltformerHeadShape), ctypes.POINTER(_capi.AltformerHeadWeights)
    assert _capi.PROTOTYPES["stgcn_vit_pool_supported"] == (I, [I] * 3)
    assert _capi.PROTOTYPES["stgcn_vit_pool"] == (I, [P, P, I, I, I, U, P])
    assert _capi.PROTOTYPES["stgcn_vit_pool_classify_supported"] == (I, [I] * 4)
    assert _capi.PROTOTYPES["stgcn_vit_pool_classify"] == (I, [P, P, P, Fl, P, P, P, I, I, I, I, U, P])
    assert _capi.PROTOTYPES["stgcn_altformer_head_supported"] == (I, [SP, U, U, U])
    assert _capi.PROTOTYPES["stgcn_altformer_head_ws_bytes"] == (Z, [SP, U, U, U])
    assert _capi.PROTOTYPES["stgcn_altformer_head_forward"] == (I, [P, WP, SP, Fl, Fl, Fl, Fl, P, Z, P, U, U, U, P])
    # the mirrors have the header's fields in the header's order
    for name, cls in (("stgcn_vit_block_weights", _capi.VitBlockWeights), ("stgcn_altformer_head_shape", _capi.AltformerHeadShape),
                      ("stgcn_altformer_head_weights", _capi.AltformerHeadWeights)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f for f in re.findall(r"\*?\s*(\w+)\s*[,;]", body)]
        assert fields == [f for f, _ in cls._fields_], name
    assert ctypes.sizeof(_capi.VitBlockWeights) == 12 * ctypes.sizeof(P) and ctypes.sizeof(_capi.AltformerHeadShape) == 12 * 4
    assert ctypes.sizeof(_capi.AltformerHeadWeights) == 12 * ctypes.sizeof(P)
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11
    assert callable(F.vit_pool) and callable(F.vit_pool_classify) and callable(F.altformer_head_forward)


def test_kernel_queries(lib):
    for S, L, D in ((7, 1, 64), (22, 180, 256), (5760, 22, 256), (3, 5, 4), (1, 1, 100)):
        assert lib.stgcn_vit_pool_supported(S, L, D) == 1
    for S, L, D in ((0, 1, 64), (1, 0, 64), (1, 1, 0), (1, 1, 66), (1, 1, 2)):
        assert lib.stgcn_vit_pool_supported(S, L, D) == 0
    for N, L, D, classes in ((1, 1, 64, 1), (5, 180, 512, 14), (5, 22, 512, 28), (1, 257, 128, 3), (2, 4096, 4096, 1000)):
        assert lib.stgcn_vit_pool_classify_supported(N, L, D, classes) == 1
    for N, L, D, classes in ((0, 1, 64, 1), (1, 0, 64, 1), (1, 1, 64, 0), (1, 1, 96, 14), (1, 1, 32, 14), (1, 1, 4160, 14)):
        assert lib.stgcn_vit_pool_classify_supported(N, L, D, classes) == 0


@pytest.mark.parametrize("classes", [14, 28])
@pytest.mark.parametrize("ts", [False, True], ids=["ST", "TS"])
@pytest.mark.parametrize("data", sorted(DATASETS))
def test_supported_and_sized_for_the_datasets(data, ts, classes, lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    T, V = DATASETS[data]
    hf = EMBED_TS if ts else 0
    for N in (1, 32):
        s = shape(N=N, T=T, V=V, classes=classes)
        for f1, f2 in itertools.product((0, HEAD_MATH["mixed"], HEAD_MATH["mixed"] | _capi.VIT_TILE_AUTO | _capi.VIT_ATTN_SPLIT,
                                         HEAD_MATH["bf16"]), repeat=2):
            for extra in (0, IN_NTVC):
                assert lib.stgcn_altformer_head_supported(s, f1, f2, hf | extra) == 1
                assert lib.stgcn_altformer_head_ws_bytes(s, f1, f2, hf | extra) > 0
    assert F.altformer_head_supported(1, T, V, 128, 256, 512, 8, 512, 1024, 6, 6, classes, "TS" if ts else "ST")
    assert F._head_ws_bytes(shape(T=T, V=V, classes=classes), 0, 0, hf) == lib.stgcn_altformer_head_ws_bytes(
        shape(T=T, V=V, classes=classes), 0, 0, hf) > 0


def test_unsupported_shapes_and_refused_flags(lib):
    from stgcn_amd import _capi
    ok = shape()
    assert lib.stgcn_altformer_head_supported(ok, 0, 0, 0) == 1
    # head_dim 48 in either stage
    for bad in (shape(E1=384), shape(E2=384), shape(E1=384, E2=768)):
        for hf in (0, EMBED_TS):
            assert lib.stgcn_altformer_head_supported(bad, 0, 0, hf) == 0 and lib.stgcn_altformer_head_ws_bytes(bad, 0, 0, hf) == 0
    # a sequence above STGCN_VIT_MAX_STREAM_L: the frames of TS's first stage and of ST's second stage, the joints the other way
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    max_l = int(re.search(r"#define\s+STGCN_VIT_MAX_STREAM_L\s+(\d+)", hdr).group(1))
    for hf in (0, EMBED_TS):
        assert lib.stgcn_altformer_head_supported(shape(T=max_l), 0, 0, hf) == 1
        assert lib.stgcn_altformer_head_supported(shape(T=max_l + 1), 0, 0, hf) == 0
        assert lib.stgcn_altformer_head_supported(shape(V=max_l + 1), 0, 0, hf) == 0
    # the bf16 mode has a resident form only: 300 frames are covered without it and not with it
    assert lib.stgcn_altformer_head_supported(shape(T=300), 0, 0, EMBED_TS) == 1
    assert lib.stgcn_altformer_head_supported(shape(T=300), _capi.VIT_BF16, 0, EMBED_TS) == 0
    assert lib.stgcn_altformer_head_supported(shape(T=300), 0, _capi.VIT_BF16, EMBED_TS) == 1    # stage 2 runs over the joints
    # a flag word that stgcn_vit_block_forward refuses, in either stage; unknown head flags; empty dimensions
    for word in (_capi.VIT_TRAIN_BF16, _capi.VIT_BF16 | _capi.VIT_QKV_F32, _capi.VIT_TRAIN_ATTN_BF16):
        assert lib.stgcn_altformer_head_supported(ok, word, 0, 0) == 0 and lib.stgcn_altformer_head_supported(ok, 0, word, 0) == 0
    for hf in (0x80, POOL_MAX, 0x400000):
        assert lib.stgcn_altformer_head_supported(ok, 0, 0, hf) == 0
    for field in ("N", "T", "V", "C", "E1", "E2", "heads", "hidden1", "hidden2", "depth1", "depth2", "classes"):
        s = shape()
        setattr(s, field, 0)
        assert lib.stgcn_altformer_head_supported(s, 0, 0, 0) == 0 and lib.stgcn_altformer_head_ws_bytes(s, 0, 0, 0) == 0
    assert lib.stgcn_altformer_head_supported(shape(N=65536), 0, 0, 0) == 0
    assert lib.stgcn_altformer_head_supported(None, 0, 0, 0) == 0 and lib.stgcn_altformer_head_ws_bytes(None, 0, 0, 0) == 0


@pytest.mark.parametrize("ts", [False, True], ids=["ST", "TS"])
def test_workspace_grows_with_the_batch_and_its_block_part_is_bounded(ts, lib):
    hf = EMBED_TS if ts else 0
    T, V, E1, E2 = 180, 22, 256, 512
    size = {N: lib.stgcn_altformer_head_ws_bytes(shape(N=N), 0, 0, hf) for N in (1, 2, 8, 9, 32, 64)}
    assert all(v > 0 for v in size.values())
    assert list(size.values()) == sorted(size.values()), "the workspace does not shrink when N grows"
    # per clip: two activation buffers of each stage and the pooled rows (every piece a multiple of the carve's 256 bytes here)
    L2 = V if ts else T
    per_clip = 4 * (2 * T * V * E1 + L2 * E1 + 2 * L2 * E2)
    # at 32 and at 64 clips stage 1 walks full slabs (126,720 tokens and more against 32,768) and its block workspace is the
    # larger one: the block term is the same, the rest is linear in N
    block = {N: size[N] - N * per_clip for N in (32, 64)}
    assert block[32] == block[64] > 0
    assert block[32] == max(lib.stgcn_vit_block_ws_bytes(32 * L2, T * V // L2, E1, 2 * E1), lib.stgcn_vit_block_ws_bytes(32, L2, E2, 2 * E2))
    assert size[1] - per_clip == max(lib.stgcn_vit_block_ws_bytes(L2, T * V // L2, E1, 2 * E1), lib.stgcn_vit_block_ws_bytes(1, L2, E2, 2 * E2))


def test_entry_point_errors_before_any_launch(lib):
    """Flags before pointers, pointers before coverage, coverage before the workspace; none of these needs a device (the
    pointers are never dereferenced)."""
    from stgcn_amd import _capi
    P = ctypes.c_void_p
    fake = P(0x1000)
    blocks = (_capi.VitBlockWeights * 6)(*[_capi.VitBlockWeights(*([fake] * 12)) for _ in range(6)])
    w = _capi.AltformerHeadWeights(fake, fake, fake, blocks, fake, fake, fake, blocks, fake, fake, fake, fake)

    def fwd(z=fake, weights=w, s=None, ws=fake, nbytes=1 << 40, logits=fake, f1=0, f2=0, hf=0):
        rc = lib.stgcn_altformer_head_forward(z, weights, s if s is not None else shape(), 1e-6, 1e-5, 0.125, 0.125, ws, nbytes,
                                              logits, f1, f2, hf, None)
        return rc, (lib.stgcn_last_error() or b"").decode()

    # flags first: with every pointer NULL the answer still names the flag
    rc, msg = fwd(z=None, weights=None, ws=None, logits=None, hf=0x80)
    assert rc == ERR_ARG and "head_flags" in msg
    rc, msg = fwd(z=None, weights=None, ws=None, logits=None, f1=_capi.VIT_TRAIN_BF16)
    assert rc == ERR_ARG and "STGCN_VIT_TRAIN_BF16" in msg
    rc, msg = fwd(z=None, f2=_capi.VIT_BF16 | _capi.VIT_QKV_F32)
    assert rc == ERR_ARG and "exclude each other" in msg
    # pointers before coverage (head_dim 48 would be STGCN_ERR_UNSUPPORTED)
    for kw in (dict(z=None), dict(weights=None), dict(ws=None), dict(logits=None)):
        assert fwd(s=shape(E1=384), **kw)[0] == ERR_ARG
    for field, _ in _capi.AltformerHeadWeights._fields_:
        if field in ("pos1", "pos2", "head_bias"):
            continue
        w2 = _capi.AltformerHeadWeights(fake, fake, fake, blocks, fake, fake, fake, blocks, fake, fake, fake, fake)
        setattr(w2, field, None)
        assert fwd(weights=w2)[0] == ERR_ARG, field
    hole = (_capi.VitBlockWeights * 6)(*[_capi.VitBlockWeights(*([fake] * 12)) for _ in range(6)])
    hole[5].W2 = None
    w3 = _capi.AltformerHeadWeights(fake, fake, fake, blocks, fake, fake, fake, hole, fake, fake, fake, fake)
    assert fwd(weights=w3)[0] == ERR_ARG
    zero = shape()
    zero.depth2 = 0
    assert fwd(s=zero)[0] == ERR_ARG
    # coverage before the workspace
    rc, msg = fwd(s=shape(E1=384), nbytes=0)
    assert rc == ERR_UNSUPPORTED and "head_dim" in msg
    assert fwd(s=shape(T=4097), nbytes=0, hf=EMBED_TS)[0] == ERR_UNSUPPORTED
    assert fwd(s=shape(N=65536), nbytes=0)[0] == ERR_UNSUPPORTED
    # the workspace last
    need = lib.stgcn_altformer_head_ws_bytes(shape(), 0, 0, 0)
    rc, msg = fwd(nbytes=need - 8)
    assert rc == ERR_WORKSPACE and str(need) in msg
    # the two kernels' entry points
    assert lib.stgcn_vit_pool(fake, fake, 3, 5, 64, 0x80, None) == ERR_ARG
    assert lib.stgcn_vit_pool(None, fake, 3, 5, 64, 0, None) == ERR_ARG and lib.stgcn_vit_pool(fake, None, 3, 5, 64, POOL_MAX, None) == ERR_ARG
    assert lib.stgcn_vit_pool(fake, fake, 0, 5, 64, 0, None) == ERR_ARG
    assert lib.stgcn_vit_pool(P(0x1004), fake, 3, 5, 64, 0, None) == ERR_ARG
    assert lib.stgcn_vit_pool(fake, fake, 3, 5, 66, 0, None) == ERR_UNSUPPORTED
    cls = lambda *a: lib.stgcn_vit_pool_classify(*a)   # noqa: E731
    assert cls(fake, fake, fake, 1e-5, fake, fake, fake, 2, 5, 64, 14, 0x1, None) == ERR_ARG
    assert cls(None, fake, fake, 1e-5, fake, fake, fake, 2, 5, 64, 14, 0, None) == ERR_ARG
    assert cls(fake, fake, fake, 1e-5, fake, fake, fake, 2, 5, 64, 0, 0, None) == ERR_ARG
    assert cls(fake, fake, fake, 1e-5, fake, fake, fake, 2, 5, 96, 14, POOL_MAX, None) == ERR_UNSUPPORTED


def small_head(cls_name, **kw):
    from stgcn_amd import altformer
    torch.manual_seed(11)
    cfg = dict(num_frame=12, num_joints=5, in_chans=16, embed_dim_ratio=64, depth=1, num_heads=2, mlp_ratio=2., qkv_bias=True,
               drop_path_rate=0.1)
    cfg.update(kw)
    return getattr(altformer, cls_name)(14, **cfg).eval()


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_switch_leaves_a_cpu_model_alone(cls_name):
    import stgcn_amd
    from stgcn_amd.altformer import _Head
    head = small_head(cls_name)
    assert head.whole_head is False and "set_whole_head" in stgcn_amd.__all__
    z = torch.randn(3, 16, 12, 5)
    with torch.no_grad():
        want = head(z)
        stgcn_amd.set_whole_head(head)
        assert head.whole_head is True and not head.runs_whole(z)
        assert torch.equal(head(z), want)
        stgcn_amd.set_whole_head(head, False)
        assert head.whole_head is False and torch.equal(head(z), want)
    wrapper = torch.nn.Sequential(head)
    stgcn_amd.set_whole_head(wrapper)
    assert all(m.whole_head for m in wrapper.modules() if isinstance(m, _Head))
    head(z).sum().backward()                       # under autograd, switch on: the per-block forward, every gradient
    assert head.mlp_head[1].weight.grad is not None
