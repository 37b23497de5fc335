"""The ST-ViT head (``stgcn_amd.vit``, ``stgcn_vit_patch_embed``, ``STGCN_VIT_POOL_CLS``), host side (no GPU): the drop-in
name, layout and seeded init against the reference fixture, the torch-op path on CPU against the fixture's logits and the fp64
restatement, the plan's answers through the queries, the workspace of the two layouts, and the argument errors reached before
any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import altformer_ref as ar
import stvit_ref as sr
from _util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
IN_NTVC, POOL_MAX, POOL_CLS, BF16X3 = 0x40, 0x4000000, 0x8000000, 1
NEW_NAMES = ["stgcn_vit_patch_embed_supported", "stgcn_vit_patch_embed_ws_bytes", "stgcn_vit_patch_embed_cut", "stgcn_vit_patch_embed"]
REAL = (128, 180, 22, 20, 2, 512)     # C, T, V, p1, p2, E of the reference configuration


@pytest.fixture(scope="module")
def lib():
    from stgcn_amd import _capi
    return _capi.lib()


@pytest.fixture(scope="module")
def golden():
    return load_golden("stvit_reference")


@pytest.fixture(scope="module")
def model():
    from stgcn_amd.vit import ViT
    torch.manual_seed(sr.MODEL_SEED)
    return ViT(**sr.CONFIG).eval()


def test_shim_resolves_to_the_package():
    import stgcn_amd.vit as vit
    from model.ST_Vit import trans
    for name in ("ViT", "Transformer", "Attention", "FeedForward", "PreNorm"):
        assert getattr(trans, name) is getattr(vit, name), name
    assert not os.path.exists(os.path.join(ROOT, "st-gcn-altformer_amd", "model", "ST_Vit", "__init__.py"))
    src = open(vit.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+einops", src, flags=re.M)


def test_header_binding_and_library_agree(lib):
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    from stgcn_amd.build import SOURCES
    assert "vit_patch.hip" in SOURCES
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(STGCN_\w+)\s+\(?0x([0-9A-Fa-f]+)u\b", hdr)}
    assert defs["STGCN_VIT_POOL_CLS"] == POOL_CLS == _capi.VIT_POOL_CLS
    assert all(POOL_CLS & v == 0 for k, v in defs.items() if k != "STGCN_VIT_POOL_CLS"), "collides with a flag of the header"
    for n in NEW_NAMES:
        assert re.search(rf"\b(int|size_t)\s+{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(lib, n), n
    P, I, U, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
    assert _capi.PROTOTYPES["stgcn_vit_patch_embed"] == (I, [P] * 6 + [I] * 7 + [P, Z, U, P])
    assert _capi.PROTOTYPES["stgcn_vit_patch_embed_ws_bytes"] == (Z, [I] * 7 + [U])
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr) and lib.stgcn_version() == 11, "additive: the ABI version stays"
    assert callable(F.vit_patch_embed)


def test_layout_and_seeded_init_equal_the_reference(golden, model):
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in golden["keys"]]
    for i, (k, v) in enumerate(sd.items()):
        assert list(v.shape) == list(golden["shapes"][i][:golden["ndim"][i]]), k
        assert v.double().sum().item() == pytest.approx(golden["sums"][i], rel=1e-12, abs=1e-12), k
        ix = np.resize(ar.sample_idx(v.numel(), len(golden["sample_idx"][i]), sr.MODEL_SEED + i).numpy(), len(golden["sample_idx"][i]))
        assert np.array_equal(ix, golden["sample_idx"][i]), k
        assert np.array_equal(v.reshape(-1)[torch.from_numpy(ix).long()].numpy(), golden["sample_val"][i]), k
    for want in ("to_patch_embedding.1.weight", "to_patch_embedding.1.bias", "pos_embedding", "cls_token",
                 "transformer.layers.5.0.norm.weight", "transformer.layers.0.0.fn.to_qkv.weight", "transformer.layers.0.0.fn.to_out.0.bias",
                 "transformer.layers.3.1.norm.bias", "transformer.layers.3.1.fn.net.0.weight", "transformer.layers.3.1.fn.net.3.bias",
                 "mlp_head.0.weight", "mlp_head.1.bias"):
        assert want in sd, want
    assert "transformer.layers.0.0.fn.to_qkv.bias" not in sd
    assert not list(model.to_patch_embedding[0].parameters()), "index 0 carries no parameters: the Linear stays .1"


def test_fixture_state_strict_loads(model):
    from stgcn_amd.vit import ViT
    other = ViT(**sr.CONFIG)
    missing = other.load_state_dict(model.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    # a layer still unpacks as the reference's ModuleList does
    attn, ff = other.transformer.layers[0]
    assert attn.fn.heads == sr.CONFIG["heads"] and ff.fn.net[0].out_features == sr.CONFIG["mlp_dim"]


def test_torch_path_on_cpu_matches_fixture_and_fp64(golden):
    """Two fp32 evaluations of one formula (the reference's ops and ours, in a different order) each sit within the reference's
    own fp32-against-fp64 floor of the fp64 value, so ours is held to 4 x that floor against the fixture's fp64 results (a
    factor for the different summation order and thread count, well inside the project's 1e-4), and the fp64 restatement to
    1e-9 of the fixture's fp64 results."""
    from stgcn_amd.vit import ViT
    torch.manual_seed(sr.MODEL_SEED)
    model = sr.prepare(ViT(**sr.CONFIG).eval())
    z = sr.make_input()
    assert np.array_equal(z.reshape(-1)[ar.sample_idx(z.numel(), 16, sr.INPUT_SEED + 2).long()].numpy(), golden["z_samples"])
    assert not model.uses_hip(z)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    eidx = torch.from_numpy(golden["embed_idx"]).long()
    with torch.no_grad():
        emb = model.embed(z)
    assert list(emb.shape) == list(golden["embed_shape"])
    err = np.abs(emb.reshape(-1)[eidx].double().numpy() - golden["embed_val_f64"]).max() / float(golden["embed_max"])
    print(f"embedding: ours fp32 vs reference fp64 {err:.3e}, floor {float(golden['floor_embed']):.3e}")
    assert err <= 4 * float(golden["floor_embed"])
    for pool in ("cls", "mean"):
        model.pool = pool
        with torch.no_grad():
            out = model(z)
        ref64 = golden[f"logits_{pool}_f64"]
        scale, floor = np.abs(ref64).max(), float(golden[f"floor_{pool}"])
        err = np.abs(out.double().numpy() - ref64).max() / scale
        err32 = np.abs(out.numpy() - golden[f"logits_{pool}"]).max() / scale
        l64, e64 = sr.vit64(z, sd, sr.CONFIG["p1"], sr.CONFIG["p2"], sr.CONFIG["depth"], sr.CONFIG["heads"], pool)
        err64 = np.abs(l64.numpy() - ref64).max() / scale
        print(f"pool={pool}: ours vs reference fp64 {err:.3e}, vs reference fp32 {err32:.3e}, floor {floor:.3e}, stvit_ref vs fp64 {err64:.3e}")
        assert err <= 4 * floor and err32 <= 4 * floor
        assert err64 <= 1e-9
        assert np.abs(e64.reshape(-1)[eidx].numpy() - golden["embed_val_f64"]).max() <= 1e-9 * float(golden["embed_max"])


def test_identity_to_out_takes_the_torch_path():
    from stgcn_amd.vit import ViT
    m = ViT(time_len=8, joint=4, p1=4, p2=2, num_classes=3, dim=64, depth=1, heads=1, mlp_dim=64, channels=32, dim_head=64).eval()
    assert isinstance(m.transformer.layers[0][0].fn.to_out, torch.nn.Identity)
    assert m.transformer.layers[0]._parts() is None
    with torch.no_grad():
        assert m(torch.randn(2, 32, 8, 4)).shape == (2, 3)


def test_switches_reach_the_vit():
    from stgcn_amd import altformer, vit
    m = vit.ViT(time_len=8, joint=4, p1=4, p2=2, num_classes=3, dim=64, depth=2, heads=1, mlp_dim=64, channels=32)
    subs = [m] + list(m.transformer.layers)
    assert all(isinstance(s, altformer.HipSwitches) for s in subs) and isinstance(altformer.Block(64, 1), altformer.HipSwitches)
    assert all(s.hip_min_tokens == vit.VIT_HIP_MIN_TOKENS and s.small_tiles is vit.VIT_SMALL_TILES and s.math_mode is None for s in subs)
    altformer.set_hip_min_tokens(m, 0)
    altformer.set_head_math(m, "bf16")
    assert all(s.hip_min_tokens == 0 and s.math_mode == altformer.HEAD_MATH["bf16"] for s in subs)
    altformer.set_low_latency(m, min_tokens=7, split_attention=True)
    assert all(s.small_tiles and s.split_attention and s.hip_min_tokens == 7 for s in subs)
    altformer.set_low_latency(m, enabled=False)
    assert all(s.small_tiles is vit.VIT_SMALL_TILES and not s.split_attention and s.hip_min_tokens == vit.VIT_HIP_MIN_TOKENS for s in subs)
    # one flag-word helper: the layer's word is the Block's for the same settings
    altformer.set_head_math(m, "mixed")
    blk = altformer.Block(512, 8)
    blk.math_mode, blk.small_tiles = altformer.HEAD_MATH["mixed"], True
    m.transformer.layers[0].small_tiles = True
    assert m.transformer.layers[0]._inference_flags(100, 512, 8, 512) == blk._inference_flags(100, 512, 8, 512)
    assert vit.Layer._inference_flags is altformer.Block._inference_flags is altformer.HipSwitches._inference_flags


def test_queries_are_pure_host_functions(lib):
    from stgcn_amd import functional as F
    C, T, V, p1, p2, E = REAL
    for N in (1, 2, 8, 32, 128):
        for fl in (0, BF16X3, IN_NTVC, BF16X3 | IN_NTVC):
            a = (lib.stgcn_vit_patch_embed_supported(N, C, T, V, p1, p2, E, fl), lib.stgcn_vit_patch_embed_ws_bytes(N, C, T, V, p1, p2, E, fl),
                 lib.stgcn_vit_patch_embed_cut(N, C, T, V, p1, p2, E, fl))
            b = (lib.stgcn_vit_patch_embed_supported(N, C, T, V, p1, p2, E, fl), lib.stgcn_vit_patch_embed_ws_bytes(N, C, T, V, p1, p2, E, fl),
                 lib.stgcn_vit_patch_embed_cut(N, C, T, V, p1, p2, E, fl))
            assert a == b and a[0] == 1 and a[1] > 0 and a[2] > 0
    # the cut is the plan's: one clip (99 rows, 5120 deep) is cut across workgroups, and the cut depends on (N n, K, E) only
    tile, parts = F.vit_patch_embed_cut(1, C, T, V, p1, p2, E)
    assert parts > 1 and tile in (32, 64, 128)
    assert F.vit_patch_embed_cut(1, C, T, V, p1, p2, E, channels_last=True) == (tile, parts)
    assert F.vit_patch_embed_cut(1, 256, 180, 11, 20, 1, E) == F.vit_patch_embed_cut(1, C, T, V, p1, p2, E), "same (N n, K, E)"
    # cases of the GPU tests
    for name, (N, c, t, v, q1, q2, e) in sr.EMBED_CASES.items():
        for fl in (0, BF16X3, IN_NTVC, BF16X3 | IN_NTVC):
            assert lib.stgcn_vit_patch_embed_supported(N, c, t, v, q1, q2, e, fl) == 1, name
    assert F.vit_patch_embed_cut(*sr.EMBED_CASES["b_K5120_rows4"])[1] > 1, "case (b) exercises the cut"
    assert {F.vit_patch_embed_cut(*c)[0] for c in sr.EMBED_CASES.values()} == {32, 64, 128}, "the cases reach every tile form"
    # not whole patches, a run that a chunk of 32 would cross, a math value without a kernel, an unknown flag
    for args in ((1, C, 181, V, p1, p2, E, 0), (1, C, T, 23, p1, p2, E, 0), (1, 24, T, V, p1, p2, E, 0), (1, C, T, V, p1, p2, E, 2),
                 (1, C, T, V, p1, p2, E, 0x80), (0, C, T, V, p1, p2, E, 0), (1, C, T, V, 0, p2, E, 0)):
        assert lib.stgcn_vit_patch_embed_supported(*args) == 0 and lib.stgcn_vit_patch_embed_ws_bytes(*args) == 0, args
    assert lib.stgcn_vit_patch_embed_supported(1, 16, T, V, p1, p2, E, 0) == 1, "(p2 C) % 32 == 0 is the rule, not C % 32"


def test_ntvc_workspace_holds_no_rearranged_copy(lib):
    C, T, V, p1, p2, E = REAL
    n, K = (T // p1) * (V // p2), p1 * p2 * C
    for N in (1, 2, 8, 32, 128):
        for math in (0, BF16X3):
            ntvc = lib.stgcn_vit_patch_embed_ws_bytes(N, C, T, V, p1, p2, E, math | IN_NTVC)
            nchw = lib.stgcn_vit_patch_embed_ws_bytes(N, C, T, V, p1, p2, E, math)
            parts = lib.stgcn_vit_patch_embed_cut(N, C, T, V, p1, p2, E, math | IN_NTVC) & 0xFFFF
            copy = N * n * K * 4
            assert ntvc == -(-parts * N * n * E * 4 // 256) * 256, "the parts' sums, (N n, E) each, and nothing else: no K in it"
            assert nchw - ntvc == -(-copy // 256) * 256, "channels-first input adds exactly the one transposed copy"


def test_refusal_order(lib):
    """Flags, then pointers and dimensions, then coverage, then the workspace; each answered with nothing launched (the
    pointers are host addresses: a launch would not survive them)."""
    from stgcn_amd import _capi
    C, T, V, p1, p2, E = REAL
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    z, W, b, cls, pos, x, ws = (ctypes.c_void_p(a + 256 * i) for i in range(7))
    null = ctypes.c_void_p(0)

    def call(z=z, W=W, b=b, cls=cls, pos=pos, x=x, dims=(1, C, T, V, p1, p2, E), ws=ws, ws_bytes=1 << 40, flags=0):
        return lib.stgcn_vit_patch_embed(z, W, b, cls, pos, x, *dims, ws, ctypes.c_size_t(ws_bytes), flags, null)

    # everything wrong at once: the flags answer first
    assert call(z=null, dims=(1, 24, T, V, p1, p2, E), ws_bytes=0, flags=0x80) == ERR_ARG
    assert b"STGCN_IN_NTVC" in lib.stgcn_last_error()
    for bit in (0x10, 0x80, 0x1000, POOL_CLS, _capi.VIT_BF16, _capi.VIT_TILE_AUTO):
        assert call(flags=bit) == ERR_ARG
    # pointers and dimensions before coverage and workspace
    for kw in (dict(z=null), dict(W=null), dict(cls=null), dict(x=null), dict(ws=null)):
        assert call(dims=(1, 24, T, V, p1, p2, E), ws_bytes=0, **kw) == ERR_ARG, kw
    for dims in ((0, C, T, V, p1, p2, E), (1, C, T, V, p1, 0, E), (1, C, 181, V, p1, p2, E), (1, 24, T, 23, p1, p2, E)):
        assert call(dims=dims, ws_bytes=0) == ERR_ARG, dims
    assert call(z=ctypes.c_void_p(a + 4), dims=(1, 24, T, V, p1, p2, E)) == ERR_ARG, "alignment is an argument error"
    assert call(x=z) == ERR_ARG
    # coverage before the workspace
    assert call(dims=(1, 24, T, V, p1, p2, E), ws_bytes=0) == ERR_UNSUPPORTED
    assert call(flags=2, ws_bytes=0) == ERR_UNSUPPORTED, "a math value without a kernel is a coverage answer"
    # the workspace last; bias and pos may be NULL
    need = lib.stgcn_vit_patch_embed_ws_bytes(1, C, T, V, p1, p2, E, 0)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(b=null, pos=null, ws_bytes=0, flags=IN_NTVC | BF16X3) == ERR_WORKSPACE


def test_pool_cls_flag_is_checked_first(lib):
    null = ctypes.c_void_p(0)
    for flags in (POOL_CLS | POOL_MAX,):
        assert lib.stgcn_vit_pool(null, null, 1, 1, 64, flags, null) == ERR_ARG
        assert b"exclude" in lib.stgcn_last_error()
        assert lib.stgcn_vit_pool_classify(null, null, null, ctypes.c_float(1e-5), null, null, null, 1, 1, 64, 1, flags, null) == ERR_ARG
        assert b"exclude" in lib.stgcn_last_error()
    # the bit alone passes the flag check (the NULL pointers answer next)
    assert lib.stgcn_vit_pool(null, null, 1, 1, 64, POOL_CLS, null) == ERR_ARG and b"NULL" in lib.stgcn_last_error()
    from stgcn_amd import functional as F
    with pytest.raises(ValueError):
        F.vit_pool(torch.zeros(1, 1, 64), mode="first")
