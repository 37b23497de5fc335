"""AltFormer heads' training path, host side (no GPU): the C ABI of the training entry points, the module's torch path against
the reference's gradient fixture and the fp64 restatement (tests/altformer_train_ref.py), and the path rule on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import altformer_ref as ar
import altformer_train_ref as tr
from _util import gather_flat, load_golden, parity_gate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_ABI = ["stgcn_vit_linear_backward_supported", "stgcn_vit_linear_backward_ws_bytes", "stgcn_vit_linear_backward",
             "stgcn_vit_attention_backward_supported", "stgcn_vit_attention_backward", "stgcn_vit_layernorm_backward_ws_bytes",
             "stgcn_vit_layernorm_backward", "stgcn_vit_block_train_supported", "stgcn_vit_block_saved_bytes",
             "stgcn_vit_block_backward_ws_bytes", "stgcn_vit_block_forward_train", "stgcn_vit_block_backward"]
HEAD_SHAPES = ((22, 256, 512), (150, 512, 1024), (180, 512, 1024), (180, 256, 512), (46, 512, 1024), (256, 256, 512))


@pytest.fixture(scope="module")
def ref():
    return load_golden("altformer_train_reference")


def test_training_abi_declared_and_exported():
    from stgcn_amd import _capi
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    handle = ctypes.CDLL(build())
    for n in TRAIN_ABI:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr)
    lib = _capi.lib()
    assert _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11
    assert (_capi.VIT_DGELU, _capi.VIT_ACCUMULATE) == (0x4000, 0x8000)
    for name, value in (("STGCN_VIT_DGELU", "0x4000u"), ("STGCN_VIT_ACCUMULATE", "0x8000u"), ("STGCN_VIT_GELU", "0x1000u"),
                        ("STGCN_VIT_QKV_F32", "0x2000u")):
        assert re.search(rf"#define\s+{name}\s+{value}", hdr), name
    for L, D, hidden in HEAD_SHAPES:
        assert lib.stgcn_vit_block_train_supported(L, D, 8, hidden) == 1
        assert lib.stgcn_vit_attention_backward_supported(L, 8, D // 8) == 1
        for M in (32 * L, 1):
            for K, Nout in ((D, 3 * D), (D, D), (D, hidden), (hidden, D)):
                assert lib.stgcn_vit_linear_backward_supported(M, K, Nout, _capi.MATH_BF16X3) == 1
        saved = [lib.stgcn_vit_block_saved_bytes(B, L, D, hidden) for B in (1, 2, 32, 1000)]
        assert saved[0] >= L * (5 * D + 2 * hidden) * 4 and saved == sorted(set(saved)), "saved bytes grow with B"
        assert saved[2] >= 32 * saved[0] - 32 * 5 * 256
        ws = [lib.stgcn_vit_block_backward_ws_bytes(B, L, D, hidden) for B in (1, 2, 32, 100000)]
        assert ws[0] > 0 and ws == sorted(ws) and ws[2] > ws[0], "the backward workspace grows with B up to one slab"
        assert lib.stgcn_vit_block_backward_ws_bytes(200000, L, D, hidden) == ws[3], "and is bounded"
    assert lib.stgcn_vit_block_train_supported(22, 384, 8, 768) == 0          # head_dim 48
    assert lib.stgcn_vit_block_train_supported(257, 256, 8, 512) == 0
    assert lib.stgcn_vit_attention_backward_supported(22, 8, 48) == 0
    for fn in (lib.stgcn_vit_block_saved_bytes, lib.stgcn_vit_block_backward_ws_bytes):
        assert fn(0, 22, 256, 512) == 0 and fn(32, 257, 256, 512) == 0 and fn(32, 22, 256, 500) == 0 and fn(32, 22, 250, 512) == 0
    assert lib.stgcn_vit_linear_backward_supported(100, 250, 768, 0) == 0 and lib.stgcn_vit_linear_backward_ws_bytes(100, 250, 768) == 0
    assert lib.stgcn_vit_linear_backward_supported(100, 256, 768, _capi.MATH_BF16) == 0
    assert lib.stgcn_vit_linear_backward_ws_bytes(1000, 256, 768) > lib.stgcn_vit_linear_backward_ws_bytes(1, 256, 768) > 0
    assert lib.stgcn_vit_layernorm_backward_ws_bytes(0, 256) == 0 < lib.stgcn_vit_layernorm_backward_ws_bytes(10, 256)
    rc = lib.stgcn_vit_block_backward(*([None] * 12), 0, *([None] * 14), 1e-6, 0.1, None, 0, 2, 22, 256, 8, 512, 0, None)
    assert rc == -1 and b"null" in lib.stgcn_last_error().lower()
    rc = lib.stgcn_vit_block_forward_train(*([None] * 15), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, 0, None)
    assert rc == -1 and b"null" in lib.stgcn_last_error().lower()


def stored(ref, key, t):
    """(got, want, scale): ``t`` where the fixture holds samples or the whole tensor; scale = the stored max over the whole."""
    if key in ref:
        return t.detach(), torch.from_numpy(ref[key]), float(ref[key + "_absmax"])
    return gather_flat(t.detach(), ref[key + "_idx"].astype(np.int64)), torch.from_numpy(ref[key + "_val"]), float(ref[key + "_absmax"])


@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_torch_path_and_fp64_restatement_reproduce_the_reference_gradients(name, ref):
    from stgcn_amd.altformer import Block
    pre = f"case.{name}."
    x, dy = ar.make_input(name), tr.make_dy(name)
    assert torch.equal(gather_flat(dy, ref[pre + "dy_idx"].astype(np.int64)), torch.from_numpy(ref[pre + "dy_val"])), \
        "the seeded upstream gradient differs from the one the fixture was made with"
    blk = ar.build_block(Block, name)
    assert not blk.trains_on_hip(x.requires_grad_(True))
    _, g = tr.module_grads(blk, x, dy)
    _, g64 = tr.grads64(x, blk.state_dict(), dy, scale=blk.attn.scale)
    assert set(g) == set(g64) == {k[len(pre) + 1:-len("_absmax")] for k in ref if k.startswith(pre + "d") and k.endswith("_absmax")
                                  and not k.startswith(pre + "dy")}
    for k in sorted(g):
        got, want, scale = stored(ref, pre + "d" + k, g[k])
        err = (got.double() - want.double()).abs().max().item()
        assert err <= 1e-5 * scale, f"{name} d{k}: torch path {err / scale:.3e} of max|ref|"
        # the stored gradients are the reference's fp32 values: its own error (floor_d*) is what separates them from fp64
        got64, _, _ = stored(ref, pre + "d" + k, g64[k])
        floor = float(ref[pre + "floor_d" + k])
        assert floor < 5e-6
        err = (got64 - want.double()).abs().max().item()
        assert err <= max(1e-6, 1.01 * floor) * scale, f"{name} d{k}: fp64 restatement {err / scale:.3e}, floor {floor:.3e}"


def test_fp64_restatement_with_factors_is_the_module_with_those_masks():
    """block64 with the two per-sequence vectors against the module's torch path with DropPath handing out the same masks."""
    from stgcn_amd.altformer import Block, DropPath
    torch.manual_seed(4)
    blk = Block(64, 2, mlp_ratio=2., qkv_bias=True, drop_path=0.1, norm_layer=ar.norm_layer()).train().double()
    x, dy = torch.randn(6, 5, 64).double(), torch.randn(6, 5, 64).double()
    s1, s2 = tr.make_scales(6, 3)
    masks = iter([s1.double().reshape(6, 1, 1), s2.double().reshape(6, 1, 1)])
    blk.drop_path.draw = lambda t: next(masks)
    assert isinstance(blk.drop_path, DropPath)
    y, g = tr.module_grads(blk, x, dy)
    want_y, want = tr.grads64(x, blk.state_dict(), dy, heads=2, s1=s1, s2=s2)
    parity_gate(y, want_y, 1e-12, "masked y")
    for k in want:
        parity_gate(g[k], want[k], 1e-11, f"masked d{k}")


def test_path_rule_and_masks_on_cpu():
    from stgcn_amd.altformer import ST, Block, DropPath, set_hip_min_tokens, set_hip_train_min_tokens
    from test_data_parallel import _replicas
    blk = Block(256, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.25).train()
    set_hip_min_tokens(blk, 0)
    assert blk.hip_min_tokens == 0 and blk.hip_train_min_tokens == 0
    set_hip_train_min_tokens(blk, 7)
    assert blk.hip_min_tokens == 0 and blk.hip_train_min_tokens == 7
    blk.hip_train_min_tokens = 0
    x = torch.randn(500, 22, 256, requires_grad=True)
    assert not blk.trains_on_hip(x) and not blk.hip_applies(x) and not blk.uses_hip(x), "CPU tensors: torch ops"
    rep = _replicas(blk, 2)[1]
    assert not rep.trains_on_hip(x) and [t.shape for t in rep._weights()] == [t.shape for t in blk._weights()]
    # the helper of the HIP path draws what DropPath draws on the torch path: same calls, same order, same generator state
    torch.manual_seed(9)
    s1, s2 = blk.draw_drop_path(x)
    after = torch.rand(3)
    torch.manual_seed(9)
    dp = DropPath(0.25).train()
    ones = torch.ones(500, 1, 1)
    m1, m2 = dp(ones), dp(ones)
    assert torch.equal(after, torch.rand(3))
    assert s1.shape == (500, 1, 1) and torch.equal(s1, m1) and torch.equal(s2, m2) and not torch.equal(s1, s2)
    assert set(s1.unique().tolist()) == {0.0, torch.tensor(1.0).div(0.75).item()}
    assert blk.eval().draw_drop_path(x) == (None, None)
    assert Block(64, 2, drop_path=0.0).train().draw_drop_path(x) == (None, None)
    plain = Block(64, 2, drop_path=0.0).train()
    torch.manual_seed(9)
    before = torch.rand(3)
    torch.manual_seed(9)
    plain.draw_drop_path(x)
    assert torch.equal(before, torch.rand(3)), "nothing is drawn where the torch path draws nothing"
    head = ST(5, num_frame=12, num_joints=7, in_chans=16, embed_dim_ratio=32, depth=2, num_heads=4, drop_path_rate=0.1).train()
    set_hip_min_tokens(head, 0)
    head(torch.randn(3, 16, 12, 7)).sum().backward()           # head_dim 8: not covered anywhere, trains through torch ops
