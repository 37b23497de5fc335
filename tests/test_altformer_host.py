"""AltFormer heads, host side (no GPU): layout and seeded init against the reference's fixture, the torch-op path of the drop-in
modules against the reference's block cases and whole-head logits, the fp64 restatement against the same cases, the C ABI
declarations, DropPath semantics and the import shims."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import altformer_ref as ar
from _util import gather_flat, load_golden, parity_gate, sub_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "st-gcn-altformer_amd")
ABI_NAMES = ["stgcn_vit_linear_supported", "stgcn_vit_linear", "stgcn_vit_attention_supported", "stgcn_vit_attention",
             "stgcn_vit_block_supported", "stgcn_vit_block_ws_bytes", "stgcn_vit_block_forward"]


@pytest.fixture(scope="module")
def ref():
    return load_golden("altformer_reference")


def whole_model(style=None):
    """stgcn_amd.ST_GCN_AltFormer as make_golden_model.py builds the reference's: 14 classes, T = 180, V = 22, SHREC graph,
    constructed right after torch.manual_seed(MODEL_SEED)."""
    import stgcn_amd
    g = load_golden("model_altformer_shre")
    torch.manual_seed(int(g["model_seed"]))
    return stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style, graph="graph.SHRE",
                                      graph_args={"labeling_mode": "spatial"}), g


def check_layout(module, ref, prefix):
    sd = module.state_dict()
    assert list(sd) == [str(k) for k in ref[prefix + "keys"]], "state_dict keys / order"
    seed = int(ref[prefix + "sample_seed"])
    for i, (k, v) in enumerate(sd.items()):
        assert list(v.shape) == list(ref[prefix + "shapes"][i][:int(ref[prefix + "ndim"][i])]), k
        assert str(v.dtype) == str(ref[prefix + "dtypes"][i]), k
        assert v.double().sum().item() == float(ref[prefix + "sums"][i]), f"{k}: sum of the seeded initial values"
        ix = ar.sample_idx(v.numel(), 16, seed + i).long()
        assert np.array_equal(ix.numpy(), ref[prefix + "sample_idx"][i][:ix.numel()]), f"{k}: sample positions"
        assert np.array_equal(v.reshape(-1)[ix].double().numpy(), ref[prefix + "sample_val"][i][:ix.numel()]), \
            f"{k}: seeded initial values differ from the reference's"


def test_heads_layout_and_seeded_init_equal_reference(ref):
    model, _ = whole_model()
    check_layout(model.modelA, ref, "ST.")
    check_layout(model.modelB, ref, "TS.")
    assert [k.split(".")[0] for k in model.state_dict()][0] == "gcn0"
    assert {k.split(".")[0] for k in model.state_dict()} == {"gcn0", "tcn0", "modelA", "modelB"}


def test_block_layout_and_seeded_init_equal_reference(ref):
    from stgcn_amd.altformer import Block
    torch.manual_seed(int(ref["block_seed"]))
    blk = Block(dim=256, num_heads=8, mlp_ratio=2., qkv_bias=True, qk_scale=None, norm_layer=ar.norm_layer())
    check_layout(blk, ref, "Block.")


def case_tensors(ref, name):
    pre = f"case.{name}."
    x = ar.make_input(name)
    assert torch.equal(gather_flat(x, ref[pre + "x_idx"].astype(np.int64)), torch.from_numpy(ref[pre + "x_val"])), \
        "the seeded input differs from the one the fixture was made with (another torch random stream?)"
    return pre, x


def gate_samples(out, ref, key, rel, what, strict=True):
    """``out`` against the stored output ``key``: whole where the fixture holds it whole, else at its sampled positions."""
    if key in ref:
        return parity_gate(out, ref[key], rel, what, strict)
    got = gather_flat(out.detach().cpu(), ref[key + "_idx"].astype(np.int64))
    return parity_gate(got, ref[key + "_val"], rel, what, strict)


@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_block_torch_path_reproduces_reference_case(name, ref):
    from stgcn_amd.altformer import Block
    pre, x = case_tensors(ref, name)
    assert float(ref[pre + "score_absmax"]) > 20 and float(ref[pre + "mean_top_prob"]) > 0.5, "the case's soft-max is peaked"
    blk = ar.build_block(Block, name)
    grabbed = {}
    blk.norm1.register_forward_hook(lambda m, i, o: grabbed.__setitem__("ln1", o))
    blk.attn.proj.register_forward_pre_hook(lambda m, i: grabbed.__setitem__("att", i[0]))
    blk.norm2.register_forward_pre_hook(lambda m, i: grabbed.__setitem__("x1", i[0]))
    with torch.no_grad():
        y = blk(x)
    gate_samples(y, ref, pre + "y", 1e-5, f"{name} y")
    for k in ("ln1", "att", "x1"):
        gate_samples(grabbed[k], ref, pre + k, 1e-5, f"{name} {k}")


@pytest.mark.parametrize("name", sorted(ar.BLOCK_CASES))
def test_fp64_restatement_agrees_with_reference_case(name, ref):
    from stgcn_amd.altformer import Block
    pre, x = case_tensors(ref, name)
    blk = ar.build_block(Block, name)                 # (same seeded parameters as the reference's: see the init test)
    y, mid = ar.block64(x, blk.state_dict(), scale=blk.attn.scale)
    assert float(ref[pre + "floor_fp32_vs_fp64"]) < 5e-7 and float(ref[pre + "floor_y"]) < 5e-7
    # max-norm criterion only: the stored y is the reference's fp32 result, whose own error (floor_y, 1.2e-7 to 2.2e-7 of max|y|)
    # is above the 1e-7 * max|y| absolute term of parity_gate's second criterion at rel = 1e-6 - an exact result would fail it.
    gate_samples(y, ref, pre + "y", 1e-6, f"{name} y (fp64 restatement)", strict=False)
    # The stored intermediates are the reference's fp32 values; its own fp32 error there (the fixture's floor_*: the reference
    # module in fp32 against itself in fp64, up to 2.2e-6 of max|.| on the attention output, where the peaked soft-max
    # amplifies the rounding of the scores) is all that separates them from an exact restatement: bound = that floor.
    # (The floor is relative to the max over the whole tensor, so the stored max|.| is the scale, not the samples' max.)
    for k in ("ln1", "att", "x1"):
        got = gather_flat(mid[k], ref[pre + k + "_idx"].astype(np.int64))
        err = (got - torch.from_numpy(ref[pre + k + "_val"]).double()).abs().max().item()
        bound = max(1e-6, 1.01 * float(ref[pre + "floor_" + k])) * float(ref[pre + k + "_absmax"])
        assert err <= bound, f"{name} {k} (fp64 restatement): {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("style", ["ST", "TS"])
def test_heads_torch_path_reproduces_reference_logits(style):
    """The drop-in heads, built from the seed, on the oracle's stem output of the fixture's clips (CPU: the torch-op path)."""
    from oracle import stgcn_oracle as so
    model, g = whole_model(style)
    gp = so.agcn_params_from_state(sub_state(g, "gcn."), torch.from_numpy(g["A_fixed"]))
    tp = so.tcn_params_from_state(sub_state(g, "tcn."))
    x = torch.from_numpy(g["skeleton"]).permute(0, 3, 1, 2).contiguous()
    z = so.stem_forward(x, gp, tp).float()
    head = (model.modelA if style == "ST" else model.modelB).eval()
    with torch.no_grad():
        logits = head(z)
    parity_gate(logits, g[f"logits_{style}"], 1e-5, f"{style} logits")
    assert np.array_equal(logits.argmax(1).numpy(), g[f"argmax_{style}"])


def test_vit_abi_declared_and_exported():
    from stgcn_amd import _capi
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    handle = ctypes.CDLL(build())
    for n in ABI_NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
    assert re.search(r"#define\s+STGCN_ABI_VERSION\s+11\b", hdr)
    lib = _capi.lib()
    assert _capi.ABI_VERSION == 11 and lib.stgcn_version() == 11
    for L, D, hidden in ((22, 256, 512), (150, 512, 1024), (180, 512, 1024), (180, 256, 512), (46, 512, 1024), (256, 256, 512)):
        assert lib.stgcn_vit_block_supported(L, D, 8, hidden) == 1
        assert lib.stgcn_vit_block_ws_bytes(32, L, D, hidden) >= min(32, max(1, 32768 // L)) * L * (5 * D + hidden) * 4
    assert lib.stgcn_vit_block_supported(22, 384, 8, 768) == 0            # head_dim 48
    assert lib.stgcn_vit_block_supported(257, 256, 8, 512) == 0           # L > 256
    assert lib.stgcn_vit_block_supported(22, 256, 8, 500) == 0            # hidden not a multiple of 64
    assert lib.stgcn_vit_attention_supported(256, 8, 64) == 1 and lib.stgcn_vit_attention_supported(22, 8, 48) == 0
    assert lib.stgcn_vit_linear_supported(1, 256, 768, _capi.MATH_BF16X3) == 1
    assert lib.stgcn_vit_linear_supported(1, 250, 768, _capi.MATH_F32) == 0
    assert lib.stgcn_vit_linear_supported(1, 256, 768, _capi.MATH_BF16) == 0
    assert lib.stgcn_vit_block_ws_bytes(0, 22, 256, 512) == 0
    rc = lib.stgcn_vit_block_forward(*([None] * 13), 1e-6, 0.1, None, 0, None, 2, 22, 256, 8, 512, 0, None)
    assert rc == -1 and b"null" in lib.stgcn_last_error().lower()


def test_drop_path_semantics():
    from stgcn_amd.altformer import Block, DropPath
    dp = DropPath(0.25)
    x = torch.ones(4000, 3, 5)
    assert dp.eval()(x) is x and DropPath(0.0).train()(x) is x
    dp.train()
    torch.manual_seed(3)
    y = dp(x)
    after = torch.rand(1)
    torch.manual_seed(3)
    mask = torch.empty(4000, 1, 1).bernoulli_(0.75)                       # one draw of batch-size elements per call
    assert torch.equal(after, torch.rand(1)), "DropPath draws exactly one bernoulli of batch-size elements"
    assert torch.equal(y, x * (mask / 0.75))
    per_sample = y.reshape(4000, -1)
    assert ((per_sample == 0).all(1) | (per_sample == 1 / 0.75).all(1)).all(), "whole samples are kept or dropped"
    assert 0.70 < (per_sample[:, 0] != 0).float().mean().item() < 0.80
    assert isinstance(Block(64, 2, drop_path=0.0).drop_path, torch.nn.Identity)
    assert isinstance(Block(64, 2, drop_path=0.1).drop_path, DropPath)


def test_head_modules_run_their_torch_path_on_cpu_and_train():
    from stgcn_amd.altformer import ST
    torch.manual_seed(0)
    head = ST(5, num_frame=12, num_joints=7, in_chans=16, embed_dim_ratio=32, depth=2, num_heads=4, drop_path_rate=0.1).train()
    out = head(torch.randn(3, 16, 12, 7))
    assert out.shape == (3, 5)
    out.sum().backward()
    used = {"Spatial_cls_token", "cls_token", "Spatial_norm.weight", "Spatial_norm.bias", "Temporal_norm.weight",
            "Temporal_norm.bias", "weighted_mean.weight", "weighted_mean.bias", "fcn.weight", "fcn.bias"}
    for k, p in head.named_parameters():
        assert (p.grad is not None) != (k in used), k                     # the reference's forward leaves exactly these out


def test_shims_resolve_without_timm(tmp_path):
    code = textwrap.dedent(f'''
        import sys
        sys.path.insert(0, {PKG!r})
        from model.AltFormer.model_ST import ST
        from model.AltFormer.model_TS import TS
        import stgcn_amd.altformer as alt
        assert ST is alt.ST and TS is alt.TS, (ST, TS)
        assert "timm" not in sys.modules and "einops" not in sys.modules
        try:
            import timm
            raise SystemExit("timm is installed: the test cannot show that it is not needed")
        except ImportError:
            pass
        print("shims ok")
    ''')
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shims ok" in r.stdout, r.stdout + r.stderr
