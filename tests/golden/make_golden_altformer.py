#!/usr/bin/env python3
"""Fixture of the AltFormer transformer heads FROM THE IMPORTED REFERENCE: altformer_reference.npz.

Build container only (needs the reference tree; see make_golden.py for the rules: the reference is imported as it lies,
run on CPU, only DATA is written - nothing of its source).  ``timm`` is replaced by make_golden_model.install_timm_stub.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_altformer.py

What it stores (the 16 M parameters of a head are not stored and need not be):

* layout and seeded init - for modelA (ST) and modelB (TS) of the reference ``ST_GCN_AltFormer`` built after
  ``torch.manual_seed(MODEL_SEED)`` (make_golden_model.build_reference_model), and for one ``Block`` built on its own from a
  seed: every state_dict key in order, shape, dtype, and per key the fp64 sum and 16 seeded samples of the values;
* block cases (tests/altformer_ref.py:BLOCK_CASES, one per stage of the heads): the reference ``Block`` built from the case's
  seed and prepared by altformer_ref.prepare_block, the input of altformer_ref.make_input (samples of it are stored so that a
  test can tell a different random stream from a wrong result), the output, and the intermediates LN1(x), the attention
  output before ``proj`` and the value after the first residual - whole where small, as seeded samples plus max |.| and the
  fp64 sum where dense would be too large;
* the reference's own floor: per case and stored tensor, its fp32 result against the same reference module run in fp64
  (``floor_y``, ``floor_ln1``, ``floor_att``, ``floor_x1``: the peaked soft-max makes the attention output the noisiest, about
  2e-6 of its max), and its fp32 output against tests/altformer_ref.block64 (``floor_fp32_vs_fp64``).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import altformer_ref as ar                     # noqa: E402
import make_golden_model as mm                 # noqa: E402

N_SAMPLES = 16
BLOCK_SEED = 9001


def _load(name):
    """model/AltFormer/<name>.py of the reference as a module (the package path is shared with the drop-in shims)."""
    import make_golden as mg
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(mg.REF, "model", "AltFormer", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def layout(prefix, module, seed):
    sd = module.state_dict()
    out = {prefix + "keys": np.array(list(sd), dtype=np.str_),
           prefix + "dtypes": np.array([str(v.dtype) for v in sd.values()], dtype=np.str_),
           prefix + "ndim": np.array([v.dim() for v in sd.values()], dtype=np.int64),
           prefix + "shapes": np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64),
           prefix + "sums": np.array([v.double().sum().item() for v in sd.values()], dtype=np.float64),
           prefix + "sample_seed": np.int64(seed)}
    idx, val = [], []
    for i, v in enumerate(sd.values()):
        ix = ar.sample_idx(v.numel(), N_SAMPLES, seed + i).long()
        ix = torch.cat([ix, ix.new_zeros(N_SAMPLES - ix.numel())])
        idx.append(ix.numpy())
        val.append(v.reshape(-1)[ix].double().numpy())
    out[prefix + "sample_idx"], out[prefix + "sample_val"] = np.stack(idx), np.stack(val)
    return out


def stored(out, key, t, seed, count):
    t = t.detach()
    n = t.numel()
    if key.endswith(".y") and n <= ar.DENSE_LIMIT:
        out[key] = t.numpy()
        return
    idx = ar.sample_idx(n, count, seed)
    out[key + "_idx"], out[key + "_val"] = idx.numpy(), t.reshape(-1)[idx.long()].numpy()
    out[key + "_absmax"] = np.float64(t.abs().max().item())
    out[key + "_sum"] = np.float64(t.double().sum().item())


def main():
    mm.install_timm_stub()
    out = {}
    model, _ = mm.build_reference_model("ST")
    out.update(layout("ST.", model.modelA, 100))
    out.update(layout("TS.", model.modelB, 200))
    ref_st = _load("model_ST")
    torch.manual_seed(BLOCK_SEED)
    blk = ref_st.Block(dim=256, num_heads=8, mlp_ratio=2., qkv_bias=True, qk_scale=None, norm_layer=ar.norm_layer())
    out.update(layout("Block.", blk, 300))
    out["block_seed"], out["model_seed"] = np.int64(BLOCK_SEED), np.int64(mm.MODEL_SEED)
    for name, (B, L, D, qkv_bias, qk_scale, seed) in ar.BLOCK_CASES.items():
        blk = ar.build_block(ref_st.Block, name)
        x = ar.make_input(name)
        grabbed = {}
        hooks = [blk.norm1.register_forward_hook(lambda m, i, o: grabbed.__setitem__("ln1", o.detach().clone())),
                 blk.attn.proj.register_forward_pre_hook(lambda m, i: grabbed.__setitem__("att", i[0].detach().clone())),
                 blk.norm2.register_forward_pre_hook(lambda m, i: grabbed.__setitem__("x1", i[0].detach().clone()))]
        with torch.no_grad():
            y = blk(x)
        got32 = dict(grabbed, y=y)
        with torch.no_grad():
            got64 = dict(y=blk.double()(x.double()), **grabbed)        # the reference itself in fp64 (hooks still on)
        blk.float()
        grabbed = {k: got32[k] for k in ("ln1", "att", "x1")}
        for h in hooks:
            h.remove()
        for k in ("y", "ln1", "att", "x1"):                            # the reference's own fp32 error, per stored tensor
            out[f"case.{name}.floor_{k}"] = np.float64(((got32[k].double() - got64[k]).abs().max() / got64[k].abs().max()).item())
        y64, mid64 = ar.block64(x, blk.state_dict(), scale=blk.attn.scale)
        floor = ((y.double() - y64).abs().max() / y64.abs().max()).item()
        pre = f"case.{name}."
        out[pre + "meta"] = np.array([B, L, D, int(qkv_bias), seed], dtype=np.int64)
        out[pre + "qk_scale"] = np.float64(qk_scale or 0.0)
        out[pre + "factor"] = np.float64(ar.QK_FACTOR)
        out[pre + "floor_fp32_vs_fp64"] = np.float64(floor)
        stored(out, pre + "x", x, seed + 11, 1024)
        stored(out, pre + "y", y, seed + 12, 8000)
        for k in ("ln1", "att", "x1"):
            stored(out, pre + k, grabbed[k], seed + 13 + len(k), 3000)
        q, kk, _ = (grabbed["ln1"] @ blk.attn.qkv.weight.T + (blk.attn.qkv.bias if qkv_bias else 0)).reshape(
            B, L, 3, 8, D // 8).permute(2, 0, 3, 1, 4).unbind(0)
        s = (q @ kk.transpose(-2, -1)) * blk.attn.scale
        out[pre + "score_absmax"] = np.float64(s.abs().max().item())
        out[pre + "mean_top_prob"] = np.float64(s.softmax(-1).max(-1).values.mean().item())
        print(name, "floor", f"{floor:.2e}", "max|score|", f"{s.abs().max().item():.1f}", "mean top prob",
              f"{out[pre + 'mean_top_prob']:.2f}", "max|y|", f"{y.abs().max().item():.2f}", "mean|y|", f"{y.abs().mean().item():.2f}")
    path = os.path.join(HERE, "altformer_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
