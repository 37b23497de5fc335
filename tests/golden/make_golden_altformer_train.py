#!/usr/bin/env python3
"""Gradient fixture of the AltFormer block FROM THE IMPORTED REFERENCE: altformer_train_reference.npz.

Build container only (needs the reference tree; the rules of make_golden.py apply: the reference is imported as it lies, run
on CPU, only DATA is written).  ``timm`` is replaced by make_golden_model.install_timm_stub.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_altformer_train.py

For the six block cases of tests/altformer_ref.py (same block and input recipes as altformer_reference.npz) and the seeded
upstream gradient altformer_train_ref.make_dy: the reference Block's gradient of ``x`` and of every parameter - whole up to
altformer_ref.DENSE_LIMIT elements, else seeded samples plus max |.| and the fp64 sum - and per tensor the reference's own
floor ``floor_d<key>``: its fp32 gradient against the same module differentiated in fp64, relative to max |fp64 gradient|.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import altformer_ref as ar                     # noqa: E402
import altformer_train_ref as tr               # noqa: E402
import make_golden_altformer as ma             # noqa: E402
import make_golden_model as mm                 # noqa: E402


def stored(out, key, t, seed):
    t = t.detach()
    n = t.numel()
    out[key + "_absmax"] = np.float64(t.abs().max().item())
    out[key + "_sum"] = np.float64(t.double().sum().item())
    if n <= ar.DENSE_LIMIT:
        out[key] = t.numpy()
        return
    idx = ar.sample_idx(n, tr.N_SAMPLES, seed)
    out[key + "_idx"], out[key + "_val"] = idx.numpy(), t.reshape(-1)[idx.long()].numpy()


def main():
    mm.install_timm_stub()
    ref_st = ma._load("model_ST")
    out = {}
    for name, (B, L, D, qkv_bias, qk_scale, seed) in ar.BLOCK_CASES.items():
        blk = ar.build_block(ref_st.Block, name)
        x, dy = ar.make_input(name), tr.make_dy(name)
        _, g32 = tr.module_grads(blk, x, dy)
        g32 = {k: v.clone() for k, v in g32.items()}
        _, g64 = tr.module_grads(blk.double(), x.double(), dy.double())
        pre = f"case.{name}."
        out[pre + "meta"] = np.array([B, L, D, int(qkv_bias), seed], dtype=np.int64)
        stored(out, pre + "dy", dy, seed + 40)
        worst = 0.0
        for i, k in enumerate(sorted(g32)):
            floor = ((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()).item()
            out[pre + "floor_d" + k] = np.float64(floor)
            worst = max(worst, floor)
            stored(out, pre + "d" + k, g32[k], seed + 41 + i)
        print(name, "worst fp32-vs-fp64 floor over the gradients", f"{worst:.2e}")
    path = os.path.join(HERE, "altformer_train_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
