#!/usr/bin/env python3
"""Fixture of the ST-ViT head FROM THE IMPORTED REFERENCE: stvit_reference.npz.

Build container only (needs the reference tree and ``einops``; see make_golden.py for the rules: the reference is imported as
it lies, run on CPU, only DATA is written - nothing of its source).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stvit.py

What it stores (the 17 M parameters are not stored and need not be):

* layout and seeded init of the reference ``ViT`` built from stvit_ref.CONFIG after ``torch.manual_seed(MODEL_SEED)``: every
  state_dict key in order, shape, and per key the fp64 sum and 16 seeded samples of the values;
* for that module prepared by stvit_ref.prepare and the input of stvit_ref.make_input: the logits with ``pool='cls'`` and
  ``pool='mean'`` and 4096 seeded samples of the embedding output (what enters the first layer), in fp32, and the same from
  the same module converted to fp64 on the same input - the reference's own floor.
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
import stvit_ref as sr                         # noqa: E402

N_SAMPLES, EMBED_SAMPLES = 16, 4096


def _load():
    """model/ST_Vit/trans.py of the reference as a module (the package path is shared with the drop-in shims)."""
    import make_golden as mg
    spec = importlib.util.spec_from_file_location("ref_stvit_trans", os.path.join(mg.REF, "model", "ST_Vit", "trans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(model, z):
    """(logits 'cls', logits 'mean', embedding output) of one module on one input."""
    seen = []
    hook = model.dropout.register_forward_hook(lambda mod, args, out: seen.append(args[0].detach().clone()))
    out = {}
    with torch.no_grad():
        for pool in ("cls", "mean"):
            model.pool = pool
            out[pool] = model(z)
    hook.remove()
    return out["cls"], out["mean"], seen[0]


def main():
    ref = _load()
    torch.manual_seed(sr.MODEL_SEED)
    model = ref.ViT(**sr.CONFIG).eval()
    sd = model.state_dict()
    g = {"keys": np.array(list(sd), dtype=np.str_),
         "ndim": np.array([v.dim() for v in sd.values()], dtype=np.int64),
         "shapes": np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64),
         "sums": np.array([v.double().sum().item() for v in sd.values()], dtype=np.float64)}
    idx, val = [], []
    for i, v in enumerate(sd.values()):
        ix = ar.sample_idx(v.numel(), N_SAMPLES, sr.MODEL_SEED + i)
        idx.append(np.resize(ix.numpy(), N_SAMPLES))
        val.append(np.resize(v.reshape(-1)[ix.long()].numpy(), N_SAMPLES))
    g["sample_idx"], g["sample_val"] = np.stack(idx), np.stack(val)

    sr.prepare(model)
    z = sr.make_input()
    cls32, mean32, emb32 = run(model, z)
    cls64, mean64, emb64 = run(model.double(), z.double())
    eix = ar.sample_idx(emb32.numel(), EMBED_SAMPLES, sr.INPUT_SEED + 1)
    g.update(z_samples=z.reshape(-1)[ar.sample_idx(z.numel(), N_SAMPLES, sr.INPUT_SEED + 2).long()].numpy(),
             logits_cls=cls32.numpy(), logits_mean=mean32.numpy(), logits_cls_f64=cls64.numpy(), logits_mean_f64=mean64.numpy(),
             embed_idx=eix.numpy(), embed_val=emb32.reshape(-1)[eix.long()].numpy(), embed_val_f64=emb64.reshape(-1)[eix.long()].numpy(),
             embed_max=np.float64(emb64.abs().max().item()), embed_shape=np.array(emb32.shape, dtype=np.int64))
    for pool, a, b in (("cls", cls32, cls64), ("mean", mean32, mean64)):
        g["floor_" + pool] = np.float64(((a.double() - b).abs().max() / b.abs().max()).item())
    g["floor_embed"] = np.float64(((emb32.double() - emb64).abs().max() / emb64.abs().max()).item())
    path = os.path.join(HERE, "stvit_reference.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes;", {k: float(g[k]) for k in ("floor_cls", "floor_mean", "floor_embed")})
    print("logits cls", cls32[0, :4].tolist(), "max", cls64.abs().max().item())


if __name__ == "__main__":
    main()
