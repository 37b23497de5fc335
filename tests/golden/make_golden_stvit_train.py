#!/usr/bin/env python3
"""Training fixture of the ST-ViT head FROM THE IMPORTED REFERENCE: stvit_train_reference.npz.

Build container only (needs the reference tree and ``einops``; the rules of make_golden.py apply: the reference is imported as
it lies, run on CPU, only DATA is written).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stvit_train.py

The reference's ``ViT`` at stvit_ref.CONFIG with ``depth = stvit_train_ref.FIXTURE_DEPTH``, built after
``torch.manual_seed(stvit_ref.MODEL_SEED)``, prepared by stvit_ref.prepare, converted to fp64, in ``.train()``, on the two
clips of stvit_ref.make_input.  Each of its six ``nn.Dropout``s inside the layers is replaced by a module that multiplies by
the seeded mask stvit_train_ref.fixture_masks gives for its layer and place, so the result does not depend on a generator:
it pins WHERE the three dropouts of a layer sit.  One backward from the seeded cotangent stvit_train_ref.fixture_dlogits.

Stored: the logits, and the gradient of the input and of every parameter - whole up to altformer_ref.DENSE_LIMIT elements,
else stvit_train_ref.N_SAMPLES seeded samples - each with its max |.| and fp64 sum, as make_golden_altformer_train.py does.
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
import stvit_ref as sr                         # noqa: E402
import stvit_train_ref as vr                   # noqa: E402
import make_golden_stvit as ms                 # noqa: E402


class Masked(torch.nn.Module):
    """Stands where an nn.Dropout stood: multiplies by a fixed tensor."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        assert x.shape == self.mask.shape, (x.shape, self.mask.shape)
        return x * self.mask


def stored(out, key, t, seed):
    t = t.detach()
    out[key + "_absmax"] = np.float64(t.abs().max().item())
    out[key + "_sum"] = np.float64(t.double().sum().item())
    if t.numel() <= ar.DENSE_LIMIT:
        out[key] = t.numpy()
        return
    idx = ar.sample_idx(t.numel(), vr.N_SAMPLES, seed)
    out[key + "_idx"], out[key + "_val"] = idx.numpy(), t.reshape(-1)[idx.long()].numpy()


def main():
    ref = ms._load()
    torch.manual_seed(sr.MODEL_SEED)
    model = ref.ViT(**dict(sr.CONFIG, depth=vr.FIXTURE_DEPTH), dropout=0.1, emb_dropout=0.0)
    sr.prepare(model)
    model = model.double().train()
    for i, (attn, ff) in enumerate(model.transformer.layers):
        m_proj, m_act, m_fc2 = (m.double() for m in vr.fixture_masks(i))
        assert all(type(d) is torch.nn.Dropout for d in (attn.fn.to_out[1], ff.fn.net[2], ff.fn.net[4]))
        attn.fn.to_out[1], ff.fn.net[2], ff.fn.net[4] = Masked(m_proj), Masked(m_act), Masked(m_fc2)
    assert not any(type(m) is torch.nn.Dropout and m.p > 0 for m in model.modules()), "a dropout the masks do not stand for"
    z = sr.make_input().double().requires_grad_(True)
    logits = model(z)
    logits.backward(vr.fixture_dlogits().double())
    out = {"logits": logits.detach().numpy(), "depth": np.int64(vr.FIXTURE_DEPTH)}
    stored(out, "dz", z.grad, sr.INPUT_SEED + 50)
    for i, (k, p) in enumerate(model.named_parameters()):
        stored(out, "d" + k, p.grad, sr.INPUT_SEED + 51 + i)
    path = os.path.join(HERE, "stvit_train_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; logits", logits[0, :4].tolist())


if __name__ == "__main__":
    main()
