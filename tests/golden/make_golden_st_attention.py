#!/usr/bin/env python3
"""Fixtures of ST-TR's spatial attention unit FROM THE IMPORTED REFERENCE (model/ST_TR/gcn_attention.py).

Runs only where the reference tree is available; the reference's modules are imported as they lie and run on the CPU, and
only data is written (tests/golden/st_attention_reference.npz).  Nothing of the reference's source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_st_attention.py

Harness-side shims (the reference tree is untouched): ``self.incidence.cuda(x.get_device())`` (gcn_attention.py:109) is
made the identity for the duration of a call, and ``torch.bernoulli`` is wrapped to record the drop-connect mask.

Per case (N = 2, T <= 12): state_dict values come from tests/st_attention_ref.make_state (seeded), the input from
make_input.  Recorded: the key / shape layout; the eval output; the train output with its mask; the updated running
statistics; the gradients of every parameter and of x for a seeded dy.  Tensors above SMALL elements are stored as a
seeded sample of their entries (index + values) to keep the file small; the rest in full.  Also recorded: the reference's
seeded initial weights (torch.manual_seed(s) before construction), sampled the same way.
"""
import contextlib
import os
import sys

import numpy as np
import torch

REF = os.environ.get("STGCN_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from model.ST_TR.gcn_attention import gcn_unit_attention    # noqa: E402  (reference)
import st_attention_ref as R                                # noqa: E402  (tests/st_attention_ref.py)

SMALL = 4096
SAMPLE = 2048
N = 2
CASES = {   # name: (V, Cin, Cout, T)
    "v22_256_256": (22, 256, 256, 6),
    "v46_131_256": (46, 131, 256, 4),
    "v46_256_512": (46, 256, 512, 2),
    "v22_512_512": (22, 512, 512, 2),
}
INIT_SEED = 1234


@contextlib.contextmanager
def shims(masks):
    orig_cuda, orig_bern = torch.Tensor.cuda, torch.bernoulli
    torch.Tensor.cuda = lambda self, *a, **k: self

    def bern(p, *a, **k):
        m = orig_bern(p, *a, **k)
        masks.append(m.clone())
        return m
    torch.bernoulli = bern
    try:
        yield
    finally:
        torch.Tensor.cuda, torch.bernoulli = orig_cuda, orig_bern


def put(out, key, t, rng):
    a = t.detach().double().numpy().reshape(-1) if isinstance(t, torch.Tensor) else np.asarray(t).reshape(-1)
    if a.size <= SMALL:
        out[key] = a.astype(np.float32 if a.dtype != np.int64 else np.int64)
    else:
        idx = np.sort(rng.choice(a.size, SAMPLE, replace=False)).astype(np.int64)
        out[key + "@idx"] = idx
        out[key + "@val"] = a[idx].astype(np.float32)


def incidence(V):
    g = torch.Generator().manual_seed(V)
    return (torch.rand(3, V, V, generator=g) > 0.8).float()


def main():
    out = {}
    rng = np.random.default_rng(5)
    for name, (V, cin, cout, T) in CASES.items():
        seed = sum(map(ord, name))
        m = gcn_unit_attention(cin, cout, incidence(V), **R.unit_kwargs(V))
        keys = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        assert keys == R.layout(cin, cout, V), (keys, R.layout(cin, cout, V))
        out[f"{name}/layout"] = np.array([f"{k}:{'x'.join(map(str, s))}" for k, s in keys])
        sd = R.make_state(cin, cout, V, seed)
        m.load_state_dict(sd, strict=True)
        x = R.make_input(N, cin, T, V, seed + 1)
        masks = []
        with shims(masks):
            m.eval()
            with torch.no_grad():
                put(out, f"{name}/y_eval", m(x), rng)
            m.train()
            torch.manual_seed(seed + 2)
            xg = x.clone().requires_grad_(True)
            y = m(xg)
            dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 3))
            y.backward(dy)
        assert len(masks) == 1 and masks[0].numel() == N * T * R.NH * V
        out[f"{name}/mask"] = masks[0].numpy().astype(np.uint8)
        put(out, f"{name}/y_train", y, rng)
        for k, v in m.state_dict().items():
            if "running" in k or "num_batches" in k:
                put(out, f"{name}/after/{k}", v, rng)
        for k, p in m.named_parameters():
            put(out, f"{name}/grad/{k}", p.grad, rng)
        put(out, f"{name}/grad/x", xg.grad, rng)
        # seeded construction: the reference's initial weights
        torch.manual_seed(INIT_SEED)
        m0 = gcn_unit_attention(cin, cout, incidence(V), **R.unit_kwargs(V))
        for k, v in m0.state_dict().items():
            put(out, f"{name}/init/{k}", v.float() if v.is_floating_point() else v, rng)
    np.savez_compressed(os.path.join(HERE, "st_attention_reference.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
