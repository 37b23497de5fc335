"""Records SHA-256 digests of what the heads' block entry points compute, case by case: tests/golden/vit_block_digests.json.
Run it on an MI355X against the library of the commit BEFORE a change that must not move a result bit (the library comes from
``STGCN_LIB``, as everywhere); tests/test_vit_block_digests_gpu.py imports ``cases()`` and ``run()`` and compares.

    STGCN_LIB=path/to/libstgcn_hip.so python tests/golden/make_vit_block_digests.py --commit <hash> [--out file.json]

The 1e-4 and 1e-2 gates of the suite cannot tell ``math`` from ``math_qkv`` handed to the wrong linear; the bits can.  The
sizes are the smallest that reach every branch of the block's plan and its slab walker: resident attention in one slab
(5 x 22), resident in slabs of 128 and 1 sequences (129 x 256), streaming in slabs of 109 and 1 (110 x 300), at D = 64 with two
heads of 32 and hidden = 128, and once with two heads of 64 (D = 128, hidden = 64).

A digest covers the result tensors only (y; dx and the twelve parameter gradients; dx, dW, db), never ``saved`` or a
workspace, whose padding is uninitialised.  Every case runs twice here and is written only if both runs agree.
"""
import argparse
import hashlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "st-gcn-altformer_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from stgcn_amd._capi import (MATH_BF16X3 as BF16X3, MATH_F32 as F32, VIT_BF16 as BF16, VIT_QKV_F32 as QKV_F32,  # noqa: E402
                             VIT_TILE_AUTO as TILE_AUTO, VIT_TRAIN_BF16 as TRAIN_BF16)

SMALL = (64, 2, 128)            # D, heads, hidden: head_dim 32
WIDE = (128, 2, 64)             # head_dim 64
SHAPES = ((5, 22), (129, 256), (110, 300))          # (B, L): see the module docstring
INFER_MATH = (F32, BF16X3, BF16X3 | QKV_F32)
TRAIN_MATH = (F32, BF16X3, BF16X3 | QKV_F32, TRAIN_BF16 | BF16X3 | QKV_F32, TRAIN_BF16 | BF16X3, TRAIN_BF16 | F32)
LINEAR_SHAPES = ((44, 64, 100), (300, 128, 64))     # M, K, Nout
LINEAR_MATH = (F32, BF16X3, TRAIN_BF16 | BF16X3)
UNSUPPORTED = "STGCN_ERR_UNSUPPORTED"               # the "digest" of the one case that must be refused
PARAMS = ("norm1.weight", "norm1.bias", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "norm2.weight", "norm2.bias",
          "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def cases():
    """Every case as a dict with a unique ``id``, in a fixed order."""
    out = []
    for B, L in SHAPES:
        for m in INFER_MATH:
            for tile in (0, TILE_AUTO):
                out.append(dict(kind="forward", dims=SMALL, B=B, L=L, flags=m | tile))
        for tile in (0, TILE_AUTO):         # the bf16 mode covers the resident lengths only: refused at 300
            out.append(dict(kind="forward", dims=SMALL, B=B, L=L, flags=BF16 | tile))
    out.append(dict(kind="forward", dims=WIDE, B=5, L=22, flags=BF16X3 | QKV_F32 | TILE_AUTO))
    for B, L in SHAPES:
        for m in TRAIN_MATH:                # stochastic-depth factors on the two-slab shapes, None on the one-slab one
            out.append(dict(kind="train", dims=SMALL, B=B, L=L, flags=m, factors=B > 5))
    out.append(dict(kind="train", dims=WIDE, B=5, L=22, flags=TRAIN_BF16 | BF16X3 | QKV_F32, factors=False))
    for M, K, Nout in LINEAR_SHAPES:
        for m in LINEAR_MATH:
            for form in ("plain", "h_pre", "accumulate"):
                out.append(dict(kind="linear_backward", M=M, K=K, Nout=Nout, flags=m, form=form))
    for c in out:
        if c["kind"] == "linear_backward":
            c["id"] = f"linear_backward-{c['M']}x{c['K']}x{c['Nout']}-{c['flags']:#x}-{c['form']}"
        else:
            c["id"] = f"{c['kind']}-B{c['B']}-L{c['L']}-D{c['dims'][0]}-{c['flags']:#x}" + ("-factors" if c.get("factors") else "")
    assert len({c["id"] for c in out}) == len(out)
    return out


_inputs = {}


def block_inputs(B, L, dims):
    """x, dy, the twelve parameters and the two factor vectors of a shape, drawn once on the CPU from a generator seeded by
    the shape and shared (unchanged) by every case of that shape."""
    key = (B, L) + tuple(dims)
    if key not in _inputs:
        D, heads, hidden = dims
        g = torch.Generator().manual_seed(1000 * L + B + D)

        def lin(o, i):
            return (torch.rand(o, i, generator=g) * 2 - 1) / math.sqrt(i), (torch.rand(o, generator=g) * 2 - 1) / math.sqrt(i)
        p = {}
        p["norm1.weight"], p["norm1.bias"] = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
        p["qkv.weight"], p["qkv.bias"] = lin(3 * D, D)
        p["qkv.weight"][:2 * D] *= 4.0      # peaked soft-max, as tests/altformer_ref.py
        p["proj.weight"], p["proj.bias"] = lin(D, D)
        p["norm2.weight"], p["norm2.bias"] = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
        p["fc1.weight"], p["fc1.bias"] = lin(hidden, D)
        p["fc2.weight"], p["fc2.bias"] = lin(D, hidden)
        x = torch.randn(B, L, D, generator=g)
        dy = torch.randn(B, L, D, generator=g)
        idx = torch.arange(B)
        s1 = torch.full((B,), 1 / 0.9)
        s2 = torch.full((B,), 1 / 0.9)
        s1[(idx % 5 == 1) | (idx == B - 1)] = 0.0     # a dropped sequence in every slab, the one-sequence last slab included,
        s2[(idx % 7 == 2) | (idx == B - 1)] = 0.0     # for both factors
        _inputs[key] = (x, dy, p, s1, s2)
    return _inputs[key]


def linear_inputs(M, K, Nout):
    key = ("linear", M, K, Nout)
    if key not in _inputs:
        g = torch.Generator().manual_seed(7 * M + K + Nout)
        _inputs[key] = tuple(torch.randn(*s, generator=g) for s in ((M, Nout), (M, K), (Nout, K), (M, K), (M, K)))
    return _inputs[key]


def run(case, dev):
    """The result tensors of one case, in a fixed order; UNSUPPORTED where the library refuses the case with that status."""
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    if case["kind"] == "linear_backward":
        dy, a, W, h_pre, dx0 = (t.to(dev) for t in linear_inputs(case["M"], case["K"], case["Nout"]))
        dx, dW, db = F.vit_linear_backward(dy, a, W, h_pre=h_pre if case["form"] == "h_pre" else None,
                                           dx_accumulate=dx0.clone() if case["form"] == "accumulate" else None, math=case["flags"])
        return [dx, dW, db]
    D, heads, hidden = case["dims"]
    x, dy, p, s1, s2 = block_inputs(case["B"], case["L"], case["dims"])
    x, dy = x.to(dev), dy.to(dev)
    params = [p[n].to(dev) for n in PARAMS]
    eps, scale = 1e-6, (D // heads) ** -0.5
    if case["kind"] == "forward":
        try:
            return [F.vit_block_forward(x, *[(params[i], params[i + 1]) for i in range(0, 12, 2)], heads, eps, scale, case["flags"])]
        except _capi.StgcnError as e:
            if e.code == -2:
                return UNSUPPORTED
            raise
    f1, f2 = (s1.to(dev), s2.to(dev)) if case["factors"] else (None, None)
    y, saved = F.vit_block_forward_train(x, params, heads, eps, scale, case["flags"], f1, f2)
    g = F.vit_block_backward(x, params, saved, dy, heads, eps, scale, case["flags"], f1, f2)
    return [y, g["x"]] + [g[n] for n in PARAMS]


def digest(result):
    if isinstance(result, str):
        return result
    h = hashlib.sha256()
    for t in result:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library is recorded")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "vit_block_digests.json"))
    args = ap.parse_args()
    from stgcn_amd import _capi
    dev = torch.device("cuda:0")
    digests = {}
    for c in cases():
        first, second = digest(run(c, dev)), digest(run(c, dev))
        if first != second:
            print(f"NOT WRITTEN {c['id']}: two runs of the same library disagree", flush=True)
            continue
        digests[c["id"]] = first
        print(c["id"], first[:16], flush=True)
    doc = {"commit": args.commit, "library": os.path.basename(_capi.LIB_PATH), "device": torch.cuda.get_device_name(0),
           "rocm": torch.version.hip, "torch": torch.__version__, "digests": digests}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(digests), "of", len(cases()), "cases")


if __name__ == "__main__":
    main()
