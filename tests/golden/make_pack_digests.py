#!/usr/bin/env python3
"""SHA-256 of the packed blobs: what tests/test_pack_digests.py holds stgcn_tcn_pack and stgcn_stem_prepare to.

    python tests/golden/make_pack_digests.py [--out FILE]   # needs the GPU; loads STGCN_LIB, else the in-tree libstgcn_hip.so

The blobs are written by pack kernels and read by every convolution and fused-stem kernel at fixed offsets, so their bytes
are the contract between the two.  Weights and scales come from numpy.random.default_rng(seed); the destination is a zeroed
buffer of the queried size (alignment padding is then defined) and the C ABI is called directly.  Writes pack_digests.json:
one entry per case with the blob's size and digest.  The digests on file were written by the library as it was before the
plan of csrc/tcn.hip existed, twice, with equal results.
"""
import hashlib
import json
import os
import sys
from ctypes import c_int, c_uint, c_void_p

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))

from stgcn_amd import _capi  # noqa: E402

OUT = os.path.join(HERE, "pack_digests.json")
MATH = {"f32": _capi.MATH_F32, "bf16x3": _capi.MATH_BF16X3, "bf16": _capi.MATH_BF16, "f32_valu": _capi.MATH_F32_VALU,
        "f16mx": _capi.MATH_F16MX}
# stgcn_tcn_pack: (Cin, Cout, K, math)
TCN_CASES = [(3, 64, 9, "f32_valu"), (3, 64, 9, "bf16x3"), (16, 128, 3, "f32"), (128, 128, 9, "f32"), (16, 128, 9, "bf16x3"),
             (32, 128, 9, "bf16x3"), (64, 64, 9, "bf16x3"), (64, 64, 9, "bf16"), (32, 64, 3, "bf16x3")]
# stgcn_stem_prepare: (C, math) at Cin = 3, 3 subsets, K = 9
STEM_CASES = [(128, "f32"), (128, "bf16x3"), (128, "bf16"), (128, "f16mx"), (256, "bf16x3")]


def _digest(blob):
    torch.cuda.synchronize()
    return hashlib.sha256(blob.cpu().numpy().tobytes()).hexdigest()


def _dev(rng, *shape, lo=None):
    a = rng.standard_normal(shape) if lo is None else rng.uniform(lo, lo + 1.0, shape)
    return torch.from_numpy(a.astype(np.float32)).cuda()


def tcn_pack_digest(lib, seed, Cin, Cout, K, math):
    """(bytes, sha256) of stgcn_tcn_pack's blob for weights drawn from `seed`."""
    rng = np.random.default_rng(seed)
    W, scale = _dev(rng, Cout, Cin, K), _dev(rng, Cout, lo=0.5)
    nbytes = lib.stgcn_tcn_packed_bytes(Cin, Cout, K, MATH[math])
    blob = torch.zeros(nbytes, device="cuda", dtype=torch.uint8)
    _capi.call("stgcn_tcn_pack", c_void_p(W.data_ptr()), c_void_p(scale.data_ptr()), c_void_p(blob.data_ptr()), c_int(Cin),
               c_int(Cout), c_int(K), c_uint(MATH[math]), c_void_p(0))
    return nbytes, _digest(blob)


def stem_prepare_digest(lib, seed, C, math, Cin=3, S=3, K=9):
    """(bytes, sha256) of stgcn_stem_prepare's blob for parameters drawn from `seed`."""
    rng = np.random.default_rng(seed)
    Wd, bd, Wdown, bdown = _dev(rng, S, C, Cin), _dev(rng, S, C), _dev(rng, C, Cin), _dev(rng, C)
    bn_scale, bn_shift, down_scale, down_shift = _dev(rng, C, lo=0.5), _dev(rng, C), _dev(rng, C, lo=0.5), _dev(rng, C)
    Wt, t_scale = _dev(rng, C, C, K), _dev(rng, C, lo=0.5)
    nbytes = lib.stgcn_stem_prep_bytes(Cin, C, K, S, MATH[math])
    blob = torch.zeros(nbytes, device="cuda", dtype=torch.uint8)
    ptrs = [c_void_p(t.data_ptr()) for t in (Wd, bd, Wdown, bdown, bn_scale, bn_shift, down_scale, down_shift, Wt, t_scale, blob)]
    _capi.call("stgcn_stem_prepare", *ptrs, c_int(Cin), c_int(C), c_int(K), c_int(S), c_uint(MATH[math]), c_void_p(0))
    return nbytes, _digest(blob)


def all_digests(lib):
    """{case name: [bytes, sha256]}; the seed of a case is its position in the two lists."""
    out = {}
    for seed, (Cin, Cout, K, math) in enumerate(TCN_CASES):
        out[f"tcn_pack/{Cin}x{Cout}_k{K}_{math}"] = list(tcn_pack_digest(lib, seed, Cin, Cout, K, math))
    for seed, (C, math) in enumerate(STEM_CASES, start=100):
        out[f"stem_prepare/c{C}_{math}"] = list(stem_prepare_digest(lib, seed, C, math))
    return out


def main():
    lib = _capi.lib()
    first, second = all_digests(lib), all_digests(lib)
    keep = {k: v for k, v in first.items() if second[k] == v}
    for k, v in first.items():
        print(f"{k:36s} {v[0]:9d} B  {v[1][:16]}  {'' if k in keep else 'NOT REPRODUCIBLE: ' + second[k][1][:16]}")
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    with open(out, "w") as fh:
        json.dump(keep, fh, indent=1)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
