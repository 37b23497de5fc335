#!/usr/bin/env python3
"""Kernel times of gcn_unit_attention's four W . X products, in both arithmetics, from a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o wx -- python tools/profile_wx_product.py run
    python tools/profile_wx_product.py parse DIR [OUT.json]

``run`` calls stgcn_wx_product for the products of the four LMDHG STR layers (N = 32, V = 46: qkv, out with the skip connection
where Cin == Cout, and the two input gradients), REPS times in bf16x3 and REPS times in f32 each, in a fixed order.  ``parse``
reads the trace's dispatches of wx_bf16x3_kernel / gemm_f32_kernel in that order and prints, per product and arithmetic, the
median kernel time and the TFLOP/s from the shapes (2 N M K TV).  The f32 path's copy of the skip connection is a memory copy,
not a kernel, and is not in these times."""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [(131, 256, 300), (256, 256, 150), (256, 512, 150), (512, 512, 75)]     # (Cin, Cout, T)
N, V, REPS = 32, 46, 3


def products():
    """(label, M, K, TV, w_transposed, with R) in call order."""
    out = []
    for cin, cout, T in LAYERS:
        cq, tv, tag = cout // 2 + cout, T * V, f"{cin}->{cout},T={T}"
        out += [(f"{tag} qkv", cq, cin, tv, False, False), (f"{tag} out", cout, cout, tv, False, cin == cout),
                (f"{tag} Wout^T.dz", cout, cout, tv, True, False), (f"{tag} Wqkv^T.dqkv", cin, cq, tv, True, False)]
    return out


def run():
    sys.path[:0] = [os.path.join(ROOT, "st-gcn-altformer_amd")]
    import torch
    from stgcn_amd import functional as F
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    for _, M, K, TV, wt, res in products():
        W = (torch.randn((K, M) if wt else (M, K), generator=g) / K ** 0.5).to(dev)
        X = torch.randn(N, K, TV, generator=g).to(dev)
        R = torch.randn(N, M, TV, generator=g).to(dev) if res else None
        bias = None if wt else torch.randn(M, generator=g).to(dev)
        for math in (F.MATH_BF16X3, F.MATH_F32):
            for _ in range(REPS):
                F.wx_product(W, X, bias, R, w_transposed=wt, math=math)
        torch.cuda.synchronize()
        del W, X, R


def parse(directory, out=None):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    rows = []
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            kind = "bf16x3" if "wx_bf16x3_kernel" in name else "f32" if "gemm_f32_kernel" in name else None
            if kind:
                rows.append((int(r["Start_Timestamp"]), kind, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    prods = products()
    assert len(rows) == len(prods) * 2 * REPS, (len(rows), len(prods))
    res, i = {}, 0
    for label, M, K, TV, _, _ in prods:
        entry = {"M": M, "K": K, "TV": TV, "gflop": round(2.0 * N * M * K * TV / 1e9, 2)}
        for kind in ("bf16x3", "f32"):
            chunk = rows[i:i + REPS]
            i += REPS
            assert all(k == kind for _, k, _ in chunk), (label, kind, chunk)
            us = statistics.median(d for _, _, d in chunk) / 1e3
            entry[kind] = {"us": round(us, 1), "tflops": round(2.0 * N * M * K * TV / (us * 1e-6) / 1e12, 1)}
        entry["speedup"] = round(entry["f32"]["us"] / entry["bf16x3"]["us"], 2)
        res[label] = entry
    text = json.dumps({"tool": "profile_wx_product", "N": N, "V": V, "reps": REPS, "products": res}, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "parse":
        parse(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        run()
