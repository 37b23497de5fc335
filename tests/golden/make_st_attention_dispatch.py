#!/usr/bin/env python3
"""Dispatch fixture of ST-TR's attention unit: what tests/test_st_attention_dispatch.py holds the unit's six host queries to.

    STGCN_LIB=path/to/libstgcn_hip.so python tests/golden/make_st_attention_dispatch.py --commit <hash>

Run it on the library of the commit BEFORE the unit's plan (csrc/st_attention.hip ``plan_st_attention``) existed: the fixture
pins that moving every decision into the plan changed no answer.  No GPU needed.  Writes st_attention_dispatch.json:
  * "unit"     [Cin, Cout, dk, V, heads, stgcn_st_attention_supported, stgcn_st_attention_math_supported per MATHS]
  * "ws"       [N, Cin, Cout, dk, T, V, heads, stgcn_st_attention_ws_bytes of pass 0, 1, 2]
  * "product"  [M, K, TV, then per MATHS: stgcn_wx_product_supported, stgcn_wx_product_kernel_name as an index into
                "kernels", stgcn_wx_product_ws_bytes]
The grid: Cin 0 - 260; (Cout, dk, heads) inside and outside the three head classes (4,16), (8,32), (16,64); V 0 - 70; N and T
up to and past the 16-bit grid axes and the two arithmetics' column limits (TV = 65535*64 for f32, 65535*128 for bf16x3); M, K
and TV across both of those, across 2^31 elements a clip and across M*K = 2^29.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))

from stgcn_amd import _capi  # noqa: E402

OUT = os.path.join(HERE, "st_attention_dispatch.json")
MATHS = {"f32": 0, "bf16x3": 1, "bf16": 2, "f32_valu": 3, "unknown": 7, "bf16x3+frozen": 1 | _capi.BN_FROZEN}
KERNELS = ["", "gemm_f32_kernel", "wx_bf16x3_kernel<64x128>", "wx_bf16x3_kernel<128x128>"]
INSIDE = [(128, 32, 8), (256, 64, 8), (512, 128, 8), (64, 16, 4), (128, 32, 4), (16, 4, 1), (32, 8, 1), (64, 16, 1), (1024, 256, 16)]
OUTSIDE = [(64, 16, 8), (192, 48, 8), (128, 32, 3), (128, 16, 8), (128, 64, 8), (128, 32, 0), (96, 24, 8), (128, 0, 8), (0, 32, 8),
           (128, 32, -1), (1024, 256, 8), (16, 4, 2)]
F32_TV, BF16_TV = 65535 * 64, 65535 * 128


def unit_grid():
    rows = [(cin, 256, 64, 25, 8) for cin in range(0, 261)]
    rows += [(cin, co, dk, V, h) for (co, dk, h) in INSIDE + OUTSIDE for cin in (1, 3, 131) for V in (1, 22, 64, 65)]
    rows += [(cin, co, dk, V, 8) for V in range(0, 71) for (cin, co, dk) in ((3, 128, 32), (256, 512, 128))]
    rows += [(-1, 128, 32, 22, 8), (64, 128, 32, -1, 8)]
    return rows


def ws_grid():
    rows = [(N, 1, 16, 4, T, 64, 1) for N in (1, 2, 16, 17, 65535, 65536) for T in (1, 300, 65535, 65536, 131072, 131073)]
    rows += [(N, cin, co, dk, T, V, h) for N in (1, 15, 16, 300) for (cin, co, dk, h) in ((3, 128, 32, 8), (131, 256, 64, 8), (512, 512, 128, 8),
                                                                                       (260, 64, 16, 4), (64, 64, 16, 8), (16, 192, 48, 8))
             for (T, V) in ((1, 1), (180, 22), (20, 25), (9, 46), (3, 64), (3, 65), (3, 70))]
    rows += [(2, cin, 128, 32, 12, 22, 8) for cin in (1, 2, 63, 64, 65, 259, 260)]
    base = (4, 64, 128, 32, 20, 25, 8)
    rows += [base[:i] + (bad,) + base[i + 1:] for i in range(7) for bad in (0, -1)]
    return rows


def product_grid():
    mk = [(1, 1), (16, 1), (1, 16), (131, 768), (192, 64), (256, 64), (768, 512), (1024, 1), (1, 1024), (1023, 7), (511, 512), (512, 512),
          (513, 512), (16384, 16384), (23170, 23000), (32768, 16384), (100000, 3), (3, 100000), (0, 4), (4, 0), (-1, 4)]
    tvs = [-1, 0, 1, 3450, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 22) - 1, F32_TV - 1, F32_TV, F32_TV + 1, 1 << 22, BF16_TV - 1, BF16_TV,
           BF16_TV + 1, (1 << 31) - 1, 1 << 31, 1 << 40]
    return [(M, K, TV) for (M, K) in mk for TV in tvs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library is recorded")
    args = ap.parse_args()
    lib = _capi.lib()
    unit = [list(r) + [lib.stgcn_st_attention_supported(*r)] + [lib.stgcn_st_attention_math_supported(*r, m) for m in MATHS.values()]
            for r in unit_grid()]
    ws = [list(r) + [lib.stgcn_st_attention_ws_bytes(*r, p) for p in (0, 1, 2)] for r in ws_grid()]
    ws += [[4, 64, 128, 32, 20, 25, 8] + [lib.stgcn_st_attention_ws_bytes(4, 64, 128, 32, 20, 25, 8, p) for p in (-1, 3)] + [None]]
    product = []
    for (M, K, TV) in product_grid():
        row = [M, K, TV]
        for m in MATHS.values():
            row += [lib.stgcn_wx_product_supported(M, K, TV, m), KERNELS.index(lib.stgcn_wx_product_kernel_name(M, K, TV, m).decode()),
                    lib.stgcn_wx_product_ws_bytes(M, K, m)]
        product.append(row)
    assert {r[5] for r in unit} == {0, 1} and {r[6] for r in unit} == {0, 1} and {r[7] for r in unit} == {0, 1}
    for i, name in enumerate(MATHS):
        got = {r[3 + 3 * i] for r in product}
        assert got == ({0, 1} if name in ("f32", "bf16x3", "bf16x3+frozen") else {0}), (name, got)
    assert {r[4] for r in product} == {0, 1} and {r[7] for r in product} == {0, 2, 3}, "a kernel name is missing from the grid"
    with open(OUT, "w") as fh:      # one row per line: a changed answer shows as a readable diff
        fh.write(json.dumps({"commit": args.commit, "library": os.path.basename(_capi.LIB_PATH), "maths": MATHS, "kernels": KERNELS})[:-1])
        for name, rows in (("unit", unit), ("ws", ws), ("product", product)):
            fh.write(',\n"%s": [\n' % name)
            fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
            fh.write("\n]")
        fh.write("}\n")
    print("wrote", OUT, {"unit": len(unit), "ws": len(ws), "product": len(product)})


if __name__ == "__main__":
    main()
