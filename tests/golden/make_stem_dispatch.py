#!/usr/bin/env python3
"""Fused-stem dispatch fixture: what tests/test_stem_dispatch.py holds the library's stem queries to.

    python tests/golden/make_stem_dispatch.py          # loads STGCN_LIB, else the in-tree libstgcn_hip.so

No GPU needed: the stem's size and support queries are host functions.  Writes stem_dispatch.json with, for each row of a
shape grid (flags, Cin, C, T, V, K, S):
  * supported      stgcn_stem_supported
  * kernel         stgcn_stem_kernel_name ("" where no fused kernel covers the shape)
  * features       stgcn_stem_features_used
  * prep_bytes     stgcn_stem_prep_bytes
  * ws_bytes       stgcn_stem_ws_bytes at N = WS_N[0] and WS_N[1]
The grid covers every math mode with and without STGCN_IN_NTVC, bf16x3 with each output option, Cin 3 / 4, 2 / 3 subsets,
C 64 - 384, K 3 / 9, T 1 - 500, V 7 - 65 and every (T, V) of the stem tests in test_gpu_parity.py.
"""
import json
import os
import sys
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))

from stgcn_amd import _capi  # noqa: E402

OUT = os.path.join(HERE, "stem_dispatch.json")
WS_N = (1, 300)

F = _capi
FLAG_SETS = {
    "f32": F.MATH_F32, "f32_valu": F.MATH_F32_VALU, "bf16x3": F.MATH_BF16X3, "bf16": F.MATH_BF16, "f16mx": F.MATH_F16MX,
}
FLAG_SETS.update({k + "+in_ntvc": v | F.IN_NTVC for k, v in list(FLAG_SETS.items())})
FLAG_SETS.update({"bf16x3+out_bf16": F.MATH_BF16X3 | F.OUT_BF16, "bf16x3+out_ntvc": F.MATH_BF16X3 | F.OUT_NTVC})

# (T, V) of the stem tests in test_gpu_parity.py
TEST_TV = [(180, 22), (200, 46), (500, 22), (37, 22), (9, 46), (5, 22), (64, 25), (1, 22), (23, 7), (30, 64), (300, 7),
           (90, 25), (60, 46), (50, 30), (60, 22), (33, 25), (40, 46), (2, 52), (20, 46), (40, 22), (13, 34), (30, 48),
           (25, 40), (12, 46), (20, 35), (4, 46), (30, 50), (12, 62), (64, 24), (90, 16), (3, 46), (9, 7), (20, 22)]


def grid():
    tv = set(TEST_TV)
    tv |= {(T, V) for V in range(7, 66) for T in (1, 40)}
    tv |= {(T, V) for V in (22, 25, 26, 33, 46, 52) for T in (2, 5, 13, 64, 180, 300, 500)}
    rows = [(f, 3, 128, T, V, 9, 3) for f in FLAG_SETS for (T, V) in sorted(tv)]
    tv_small = [(1, 22), (9, 7), (40, 22), (64, 25), (40, 26), (40, 32), (40, 33), (40, 46), (200, 46), (2, 52), (30, 64),
                (180, 22), (500, 22)]
    rows += [(f, 3, C, T, V, 9, 3) for f in FLAG_SETS for C in (64, 192, 256, 384) for (T, V) in tv_small]
    tv_tiny = [(1, 22), (9, 7), (40, 22), (40, 25), (40, 46), (2, 52), (180, 22), (200, 46)]
    rows += [(f, cin, C, T, V, K, S) for f in FLAG_SETS for (cin, K, S) in ((4, 9, 3), (3, 9, 2), (3, 3, 3))
             for C in (128, 256) for (T, V) in tv_tiny]
    return rows


COLUMNS = ["flags", "Cin", "C", "T", "V", "K", "S", "supported", "kernel", "features", "prep_bytes", "ws_bytes_n0",
           "ws_bytes_n1"]


def query(lib, f, cin, C, T, V, K, S):
    """One fixture row (COLUMNS) for the shape."""
    fl = FLAG_SETS[f]
    return [f, cin, C, T, V, K, S,
            lib.stgcn_stem_supported(cin, C, T, V, K, S, fl),
            lib.stgcn_stem_kernel_name(cin, C, T, V, K, S, fl).decode(),
            lib.stgcn_stem_features_used(cin, C, T, V, K, S, fl),
            lib.stgcn_stem_prep_bytes(cin, C, K, S, fl)] + [lib.stgcn_stem_ws_bytes(n, cin, C, T, V, K, S, fl) for n in WS_N]


def main():
    lib = _capi.lib()
    rows = [query(lib, *r) for r in grid()]
    names = Counter(r[8] or "unsupported" for r in rows)
    for name, n in sorted(names.items()):
        print(f"{name:24s} {n}")
    print(f"{len(rows)} rows")
    want = {"stem_mfma_f32_kernel", "stem_mfma_bf16_kernel", "stem_bf16_v4_kernel", "stem_bf16_v6_kernel",
            "stem_f16mx_kernel", "unsupported"}
    assert want <= set(names), f"grid misses {sorted(want - set(names))}"
    with open(OUT, "w") as fh:      # one row per line: a change of dispatch shows as a readable diff
        head = json.dumps({"flag_sets": FLAG_SETS, "ws_n": list(WS_N), "columns": COLUMNS})
        fh.write(head[:-1] + ', "rows": [\n')
        fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        fh.write("\n]}\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
