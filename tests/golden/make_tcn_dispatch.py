#!/usr/bin/env python3
"""Temporal-conv dispatch fixture: what tests/test_tcn_dispatch.py holds the library's temporal-conv queries to.

    python tests/golden/make_tcn_dispatch.py          # loads STGCN_LIB, else the in-tree libstgcn_hip.so

No GPU needed: the size and support queries are host functions.  Writes tcn_dispatch.json: one line per group
[flags, Cin, Cout, K, stride, packed_bytes, entries] with one entry per (T, V) of the section's "tv" list,
[supported, kernel, train_ws_n0, train_ws_n1, backward_ws_n0, backward_ws_n1]:
  * supported      stgcn_tcn_supported
  * kernel         stgcn_tcn_kernel_name as an index into "kernels" ("" where no kernel takes the shape)
  * packed_bytes   stgcn_tcn_packed_bytes (it depends on the group alone, which the generator checks)
  * train_ws       stgcn_tcn_train_ws_bytes at N = WS_N[0] and WS_N[1]
  * backward_ws    stgcn_tcn_backward_ws_bytes, likewise
"frozen_sizes": "equal" records that every workspace size was the same with STGCN_BN_FROZEN (the generator checks it; the
test queries both and holds both to the one figure).  The file was first written by the library as it was before the plan
of csrc/tcn.hip existed (which had no name query: kernel = null); `--add-kernel` reads the existing file, checks that
every other figure still holds and fills in the kernels.
"""
import json
import os
import sys
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))

from stgcn_amd import _capi  # noqa: E402

OUT = os.path.join(HERE, "tcn_dispatch.json")
WS_N = (2, 64)

F = _capi
FLAG_SETS = {"f32": F.MATH_F32, "bf16x3": F.MATH_BF16X3, "bf16": F.MATH_BF16, "f32_valu": F.MATH_F32_VALU,
             "f32_valu+along_v": F.MATH_F32_VALU | F.CONV_ALONG_V}
CHANNELS = [(3, 64), (16, 128), (32, 128), (64, 64), (64, 128), (128, 128), (128, 64), (48, 128), (30, 128), (64, 96),
            (256, 256)]
K_STRIDE = [(9, 1), (9, 2), (3, 1), (1, 2), (1, 1), (5, 1), (4, 1)]
TV = [(1, 22), (5, 22), (12, 22), (180, 22), (90, 25), (12, 46), (200, 46), (30, 64), (9, 7), (40, 32), (40, 33), (2, 52),
      (300, 7)]
MATRIX_CORE = {"tcn_mfma_f32_kernel", "tcn_mfma_bf16_kernel", "tcn_bf16_v4_kernel", "tcn_bf16_v6_kernel"}
KERNELS = MATRIX_CORE | {"", "tcn_valu_kernel", "tcn_valu_joint_axis_kernel"}


KERNEL_LIST = ["", "tcn_valu_kernel", "tcn_valu_joint_axis_kernel", "tcn_mfma_f32_kernel", "tcn_mfma_bf16_kernel",
               "tcn_bf16_v4_kernel", "tcn_bf16_v6_kernel"]
# sections: name -> (flag sets, (Cin, Cout), (K, stride), (T, V)); "joint_axis" is Unit2D(dim=3) in the math mode it goes with
SECTIONS = {"grid": (("f32", "bf16x3", "bf16", "f32_valu"), CHANNELS, K_STRIDE, TV),
            "joint_axis": (("f32_valu+along_v",), [(3, 64), (64, 128)], [(9, 1), (3, 2), (4, 1)], [(12, 22), (5, 1), (40, 33)])}


def query(lib, f, ci, co, K, s, tv):
    """One group (a line of the file); the kernel is None from a library without the name query."""
    fl = FLAG_SETS[f]
    name = getattr(lib, "stgcn_tcn_kernel_name", None)
    entries = []
    for (T, V) in tv:
        sizes = []
        for fn in (lib.stgcn_tcn_train_ws_bytes, lib.stgcn_tcn_backward_ws_bytes):
            for n in WS_N:
                sizes.append(fn(n, ci, co, T, V, K, s, fl))
                assert fn(n, ci, co, T, V, K, s, fl | F.BN_FROZEN) == sizes[-1], "a size depends on STGCN_BN_FROZEN"
        kernel = KERNEL_LIST.index(name(ci, co, T, V, K, s, fl).decode()) if name and name.restype is F.c_char_p else None
        entries.append([lib.stgcn_tcn_supported(ci, co, T, V, K, s, fl), kernel] + sizes)
    return [f, ci, co, K, s, lib.stgcn_tcn_packed_bytes(ci, co, K, fl), entries]


def main():
    lib = _capi.lib()
    doc = {name: {"tv": [list(x) for x in tv], "groups": [query(lib, f, ci, co, K, s, tv) for f in flags for (ci, co) in ch
                                                           for (K, s) in ks]}
           for name, (flags, ch, ks, tv) in SECTIONS.items()}
    entries = [(g[0], e) for sec in doc.values() for g in sec["groups"] for e in g[6]]
    if "--add-kernel" in sys.argv:
        with open(OUT) as fh:
            old = json.load(fh)
        strip = lambda d: {k: [g[:6] + [[e[:1] + e[2:] for e in g[6]]] for g in v["groups"]] for k, v in d.items()}  # noqa: E731
        assert strip(doc) == strip({k: old[k] for k in SECTIONS}), "a figure the earlier library wrote has changed"
    for (f, sup), n in sorted(Counter((f, e[0]) for f, e in entries).items()):
        print(f"{f:20s} supported={sup} {n}")
    names = Counter(None if e[1] is None else KERNEL_LIST[e[1]] for _, e in entries)
    for name, n in sorted(names.items(), key=str):
        print(f"{name!r:32s} {n}")
    print(f"{len(entries)} shapes")
    assert None in names or KERNELS <= set(names), f"grid misses {sorted(KERNELS - set(names))}"
    with open(OUT, "w") as fh:      # one group per line: a change of dispatch shows as a readable diff
        fh.write(json.dumps({"flag_sets": FLAG_SETS, "ws_n": list(WS_N), "frozen_sizes": "equal", "kernels": KERNEL_LIST})[:-1])
        for name, sec in doc.items():
            fh.write(',\n"%s": {"tv": %s, "groups": [\n' % (name, json.dumps(sec["tv"], separators=(",", ":"))))
            fh.write(",\n".join(json.dumps(g, separators=(",", ":")) for g in sec["groups"]))
            fh.write("\n]}")
        fh.write("}\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
