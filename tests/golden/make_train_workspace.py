#!/usr/bin/env python3
"""Workspace-size fixture: what tests/test_train_workspace.py holds the library's non-stem size queries to.

    python tests/golden/make_train_workspace.py          # loads STGCN_LIB, else the in-tree libstgcn_hip.so

No GPU needed: the size queries are host functions.  The Python wrappers allocate exactly what these queries return, so a
carve inside the library that runs past its own size query writes into a neighbouring allocation; the fixture pins every
size to the byte.  Writes train_workspace.json with one section per query (SECTIONS: the argument names, then the sizes):
  * agcn_fwd      stgcn_agcn_train_ws_bytes      materialise 0 / 1, the stem class (Cin = 3, 3 subsets), a stem-class shape too
                                                 wide for the moments kernel (V = 120), and Cin 64 / 128 with 2 subsets
  * agcn_bwd      stgcn_agcn_backward_ws_bytes   recompute 0 - 3; shapes the moment form covers and shapes it does not
                                                 (identity residual, Cout = 192, 2 subsets, V = 64, V = 65 -> 0); N below and
                                                 above the moment form's grid cap of 256
  * tcn           stgcn_tcn_train_ws_bytes and stgcn_tcn_backward_ws_bytes on the same arguments: each math mode, with and
                                                 without BN_FROZEN (must not change a size), stride 1 / 2, K 1 / 3 / 8 / 9, V inside
                                                 and outside the one-wave wgrad's 17 - 24, Cin 3 / 64 / 128, T = 1 (no output
                                                 frame for K = 8 at stride 1 -> 0)
  * st_attention  stgcn_st_attention_ws_bytes    passes 0, 1, 2 (and -1, 3 -> 0)
  * vit_block     stgcn_vit_block_ws_bytes       batches below and above one slab of sequences
Every section ends with a base row whose arguments are set to 0 and to -1 one at a time (-> 0).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))

from stgcn_amd import _capi  # noqa: E402

OUT = os.path.join(HERE, "train_workspace.json")

F = _capi
FLAG_SETS = {"f32": F.MATH_F32, "f32_valu": F.MATH_F32_VALU, "bf16x3": F.MATH_BF16X3, "bf16": F.MATH_BF16}
FLAG_SETS.update({k + "+frozen": FLAG_SETS[k] | F.BN_FROZEN for k in ("f32", "bf16x3")})

# section -> (argument names, queries answered on those arguments)
SECTIONS = {
    "agcn_fwd": (["N", "Cin", "Cout", "T", "V", "S", "materialise"], ["stgcn_agcn_train_ws_bytes"]),
    "agcn_bwd": (["N", "Cin", "Cout", "T", "V", "S", "recompute"], ["stgcn_agcn_backward_ws_bytes"]),
    "tcn": (["N", "Cin", "Cout", "T", "V", "K", "stride", "flags"], ["stgcn_tcn_train_ws_bytes", "stgcn_tcn_backward_ws_bytes"]),
    "st_attention": (["N", "Cin", "Cout", "dk", "T", "V", "heads", "pass"], ["stgcn_st_attention_ws_bytes"]),
    "vit_block": (["B", "L", "D", "hidden"], ["stgcn_vit_block_ws_bytes"]),
}


def degenerate(base, skip=()):
    """The base row with each integer argument in turn at 0 and at -1."""
    return [base[:i] + (bad,) + base[i + 1:] for i in range(len(base)) if i not in skip for bad in (0, -1)]


def grid():
    g = {}
    tv = [(180, 22), (40, 46), (9, 7), (20, 25)]
    g["agcn_fwd"] = [(N, cin, cout, T, V, S, m) for N in (1, 64, 300) for (cin, S) in ((3, 3), (3, 2), (64, 2), (128, 2), (64, 3))
                     for cout in (64, 128, 256) for (T, V) in tv + [(12, 120)] for m in (0, 1)]
    g["agcn_fwd"] += degenerate((64, 3, 128, 180, 22, 3, 0), skip=(6,))
    layers = [(3, 64, 3), (3, 128, 3), (3, 192, 3), (3, 256, 3), (3, 128, 2), (64, 64, 2), (64, 128, 2), (128, 256, 2), (128, 128, 3)]
    g["agcn_bwd"] = [(N, cin, cout, T, V, S, r) for N in (1, 64, 300) for (cin, cout, S) in layers
                     for (T, V) in [(180, 22), (40, 46), (9, 7), (30, 64), (30, 65)] for r in (0, 1, 2, 3)]
    g["agcn_bwd"] += degenerate((64, 3, 128, 180, 22, 3, 0), skip=(6,))
    g["tcn"] = [(N, cin, cout, T, V, K, s, f) for (N, T) in ((8, 180), (256, 20), (8, 1)) for f in FLAG_SETS
                for (cin, cout) in ((3, 64), (64, 64), (64, 128), (128, 256)) for V in (7, 22, 25) for K in (1, 3, 8, 9)
                for s in (1, 2)]
    g["tcn"] += [(N, cin, 128, 60, V, 9, s, f) for N in (2, 64) for f in ("f32", "bf16x3", "bf16") for cin in (64, 128)
                 for V in (16, 17, 24) for s in (1, 2)]
    g["tcn"] += degenerate((8, 64, 128, 180, 22, 9, 1, "bf16x3"), skip=(7,))
    g["st_attention"] = [(N, cin, cout, cout // 4, T, V, h, p) for N in (1, 64, 300) for (cin, cout) in ((3, 64), (64, 64), (64, 128), (128, 256))
                         for (T, V) in ((180, 22), (20, 25), (9, 46)) for h in (4, 8) for p in (0, 1, 2)]
    g["st_attention"] += [(64, 64, 128, 32, 20, 25, 8, p) for p in (-1, 3)]
    g["st_attention"] += degenerate((64, 64, 128, 32, 20, 25, 8, 1), skip=(7,))
    g["vit_block"] = [(B, L, D, H) for B in (1, 8, 300, 4000) for L in (22, 180, 500) for D in (64, 256) for H in (256, 1024)]
    g["vit_block"] += degenerate((8, 180, 256, 1024))
    return g


def query(lib, section, args):
    """One fixture row: the arguments, then the size every query of the section returns for them."""
    call = [FLAG_SETS[a] if isinstance(a, str) else a for a in args]
    return list(args) + [getattr(lib, fn)(*call) for fn in SECTIONS[section][1]]


def check_coverage(rows):
    """The grid reaches every branch of the plans, by shape class (the library itself cannot be asked which path it sized)."""
    def need(section, classes, key):
        seen = {key(r) for r in rows[section]}
        assert classes <= seen, f"{section}: grid misses {sorted(classes - seen)}"

    def size(section, args, which=-1):
        hit = [r for r in rows[section] if tuple(r[:len(args)]) == tuple(args)]
        assert len(hit) == 1, (section, args)
        return hit[0][which]

    pos = lambda r, n: all(isinstance(a, str) or a > 0 for a in r[:n])
    # agcn forward: materialise x stem class x Cout; the moments scratch is smaller than the two branches, and only there
    need("agcn_fwd", {(m, stem, c) for m in (0, 1) for stem in (False, True) for c in (64, 128, 256)},
         lambda r: (r[6], r[1] == 3 and r[5] == 3, r[2]))
    assert size("agcn_fwd", (64, 3, 128, 180, 22, 3, 0)) < size("agcn_fwd", (64, 3, 128, 180, 22, 3, 1))
    assert size("agcn_fwd", (64, 3, 128, 12, 120, 3, 0)) == size("agcn_fwd", (64, 3, 128, 12, 120, 3, 1))   # too wide for the moments
    assert size("agcn_fwd", (64, 64, 128, 180, 22, 2, 0)) == size("agcn_fwd", (64, 64, 128, 180, 22, 2, 1))
    # agcn backward: recompute x {moment form covers it, identity residual, Cout 192, V 64, V 65} x N around 256
    kind = lambda r: ("v65" if r[4] == 65 else "v64" if r[4] == 64 else "identity" if r[1] == r[2] else
                      "c192" if r[2] == 192 else "moment" if (r[1], r[5]) == (3, 3) else "generic")
    need("agcn_bwd", {(rc, k, big) for rc in (0, 1, 2, 3) for k in ("moment", "identity", "c192", "v64", "v65", "generic")
                      for big in (False, True)}, lambda r: (r[6], kind(r), r[0] > 256))
    assert all(r[-1] == 0 for r in rows["agcn_bwd"] if r[4] == 65)
    assert all(r[-1] > 0 for r in rows["agcn_bwd"] if r[4] <= 64 and pos(r, 6))
    moment = [size("agcn_bwd", (300, 3, 128, 180, 22, 3, rc)) for rc in (0, 1, 2, 3)]
    assert moment[0] == moment[1] < moment[2] < moment[3], moment          # the moment form needs neither branch
    generic = [size("agcn_bwd", (300, 3, 192, 180, 22, 3, rc)) for rc in (0, 1, 2, 3)]
    assert generic[0] == generic[2] < generic[1] == generic[3], generic
    # tcn: math x frozen x stride x K x V inside / outside 17-24 x Cin
    need("tcn", {(f, s, K, 17 <= V <= 24, cin) for f in FLAG_SETS for s in (1, 2) for K in (1, 3, 8, 9) for V in (7, 22)
                 for cin in (3, 64, 128)}, lambda r: (r[7], r[6], r[5], 17 <= r[4] <= 24, r[1]))
    for r in rows["tcn"]:
        if r[7].endswith("+frozen"):
            plain = r[:7] + [r[7][:-len("+frozen")]]
            assert r[8:] == [size("tcn", plain, 8), size("tcn", plain, 9)], f"BN_FROZEN changes a size: {r}"
    empty = [r for r in rows["tcn"] if pos(r, 7) and r[8] == 0]
    assert empty and all(r[3] == 1 and r[5] == 8 and r[9] == 0 for r in empty), "T that leaves no output frame"
    up, plain = size("tcn", (8, 64, 128, 180, 22, 9, 2, "bf16x3")), size("tcn", (8, 64, 128, 180, 22, 8, 2, "bf16x3"))
    assert up > plain, "stride 2 with odd K: the upsampled gradient and the dgrad-by-forward regions"
    assert size("tcn", (8, 64, 128, 180, 22, 9, 1, "bf16x3")) > size("tcn", (8, 64, 128, 180, 22, 9, 1, "f32"))   # wgrad partials
    need("st_attention", {0, 1, 2, -1, 3}, lambda r: r[7])
    assert all((r[-1] > 0) == (pos(r, 7) and 0 <= r[7] <= 2) for r in rows["st_attention"])
    assert size("vit_block", (300, 500, 256, 1024)) == size("vit_block", (4000, 500, 256, 1024))   # slabs: no growth with B
    for section in rows:   # zero and negative arguments
        n = len(SECTIONS[section][0])
        bad = [r for r in rows[section] if not pos(r, n - 1 if section in ("agcn_fwd", "agcn_bwd", "st_attention") else n)]
        assert len(bad) >= 2 * (n - 1) and all(set(r[n:]) == {0} for r in bad), section


def main():
    lib = _capi.lib()
    rows = {s: [query(lib, s, a) for a in args] for s, args in grid().items()}
    check_coverage(rows)
    total = 0
    with open(OUT, "w") as fh:      # one row per line: a change of a size shows as a readable diff
        head = json.dumps({"flag_sets": FLAG_SETS, "sections": {s: {"args": a, "queries": q} for s, (a, q) in SECTIONS.items()}})
        fh.write(head[:-1] + ', "rows": {\n')
        for i, (s, rs) in enumerate(rows.items()):
            fh.write(f'"{s}": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rs) + "\n]" +
                     (",\n" if i + 1 < len(rows) else "\n"))
            print(f"{s:14s} {len(rs)} rows")
            total += len(rs)
        fh.write("}}\n")
    print(f"{total} rows, wrote", OUT)


if __name__ == "__main__":
    main()
