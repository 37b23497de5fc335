#!/usr/bin/env python3
"""Counts that the one-wave-per-SIMD kernels (KF6, KF6-wide, K3v6) are held to, read from hipcc's gfx950 assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -S st-gcn-altformer_amd/csrc/stem_bf16_v6.hip -o v6.s
    python tools/kf6_isa_counts.py v6.s [--kernel stem_bf16_v6_kernelILi3ELb0ELb0]

Per kernel whose mangled name contains --kernel (default: every kernel with a loop of >= 256 MFMAs):
  * main loop: instructions, MFMAs, v_accvgpr_* copies and s_waitcnt of the innermost loop that holds the MFMAs (one trip =
    one period of 9 pairs); a kernel with a short tile form has two such loops: the smaller is reported as the main loop and
    both are listed beside it;
  * tile loop: global_load_dwordx4 (LDS-DMAs excluded: those are global_load_lds_*) and scratch_* / buffer_*_offen scratch use;
  * tile tail: global_store_* instructions behind the main loop, and the `s_waitcnt vmcnt` that stand between the first and
    the last of them in program order, basic blocks ignored (every form of the epilogue is counted: divide by the forms);
  * result stores: every basic block of the tile loop's tail with >= 8 global_store_dwordx{2,4}: how many stores, and how
    many `s_waitcnt vmcnt` stand between its first and its last store (0 = the stores issue back to back);
  * resources from the kernel's metadata: .vgpr_count, .agpr_count, .sgpr_spill_count, .vgpr_spill_count and
    .private_segment_fixed_size (scratch bytes per lane).
"""
import argparse
import re
import sys

LABEL = re.compile(r"^([.\w$]+):")
INSTR = re.compile(r"^\s+([a-z_][\w.]*)\b(.*)")
BRANCH = re.compile(r"^s_(?:cbranch\w+|branch)$")


def kernels(lines):
    """(name, [lines]) per kernel: from its label to s_endpgm."""
    out, name, body = [], None, []
    for ln in lines:
        m = LABEL.match(ln)
        if m and m.group(1).startswith("_Z") and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(ln)
            if ln.strip().startswith(".end_amdhsa_kernel") or ln.strip() == ".cfi_endproc" or re.match(r"^\.Lfunc_end", ln):
                out.append((name, body))
                name = None
    return out


def analyse(name, body):
    ins = []          # (mnemonic, operands, label-or-None)
    labels = {}
    for ln in body:
        m = LABEL.match(ln)
        if m:
            labels[m.group(1)] = len(ins)
            ins.append(("<label>", m.group(1)))
            continue
        if ln.lstrip().startswith((".", ";")):
            continue
        m = INSTR.match(ln)
        if m:
            ins.append((m.group(1), m.group(2).split(";")[0].strip()))
    loops = []        # (start, end) of backward branches
    for i, (op, arg) in enumerate(ins):
        if BRANCH.match(op) and arg in labels and labels[arg] < i:
            loops.append((labels[arg], i))
    def count(a, b, pred):
        return sum(1 for op, arg in ins[a:b + 1] if op != "<label>" and pred(op, arg))
    mf = lambda op, arg: op.startswith("v_mfma")
    with_mfma = [(a, b) for a, b in loops if count(a, b, mf) >= 256]
    if not with_mfma:
        return None
    main = min(with_mfma, key=lambda l: l[1] - l[0])
    tile = max((l for l in loops if l[0] <= main[0] and l[1] >= main[1]), key=lambda l: l[1] - l[0])
    # every innermost MFMA loop: a kernel with a short tile form has two main loops (the short form's is the smaller `main`)
    inner = [l for l in with_mfma if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in with_mfma)]
    res = {
        "kernel": name,
        "main_loops": [{"instructions": count(*l, lambda op, arg: True), "mfma": count(*l, mf),
                        "v_accvgpr": count(*l, lambda op, arg: op.startswith("v_accvgpr"))} for l in inner],
        "main_loop": {
            "instructions": count(*main, lambda op, arg: True),
            "mfma": count(*main, mf),
            "v_accvgpr": count(*main, lambda op, arg: op.startswith("v_accvgpr")),
            "s_waitcnt": count(*main, lambda op, arg: op == "s_waitcnt"),
        },
        "tile_loop": {
            "global_load_dwordx4": count(*tile, lambda op, arg: op == "global_load_dwordx4"),
            "scratch": count(*tile, lambda op, arg: op.startswith("scratch_") or "offen" in arg and op.startswith("buffer_") and "s[0:3]" in arg),
        },
        "store_blocks": [],
    }
    tail = ins[main[1] + 1:tile[1] + 1]
    st_all = [k for k, (op, arg) in enumerate(tail) if op.startswith("global_store")]
    res["tile_tail"] = {
        "global_stores": len(st_all),
        "vmcnt_waits_between_first_and_last": sum(1 for op, arg in tail[st_all[0]:st_all[-1] + 1]
                                                  if op == "s_waitcnt" and "vmcnt" in arg) if st_all else 0,
    }
    # basic blocks of the tile loop behind the main loop
    blk = []
    def flush():
        st = [k for k, (op, arg) in enumerate(blk) if op in ("global_store_dwordx4", "global_store_dwordx2")]
        if len(st) >= 8:
            waits = sum(1 for op, arg in blk[st[0]:st[-1] + 1] if op == "s_waitcnt" and "vmcnt" in arg)
            res["store_blocks"].append({"stores": len(st), "vmcnt_waits_between": waits})
    for op, arg in ins[main[1] + 1:tile[1] + 1]:
        if op == "<label>" or BRANCH.match(op):
            flush()
            blk = []
        else:
            blk.append((op, arg))
    flush()
    return res


def resources(text, name):
    """The kernel's entry in the amdhsa.kernels metadata."""
    out = {}
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\s*\n", text)
    if not m:
        return out
    a = text.rfind("  - .agpr_count", 0, m.start())
    b = text.find("\n  - ", m.end())
    blk = text[a:b if b > 0 else len(text)]
    for key in ("vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
        k = re.search(r"\." + key + r":\s+(\d+)", blk)
        if k:
            out[key] = int(k.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="")
    a = ap.parse_args()
    found = False
    text = open(a.asm).read()
    for name, body in kernels(text.splitlines()):
        if a.kernel not in name:
            continue
        r = analyse(name, body)
        if r is None:
            continue
        found = True
        print(r["kernel"])
        print("  main loop (one period):", r["main_loop"])
        if len(r["main_loops"]) > 1:
            print("  every main loop (short and full tile form):", r["main_loops"])
        print("  tile loop:", r["tile_loop"])
        print("  tile tail:", r["tile_tail"])
        print("  resources:", resources(text, name))
        for b in r["store_blocks"]:
            print("  store block:", b)
    if not found:
        sys.exit("no matching kernel with an MFMA loop")


if __name__ == "__main__":
    main()
