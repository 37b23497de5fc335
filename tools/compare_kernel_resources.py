#!/usr/bin/env python3
"""Compares what the compiler made of every kernel in two sets of gfx950 assembly files, by kernel name:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/FILE.hip -o DIR/FILE.s     (once per tree)
    python tools/compare_kernel_resources.py PARENT_DIR NEW_DIR > profiles/....txt

Per kernel: VGPRs, AGPRs, SGPR and VGPR spills, scratch (.private_segment_fixed_size), static LDS
(.group_segment_fixed_size) from the code object's metadata, and the number of v_mfma instructions in its body.  Exit status 1
if a kernel is missing on either side, a count rose, or an MFMA count differs.

The last column is the number of instructions in the kernel's body.  It is reported, not judged: it moves where the other
columns hold still.  ``=`` behind it: the two instruction streams are the same text once comments and the numbering of the
local labels are set aside.
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = ("vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")
SHORT = ("vgpr", "agpr", "s_spill", "v_spill", "scratch", "lds")


def kernels(path):
    """{mangled name: {field: int, 'mfma': int, 'insts': [instruction lines, labels renumbered]}} of one .s file."""
    text = open(path).read()
    out = {}
    for block in text.split("  - .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1)) for f in FIELDS}
    for name in out:
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index(".Lfunc_end")]
        out[name]["mfma"] = len(re.findall(r"^\s+v_mfma", body, re.M))
        insts = [re.sub(r"\s*;.*$", "", line).strip() for line in re.findall(r"^\s+[a-z][a-z0-9_]*(?:\s.*)?$", body, re.M)]
        labels = {}
        out[name]["insts"] = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), i) for i in insts]
    return out


def demangle(names):
    """'void stgcn::(anonymous namespace)::k<1, ns::(anonymous namespace)::Form<4, 2>, false>(float const*, ...)' ->
    'k<1, Form<4, 2>, false>': the kernel with its template arguments, namespace qualifiers dropped wherever they stand."""
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    short = [re.sub(r"^void |\(.*$", "", re.sub(r"(?:[A-Za-z_0-9]+|\(anonymous namespace\))::", "", n)) for n in r.stdout.split("\n")]
    return dict(zip(names, short))


def main():
    old_dir, new_dir = sys.argv[1:3]
    bad = same = total = 0
    print("%-58s %s | %-8s | instructions   (parent -> new; one number where they agree)" % ("kernel", " ".join("%9s" % s for s in SHORT), "mfma"))
    for old_path in sorted(glob.glob(os.path.join(old_dir, "*.s"))):
        new_path = os.path.join(new_dir, os.path.basename(old_path))
        old, new = kernels(old_path), kernels(new_path)
        print("# " + os.path.basename(old_path).replace(".s", ".hip"))
        pretty = demangle(sorted(set(old) | set(new)))
        for name in sorted(pretty, key=pretty.get):
            if name not in old or name not in new:
                print("%-58s only in the %s" % (pretty[name], "parent" if name in old else "new tree"))
                bad += 1
                continue
            o, n = old[name], new[name]
            cols = ["%9s" % (o[f] if o[f] == n[f] else "%d->%d" % (o[f], n[f])) for f in FIELDS]
            mf = "%d" % o["mfma"] if o["mfma"] == n["mfma"] else "%d->%d" % (o["mfma"], n["mfma"])
            oi, ni = len(o["insts"]), len(n["insts"])
            ins = ("%d" % oi if oi == ni else "%d->%d" % (oi, ni)) + (" =" if o["insts"] == n["insts"] else "")
            rose = [f for f in FIELDS if n[f] > o[f]]
            if rose or o["mfma"] != n["mfma"]:
                bad += 1
            total += 1
            same += o["insts"] == n["insts"]
            print("%-58s %s | %-8s | %s%s" % (pretty[name], " ".join(cols), mf, ins, "   ROSE: " + ", ".join(rose) if rose else ""))
    print("# %s" % ("no count rose, no kernel has scratch it had not, MFMA counts equal" if not bad else "%d kernels differ for the worse" % bad))
    print("# %d of %d kernels have the parent's instruction stream (=)" % (same, total))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
