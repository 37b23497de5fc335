"""Records what the graph conv's forward entry points compute and launch, case by case, from the commit BEFORE its kernel
choice moved behind plan_attention / plan_agcn_expand (csrc/agcn.hip):

    STGCN_LIB=path/to/libstgcn_hip.so python tests/golden/make_agcn_digests.py --commit <hash> [--out file.json]
        tests/golden/agcn_digests.json: per case the SHA-256 of its result tensors (P; y or the stem's out; for training
        cases also the saved statistics and the running buffers — never a workspace), or "STATUS: message" where the call is
        refused.  Every case runs twice and is written only if both runs agree.  Needs an MI355X.
    python tests/golden/make_agcn_digests.py --commit <hash> --trace kernel_trace.csv [--dispatch-out file.json]
        tests/golden/agcn_dispatch.json from the kernel trace of the run above under
        ``rocprofv3 --kernel-trace --output-format csv -- python ...``: per case every stgcn:: dispatch as
        [name with template arguments, grid in workgroups, workgroup size, LDS bytes].  ``--compare fixture.json`` prints the
        differences against a recorded fixture instead of writing one.  Needs no GPU.

tests/test_agcn_digests_gpu.py and tests/test_agcn_dispatch.py import ``cases()`` and ``run()``.  A stgcn_bn_fold over
256 * (MARK + i) channels in front of case i marks the cases in the trace (no case launches that kernel itself).

Shapes: N = 2, T = 8, three subsets, inter_c = Cout / 4 unless a case says otherwise — the smallest that reach every kernel
and instantiation of both plans and every chunking branch.  Found with the name queries, against the first list drawn up:
the fused stem asks for features only at V = 23 or 25..47 odd-or-narrow frames with T >= 40 (V = 22 and every even wide frame
take fragments), so features run at V = 23, 27 and 45 (<1,16> with P behind the Gram matrix, <2,16>, <6,8>); <12,8> WITH
features (V = 48..51) is reached by no entry point, <12,8> without (V = 54) is; <2,8> needs the stem's attention called with
inter_c = 1024.
"""
import argparse
import csv
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "st-gcn-altformer_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

MARK = 1000
BF16X3, F16MX = 1, 1 | 0x400
KERNELS = ([f"attention_folded_kernel<{a}>" for a in ("1,16", "2,16", "4,16", "2,8", "6,8", "12,8")]
           + [f"attention_generic_mfma_kernel<{k},{m}>" for m in (1, 2) for k in (16, 32, 64)]
           + [f"attention_generic_kernel<{i}>" for i in (2, 4, 9, 16)]
           + ["agcn_expand_small4_kernel<3,3>", "agcn_expand_small_kernel<3,3>", "agcn_expand_mfma_kernel<1,8>",
              "agcn_expand_mfma_kernel<1,16>", "agcn_expand_mfma_kernel<2,16>", "agcn_expand_generic_kernel"])


def cases():
    """Every case as a dict with a unique ``id``, in a fixed order."""
    out = []

    def add(kind, Cin, Cout, V, T=8, N=2, S=3, extra=0, **kw):
        c = dict(kind=kind, N=N, Cin=Cin, Cout=Cout, T=T, V=V, S=S, extra=extra, inter_c=max(Cout // 4, 1), **kw)
        c["id"] = f"{kind}-N{N}-{Cin}to{Cout}-T{T}-V{V}" + "".join(f"-{k}{v}" for k, v in sorted(kw.items())) + (f"-S{S}" if S != 3 else "")
        out.append(c)
    for V in (22, 27, 46, 54):                                  # folded <1,16> <2,16> <4,16> <12,8>
        add("attention", 3, 128, V)
    add("attention", 3, 128, 22, T=310)                         # two frame chunks, the second ragged
    for V in (22, 46):                                          # generic MFMA <16|32|64, 1|2>
        for Cin in (64, 128, 256):
            add("attention", Cin, Cin, V)
    add("attention", 64, 64, 22, T=4, N=130)                    # ... with grid.y = 1
    for Cin, V in ((6, 22), (6, 32), (6, 46), (3, 64)):         # generic VALU <2> <4> <9> <16>
        add("attention", Cin, 24 if Cin == 6 else 32, V)
    add("attention", 3, 128, 65)                                # refused
    add("attention", 1, 4, 1, T=1, N=65536)                     # refused
    # (extra: what the stem's attention writes besides P, as the name query counts it; queries() checks it against the workspace)
    add("stem", 3, 128, 22, math=BF16X3, extra=2)               # fragments
    add("stem", 3, 128, 46, math=BF16X3, extra=3)               # fragments of the wide split
    add("stem", 3, 128, 22, math=F16MX, extra=2)                # fragments and bounds (KF7)
    for V in (23, 27, 45):                                      # features
        add("stem", 3, 128, V, T=40, math=BF16X3, extra=1)
    add("stem", 3, 128, 23, T=40, math=BF16X3, ic=1024, extra=1)   # features from <2,8>
    add("forward", 3, 128, 22)                                  # small4
    add("forward", 3, 128, 22, T=50)                            # small4, two chunks, ragged tail
    add("forward", 3, 128, 25, T=9)                             # small (T*V % 4 != 0)
    for Cout in (64, 128, 256):                                 # mfma <1,8> <1,16> <2,16>
        add("forward", 64, Cout, 22, down=1)
    add("forward", 64, 64, 22)                                  # mfma, identity residual
    add("forward", 6, 24, 22)                                   # generic
    add("train", 3, 128, 22, save="stats")                      # the stem class on the moments path
    add("train", 3, 128, 22, save="branches")
    add("train", 64, 128, 22, save="stats")                     # conv_down as a plain product
    add("train", 64, 64, 22, save="stats")                      # identity residual
    add("train", 3, 128, 22, save="stats", frozen=1)
    add("train", 3, 128, 22, save="branches", S=1)              # Cin = 3 outside the stem class: the generic expansion, twice
    for c in out:
        if "ic" in c:
            c["inter_c"] = c["ic"]
        c["has_down"] = bool(c["Cin"] != c["Cout"] or c.get("down"))
    assert len({c["id"] for c in out}) == len(out)
    return out


def queries(c, lib):
    """(attention query arguments or None, [expansion query arguments in launch order]) of a case."""
    shape = (c["N"], c["Cin"], c["T"], c["V"])
    exp = (c["N"], c["Cin"], c["Cout"], c["T"], c["V"], c["S"])
    if c["kind"] == "stem":
        a = (c["N"], 3, c["Cout"], c["T"], c["V"], 9, 3, c["math"])
        # the workspace part behind P has the size of what the case declares (x is contiguous: no channel-major copy of it);
        # KF7's bounds add 256 B
        part = lib.stgcn_stem_ws_bytes(*a) - (c["N"] * 3 * c["V"] ** 2 * 4 + 255) // 256 * 256
        sizes = {1: c["N"] * c["T"] * c["V"] * 64, 2: c["N"] * 12288, 3: c["N"] * 49152}
        assert part - (256 if c["math"] == F16MX else 0) == sizes[c["extra"]], (c["id"], part)
        return shape + (c["inter_c"], 3, c["extra"]), []
    att = shape + (c["inter_c"], c["S"], 0)
    if c["kind"] == "attention":
        return att, []
    if c["kind"] == "forward":
        return att, [exp + (int(c["has_down"]),)]
    if c["Cin"] == 3 and c["S"] == 3 and c["save"] == "stats" and not c.get("frozen"):
        return att, [exp + (1,)]                    # the moments path
    return att, [exp + (1,), exp + (1,)] if c["Cin"] == 3 else [exp + (0,)]   # both branches expanded / conv_down as a product


_inputs = {}


def inputs(c):
    """The operands of a case, drawn once on the CPU from a generator seeded by its shape and left unchanged."""
    import torch
    key = c["id"]
    if key not in _inputs:
        N, Cin, Cout, T, V, S, ic = (c[k] for k in ("N", "Cin", "Cout", "T", "V", "S", "inter_c"))
        g = torch.Generator().manual_seed(100003 * Cin + 1009 * V + 31 * T + Cout + ic)
        r = lambda *s: torch.randn(*s, generator=g)
        u = lambda *s: torch.rand(*s, generator=g) + 0.5
        p = dict(x=r(N, Cin, T, V), A=torch.rand(S, V, V, generator=g) * 0.1, Wa=r(S, ic, Cin) * 0.3, ba=r(S, ic) * 0.1,
                 Wb=r(S, ic, Cin) * 0.3, bb=r(S, ic) * 0.1, Wd=r(S, Cout, Cin) / Cin ** 0.5, bd=r(S, Cout) * 0.1,
                 Wdown=r(Cout, Cin) / Cin ** 0.5, bdown=r(Cout) * 0.1, bn=[u(Cout), r(Cout) * 0.1, r(Cout) * 0.3, u(Cout)],
                 dbn=[u(Cout), r(Cout) * 0.1, r(Cout) * 0.3, u(Cout)], Wt=r(Cout, Cout, 9) / (9 * Cout) ** 0.5,
                 t_scale=u(Cout), t_shift=r(Cout) * 0.1)
        _inputs[key] = p
    return _inputs[key]


def run(c, dev):
    """The result tensors of one case, in a fixed order; "STATUS: message" where the library refuses it."""
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    p = {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in inputs(c).items()}
    att = (p["x"], p["A"], p["Wa"], p["ba"], p["Wb"], p["bb"])
    down = (p["Wdown"], p["bdown"]) if c["has_down"] else (None, None)
    try:
        if c["kind"] == "attention":
            return [F.agcn_attention(*att)]
        if c["kind"] == "forward":
            y, P = F.agcn_forward(*att, p["Wd"], p["bd"], *down, p["bn"][0], p["bn"][1],
                                  *((p["dbn"][0], p["dbn"][1]) if c["has_down"] else (None, None)))
            return [P, y]
        if c["kind"] == "stem":
            prep = F.stem_prepare(p["Wd"], p["bd"], p["Wdown"], p["bdown"], p["bn"][0], p["bn"][1], p["dbn"][0], p["dbn"][1],
                                  p["Wt"], p["t_scale"], math=c["math"])
            out, P = F.stem_forward(*att, prep, p["t_shift"], c["Cout"], 9, math=c["math"])
            return [P, out]
        bn, dbn = [t.clone() for t in p["bn"]], [t.clone() for t in p["dbn"]] if c["has_down"] else None
        y, P, zm, zd, stats = F.agcn_forward_train(*att, p["Wd"], p["bd"], *down, bn, dbn,
                                                   save="branches" if c["save"] == "branches" else True,
                                                   frozen=bool(c.get("frozen")))
        # (the last float of the statistics block is a spare no path writes)
        return [P, y, stats[:-1]] + bn[2:] + (dbn[2:] if dbn else []) + [t for t in (zm, zd) if t is not None]
    except _capi.StgcnError as e:
        return str(e).split(" -> ", 1)[1]


def digest(result):
    if isinstance(result, str):
        return result
    h = hashlib.sha256()
    for t in result:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def record(args):
    import torch
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    lib, dev = _capi.lib(), torch.device("cuda:0")
    named = hasattr(lib, "stgcn_agcn_attention_kernel_name")     # (the recorded commit has no name queries: its trace tells)
    digests, reached = {}, set()
    ones = torch.ones(256 * (MARK + len(cases())), device=dev)
    for i, c in enumerate(cases()):
        n = 256 * (MARK + i)
        F.bn_fold(ones[:n], ones[:n], ones[:n], ones[:n])
        first, second = digest(run(c, dev)), digest(run(c, dev))
        names = []
        if named:
            a, e = queries(c, lib)
            names = [lib.stgcn_agcn_attention_kernel_name(*a).decode()] + [lib.stgcn_agcn_expand_kernel_name(*q).decode() for q in e]
            reached.update(names)
        if first != second:
            print(f"NOT WRITTEN {c['id']}: two runs of the same library disagree", flush=True)
            continue
        digests[c["id"]] = first
        print(c["id"], first if first.startswith("STGCN_") else first[:16], *names, flush=True)
    torch.cuda.synchronize()
    if named:
        missing = sorted(set(KERNELS) - reached)
        assert not missing, f"no case reaches {missing}"
    doc = {"commit": args.commit, "library": os.path.basename(_capi.LIB_PATH), "device": torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName,
           "rocm": torch.version.hip, "torch": torch.__version__, "digests": digests}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(digests), "of", len(cases()), "cases")


def short_name(name):
    """'void stgcn::(anonymous namespace)::k<1, 16>(float const*, ...)' -> 'k<1,16>'."""
    m = re.search(r"stgcn::(?:\(anonymous namespace\)::)?([A-Za-z_0-9]+(?:<[^(]*>)?)", name)
    return m.group(1).replace(" ", "") if m else None


def dispatches_by_case(path):
    """{case id: the stgcn:: dispatches of ONE run of the case} from a rocprofv3 kernel trace; the two runs must agree."""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    cs, per, cur = cases(), {}, None
    for r in rows:
        name = short_name(r["Kernel_Name"])
        if name is None:
            continue
        wg = [int(r[f"Workgroup_Size_{d}"]) for d in "XYZ"]
        grid = [int(r[f"Grid_Size_{d}"]) // w for d, w in zip("XYZ", wg)]
        if name == "bn_fold_kernel" and MARK <= grid[0] < MARK + len(cs):
            cur = per.setdefault(cs[grid[0] - MARK]["id"], [])
        elif cur is not None:
            cur.append([name, grid, wg, int(r["LDS_Block_Size"])])
    out = {}
    for c in cs:
        d = per[c["id"]]
        half = len(d) // 2
        assert d[:half] == d[half:], f"{c['id']}: the two runs launched differently"
        out[c["id"]] = d[:half]
    return out


def trace(args):
    got = dispatches_by_case(args.trace)
    names = {d[0] for v in got.values() for d in v}
    missing = sorted(set(KERNELS) - names)
    assert not missing, f"no case reaches {missing}"
    if args.compare:
        with open(args.compare) as f:
            want = json.load(f)
        bad = [k for k in want["cases"] if want["cases"][k]["dispatches"] != got.get(k)]
        n = sum(len(v["dispatches"]) for v in want["cases"].values())
        print(f"{args.trace} against {args.compare} (recorded from {want['commit'][:7]}): {len(want['cases'])} cases, {n} stgcn:: "
              f"dispatches per run, {len(names)} distinct kernels; name, grid, workgroup size and LDS bytes "
              + ("agree dispatch by dispatch" if not bad else f"DIFFER in {bad}"))
        for k in bad:
            print(k, "\n  recorded", want["cases"][k]["dispatches"], "\n  traced  ", got.get(k))
        for k, v in want["cases"].items():
            print(k, " | ".join(f"{d[0]} grid {d[1]} wg {d[2]} lds {d[3]}" for d in v["dispatches"]) or "(refused: nothing launched)")
        sys.exit(1 if bad else 0)
    doc = {"commit": args.commit, "cases": {}}
    for c in cases():
        a, e = queries_offline(c)
        doc["cases"][c["id"]] = {"attention_query": a, "expand_queries": e, "dispatches": got[c["id"]]}
    with open(args.dispatch_out, "w") as f:       # one line per case
        f.write('{"commit": %s, "cases": {\n' % json.dumps(doc["commit"]))
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in doc["cases"].items()) + "\n}}\n")
    print(args.dispatch_out, len(doc["cases"]), "cases")


def queries_offline(c):
    from stgcn_amd import _capi
    a, e = queries(c, _capi.lib())
    return list(a), [list(q) for q in e]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library is recorded")
    ap.add_argument("--out", default=os.path.join(here, "agcn_digests.json"))
    ap.add_argument("--trace", help="rocprofv3 kernel trace (csv) of a recording run")
    ap.add_argument("--dispatch-out", default=os.path.join(here, "agcn_dispatch.json"))
    ap.add_argument("--compare", help="dispatch fixture to compare the trace with")
    args = ap.parse_args()
    trace(args) if args.trace else record(args)


if __name__ == "__main__":
    main()
