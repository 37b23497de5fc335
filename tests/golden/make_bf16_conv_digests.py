"""Records SHA-256 digests of what the two older generations of bf16 matrix-core kernels compute, case by case:
tests/golden/bf16_conv_digests.json.  The generations are the 128-pixel pair of csrc/tcn_bf16.hip (tcn_mfma_bf16_kernel,
stem_mfma_bf16_kernel) and the 256-pixel persistent pair of csrc/stem_bf16_v4.hip (tcn_bf16_v4_kernel = K3v4,
stem_bf16_v4_kernel = KF4).  Run it on an MI355X against the library of the commit BEFORE a change that must not move a result
bit of these kernels (the library comes from ``STGCN_LIB``, as everywhere); tests/test_bf16_conv_digests_gpu.py imports
``cases()``, ``check_family()`` and ``run()`` and compares.

    STGCN_LIB=path/to/libstgcn_hip.so python tests/golden/make_bf16_conv_digests.py --commit <hash> [--out file.json]
    python tests/golden/make_bf16_conv_digests.py --stats kernel_stats.csv
        the instantiations of the four kernels that a recording run under ``rocprofv3 --kernel-trace --stats`` reached, against
        the ones the launchers can dispatch.  Needs no GPU.

Shapes: the smallest that reach each family and, within it, each tile-columns-per-thread count (JPR), the unrolled (K = 9) and
the runtime tap loop, the padded 64-channel layer, both tile widths of KF4 and both of its feature sources.  N = 2 clips: tiles
cross a clip boundary and the persistent kernels walk more than one tile.  Every shape runs under bf16x3 and bf16, with fp32
and bf16 results, and with each flag its family reads (STGCN_RAW for the convs, STGCN_OUT_NTVC for the stems and K3v4,
STGCN_IN_NTVC for the stems).  Each case asserts through the host queries that the family it is named for is the one that runs.

A digest covers the result tensor only.  Every case runs twice here and is written only if both runs agree.
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

N, C, S = 2, 128, 3
MATHS = {"bf16x3": 1, "bf16": 2}
OUT_BF16, RAW, IN_NTVC, OUT_NTVC = 0x10, 0x20, 0x40, 0x80
# (Cin, Cout, T, V, K, stride) of the 128-pixel conv: tile columns per thread (JPR) 1 .. 3, runtime (KT 0) and unrolled (KT 9) taps
TCN_SMALL = ((64, 128, 8, 22, 1, 2), (64, 128, 8, 22, 5, 1), (16, 64, 8, 22, 3, 1), (64, 128, 8, 46, 5, 1), (128, 128, 8, 64, 5, 2),
             (64, 128, 28, 7, 9, 2), (64, 128, 8, 22, 9, 2), (64, 128, 12, 46, 9, 2), (128, 128, 6, 46, 9, 1))
TCN_V4 = ((64, 128, 6, 33, 9, 1), (16, 64, 6, 22, 9, 1))
STEM_SMALL = ((8, 22, 5), (8, 22, 3), (2, 52, 9))        # (T, V, K)
# (T, V, math, what KF4 reads besides P): the attention's features on the 128-pixel tile, its fragments on the 256-pixel tile
STEM_V4 = ((2, 33, "bf16x3", "features"), (2, 33, "bf16", "features"), (8, 35, "bf16x3", "features"), (8, 35, "bf16", "features"),
           (2, 46, "bf16x3", "features"), (16, 23, "bf16x3", "features"), (16, 27, "bf16x3", "features"),
           (16, 27, "bf16", "fragments"), (16, 32, "bf16", "fragments"))
CONV_FLAGS = {"": 0, "-obf16": OUT_BF16, "-raw": RAW}
V4_FLAGS = dict(CONV_FLAGS, **{"-ontvc": OUT_NTVC, "-ontvc-obf16": OUT_NTVC | OUT_BF16, "-ontvc-raw": OUT_NTVC | RAW})
STEM_FLAGS = {"": 0, "-obf16": OUT_BF16, "-ontvc": OUT_NTVC, "-intvc": IN_NTVC, "-intvc-ontvc-obf16": IN_NTVC | OUT_NTVC | OUT_BF16}
FAMILIES = ("tcn_mfma_bf16_kernel", "tcn_bf16_v4_kernel", "stem_mfma_bf16_kernel", "stem_bf16_v4_kernel")
# every instantiation the launchers can dispatch, as rocprofv3 prints them (template arguments without blanks)
_B = ("false", "true")
DISPATCHABLE = ([f"tcn_mfma_bf16_kernel<{j},{t},{b},{k}>" for j in (1, 2, 3) for t in (3, 1) for b in _B for k in (9, 0)]
                + [f"tcn_bf16_v4_kernel<{t},{b}>" for t in (3, 1) for b in _B]
                + [f"stem_mfma_bf16_kernel<{p},{t},{b},{k}>" for p, k in ((3, 9), (6, 9), (9, 9), (9, 0)) for t in (3, 1) for b in _B]
                + [f"stem_bf16_v4_kernel<{p},{t},{b},{j}>" for p, j in ((6, 1), (9, 1), (4, 2), (6, 2), (9, 2)) for t in (3, 1) for b in _B])


def cases():
    """Every case as a dict with a unique ``id``, in a fixed order."""
    out = []
    for family, shapes, flagsets in ((FAMILIES[0], TCN_SMALL, CONV_FLAGS), (FAMILIES[1], TCN_V4, V4_FLAGS)):
        for Cin, Cout, T, V, K, stride in shapes:
            for math in MATHS:
                for tag, fl in flagsets.items():
                    out.append(dict(family=family, Cin=Cin, Cout=Cout, T=T, V=V, K=K, stride=stride, math=math, flags=fl,
                                    id=f"{family}-{Cin}to{Cout}-T{T}-V{V}-K{K}-s{stride}-{math}{tag}"))
    # (under bf16 no K = 9 stem reaches the 128-pixel kernel: where KF4's tiles do not fit, its own half-sized images are
    #  too small for the attention matrices staged in them, so the unrolled form runs under bf16x3 only)
    stems = ([(FAMILIES[2], T, V, K, m, None) for T, V, K in STEM_SMALL for m in MATHS if K != 9 or m == "bf16x3"]
             + [(FAMILIES[3], T, V, 9, m, f) for T, V, m, f in STEM_V4])
    for family, T, V, K, math, form in stems:
        for tag, fl in STEM_FLAGS.items():
            out.append(dict(family=family, Cin=3, Cout=C, T=T, V=V, K=K, stride=1, math=math, flags=fl, form=form,
                            id=f"{family}-T{T}-V{V}-K{K}-{math}{tag}"))
    assert len({c["id"] for c in out}) == len(out)
    return out


def check_family(c, lib):
    """The kernel family the case is named for is the one the library runs for it (and, for KF4, from the feature source
    the case names: the workspace behind P holds (N,T,V) x 64 B of features or (N,12,64) x 16 B of fragments)."""
    fl = MATHS[c["math"]] | c["flags"]
    if c["Cin"] != 3:
        got = lib.stgcn_tcn_kernel_name(c["Cin"], c["Cout"], c["T"], c["V"], c["K"], c["stride"], fl).decode()
    else:
        got = lib.stgcn_stem_kernel_name(3, C, c["T"], c["V"], c["K"], S, fl).decode()
        if c["form"]:
            a = (N, 3, C, c["T"], c["V"], c["K"], S, MATHS[c["math"]])
            part = lib.stgcn_stem_ws_bytes(*a) - (N * S * c["V"] ** 2 * 4 + 255) // 256 * 256
            assert part == {"features": N * c["T"] * c["V"] * 64, "fragments": N * 12 * 64 * 16}[c["form"]], (c["id"], part)
    assert got == c["family"], f"{c['id']}: served by {got!r}"


_inputs = {}


def inputs(c):
    """The operands of a shape, drawn once on the CPU from a generator seeded by the shape and shared (unchanged) by every
    case of that shape."""
    import torch
    key = tuple(c[k] for k in ("Cin", "Cout", "T", "V", "K", "stride"))
    if key not in _inputs:
        Cin, Cout, T, V, K, _ = key
        g = torch.Generator().manual_seed(((((Cin * 131 + Cout) * 131 + T) * 131 + V) * 131 + K) * 131 + key[5])
        r = lambda *s: torch.randn(*s, generator=g)
        u = lambda *s: torch.rand(*s, generator=g) + 0.5
        p = dict(x=r(N, Cin, T, V), Wt=r(Cout, Cin if Cin != 3 else Cout, K) / (K * max(Cin, 16)) ** 0.5, t_scale=u(Cout), t_shift=r(Cout) * 0.1)
        if Cin == 3:
            ic = Cout // 4
            p.update(A=torch.rand(S, V, V, generator=g) * 0.1, Wa=r(S, ic, 3) * 0.3, ba=r(S, ic) * 0.1, Wb=r(S, ic, 3) * 0.3,
                     bb=r(S, ic) * 0.1, Wd=r(S, Cout, 3) / 3 ** 0.5, bd=r(S, Cout) * 0.1, Wdown=r(Cout, 3) / 3 ** 0.5,
                     bdown=r(Cout) * 0.1, bn=[u(Cout), r(Cout) * 0.1], dbn=[u(Cout), r(Cout) * 0.1])
        _inputs[key] = p
    return _inputs[key]


def run(c, dev):
    """The result tensor of one case."""
    import torch
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    p = {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in inputs(c).items()}
    math, fl = MATHS[c["math"]], c["flags"]
    if c["Cin"] != 3:
        Wp = F.tcn_pack(p["Wt"], p["t_scale"], math)
        # (tcn_forward_packed with the flags F._flags() drops: STGCN_RAW, STGCN_OUT_NTVC)
        Tout = F.tcn_out_frames(c["T"], c["K"], c["stride"])
        shape = (N, Tout, c["V"], c["Cout"]) if fl & OUT_NTVC else (N, c["Cout"], Tout, c["V"])
        y = torch.full(shape, float("nan"), device=dev, dtype=torch.bfloat16 if fl & OUT_BF16 else torch.float32)
        with torch.cuda.device(dev):
            _capi.call("stgcn_tcn_forward_packed", p["x"].data_ptr(), Wp.data_ptr(), p["t_shift"].data_ptr(), y.data_ptr(), N, c["Cin"],
                       c["Cout"], c["T"], c["V"], c["K"], c["stride"], math | fl, F._stream(dev))
        return y
    x = p["x"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if fl & IN_NTVC else p["x"]
    prep = F.stem_prepare(p["Wd"], p["bd"], p["Wdown"], p["bdown"], *p["bn"], *p["dbn"], p["Wt"], p["t_scale"], math=math)
    out, _ = F.stem_forward(x, p["A"], p["Wa"], p["ba"], p["Wb"], p["bb"], prep, p["t_shift"], C, c["K"], math=math,
                            out_bf16=bool(fl & OUT_BF16), channels_last_out=bool(fl & OUT_NTVC))
    return out


def digest(result):
    import torch
    r = result.detach().contiguous() if result.is_contiguous() else result.detach().permute(0, 2, 3, 1).contiguous()   # (memory order)
    if r.dtype == torch.bfloat16:
        r = r.view(torch.int16)
    return hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest()


def record(args):
    import torch
    from stgcn_amd import _capi
    lib, dev = _capi.lib(), torch.device("cuda:0")
    digests = {}
    for c in cases():
        check_family(c, lib)
        first, second = digest(run(c, dev)), digest(run(c, dev))
        if first != second:
            print(f"NOT WRITTEN {c['id']}: two runs of the same library disagree", flush=True)
            continue
        digests[c["id"]] = first
        print(c["id"], first[:16], flush=True)
    doc = {"commit": args.commit, "library": os.path.basename(_capi.LIB_PATH), "device": f"{torch.cuda.get_device_name(0)} / {torch.cuda.get_device_properties(0).gcnArchName}",
           "rocm": torch.version.hip, "torch": torch.__version__, "digests": digests}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(digests), "of", len(cases()), "cases")


def short_name(name):
    """'void stgcn::(anonymous namespace)::k<1, 3, false, 9>(float const*, ...)' -> 'k<1,3,false,9>'."""
    m = re.search(r"stgcn::(?:\(anonymous namespace\)::)?([A-Za-z_0-9]+(?:<[^(]*>)?)", name)
    return m.group(1).replace(" ", "") if m else None


def stats(args):
    with open(args.stats, newline="") as f:
        calls = {short_name(r["Name"]): int(r["Calls"]) for r in csv.DictReader(f) if short_name(r["Name"])}
    reached = [k for k in DISPATCHABLE if k in calls]
    print(f"Instantiations of {', '.join(FAMILIES)} in one recording run of tests/golden/make_bf16_conv_digests.py "
          f"({len(cases())} cases, each run twice): {len(reached)} of the {len(DISPATCHABLE)} the launchers can dispatch.")
    print("\nreached (launches):")
    for k in reached:
        print(f"  {k}  {calls[k]}")
    print("\ndispatchable, reached by no case:")
    for k in DISPATCHABLE:
        if k not in calls:
            print(f"  {k}")
    other = sorted(k for k in calls if k.split("<")[0] in FAMILIES and k not in DISPATCHABLE)
    assert not other, f"launched but not listed as dispatchable: {other}"
    print("\nother stgcn:: kernels of the run (packing, the stem's attention):")
    for k in sorted(calls):
        if k.split("<")[0] not in FAMILIES:
            print(f"  {k}  {calls[k]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="hash of the commit whose library is recorded")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bf16_conv_digests.json"))
    ap.add_argument("--stats", help="kernel_stats.csv of a recording run under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    if args.stats:
        return stats(args)
    if not args.commit:
        ap.error("--commit is required to record")
    record(args)


if __name__ == "__main__":
    main()
