#!/usr/bin/env python3
"""Times the two older generations of bf16 matrix-core kernels (csrc/tcn_bf16.hip, csrc/stem_bf16_v4.hip) on shapes a user
runs, one library per process (``STGCN_LIB``), and compares three such runs:

    STGCN_LIB=... python tools/time_bf16_conv.py --out run.json [--clips 256] [--shapes tcn:64,128,180,22,9,2 stem:300,25,9 ...]
    python tools/time_bf16_conv.py --table parent1.json new.json parent2.json

A conv shape is tcn:Cin,Cout,T,V,K,stride (stgcn_tcn_forward_packed on weights packed once), a stem shape stem:T,V,K (the
fused stem's two launches, attention and tail, on a prepared blob, 3 -> 128 channels); every shape runs under bf16x3 and bf16.
Per row: every shape is warmed up, then ROUNDS windows of LAUNCHES launches between two HIP events; the row's figure is the
median window.  The table puts a new library between two runs of the parent's: a row is ok if the new median is no further
from the nearer parent median than the parent's own spread, the larger of |parent2 - parent1| / parent1 and the parent runs'
(max - min) / min over their windows.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

ROUNDS, LAUNCHES, WARMUP = 7, 40, 10
# The generic model's stride-2, K = 1 and K = 5 temporal convs and its K = 9 / stride 1 conv on wide frames (all the 128-pixel
# conv); K3v4 where long clips reach it (input channels K3v6 packs no weights for: 16, 80; at V = 46 its tile does not fit and
# the 128-pixel conv runs); KF4 on frames KF6 does not take (V = 25 and 27: features under bf16x3, and at V = 27 fragments
# under bf16; V = 45: the 128-pixel tile; V = 46 itself is KF6's wide form); the 128-pixel stem at K = 3.
DEFAULT = [f"tcn:{ci},{co},180,{V},{K},{s}" for V in (22, 46) for ci, co, K, s in ((64, 128, 9, 2), (128, 256, 9, 2), (64, 128, 1, 2), (128, 128, 5, 1))] \
    + ["tcn:128,128,180,46,9,1", "tcn:16,64,180,22,9,1", "tcn:80,128,180,22,9,1", "stem:300,25,9", "stem:300,27,9", "stem:200,45,9", "stem:180,22,3"]


def windows(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    return out


def run(args):
    import torch
    import make_bf16_conv_digests as mk
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    lib, dev = _capi.lib(), torch.device("cuda:0")
    mk.N = args.clips
    rows = {}
    for spec in args.shapes:
        kind, dims = spec.split(":")
        dims = [int(v) for v in dims.split(",")]
        for math, m in mk.MATHS.items():
            if kind == "tcn":
                c = dict(zip(("Cin", "Cout", "T", "V", "K", "stride"), dims))
                name = lib.stgcn_tcn_kernel_name(*dims, m).decode()
                p = {k: v.to(dev) for k, v in mk.inputs(c).items()}
                Wp = F.tcn_pack(p["Wt"], p["t_scale"], m)
                fn = lambda: F.tcn_forward_packed(p["x"], Wp, p["t_shift"], c["Cout"], c["K"], c["stride"], math=m)
            else:
                T, V, K = dims
                c = dict(Cin=3, Cout=mk.C, T=T, V=V, K=K, stride=1)
                name = lib.stgcn_stem_kernel_name(3, mk.C, T, V, K, mk.S, m).decode()
                p = {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in mk.inputs(c).items()}
                prep = F.stem_prepare(p["Wd"], p["bd"], p["Wdown"], p["bdown"], *p["bn"], *p["dbn"], p["Wt"], p["t_scale"], math=m)
                out = torch.empty(args.clips, mk.C, T, V, device=dev)
                ws = torch.empty((lib.stgcn_stem_ws_bytes(args.clips, 3, mk.C, T, V, K, mk.S, m) + 3) // 4, device=dev)
                fn = lambda: F.stem_forward(p["x"], p["A"], p["Wa"], p["ba"], p["Wb"], p["bb"], prep, p["t_shift"], mk.C, K, math=m, out=out, ws=ws)
            with torch.no_grad():
                w = windows(fn)
            rows[f"{spec} {math} {name}"] = w
            print(f"{spec:28s} {math:7s} {name:24s} median {statistics.median(w):9.1f} us  windows {[round(v, 1) for v in w]}", flush=True)
            del p, fn
        mk._inputs.clear()
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump({"library": os.path.basename(_capi.LIB_PATH), "clips": args.clips, "rows": rows}, f, indent=1)


def table(paths):
    p1, new, p2 = (json.load(open(p))["rows"] for p in paths)
    print("median us per call (%d windows of %d launches)" % (ROUNDS, LAUNCHES))
    print("%-62s %10s %10s %10s %8s %8s %7s  verdict" % ("shape, arithmetic, kernel", "parent", "new", "parent", "new/par", "par/par", "in-run"))
    outside = 0
    for k in p1:
        a, n, b = (statistics.median(r[k]) for r in (p1, new, p2))
        inrun = max((max(r[k]) - min(r[k])) / min(r[k]) for r in (p1, p2))
        spread = max(abs(b - a) / a, inrun)
        near = a if abs(n - a) <= abs(n - b) else b
        ok = abs(n - near) / near <= spread
        outside += not ok
        verdict = "ok" if ok else "OUTSIDE (slower)" if n > near else "outside (faster)"
        print("%-62s %10.1f %10.1f %10.1f %8.3f %8.3f %7.3f  %s" % (k, a, n, b, n / a, b / a, inrun, verdict))
    print("# %d rows, %d outside the parent's spread" % (len(p1), outside))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="time_bf16_conv.json")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--shapes", nargs="*", default=DEFAULT)
    ap.add_argument("--table", nargs=3, metavar=("PARENT1", "NEW", "PARENT2"))
    args = ap.parse_args()
    table(args.table) if args.table else run(args)


if __name__ == "__main__":
    main()
