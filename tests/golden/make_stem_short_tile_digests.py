"""Records SHA-256 digests of what the fused stem's narrow three-term kernel (stem_bf16_v6_kernel, bf16x3) stores on shapes whose
clips end in a tile of at most 128 pixels: tests/golden/stem_short_tile_digests.json.  Run it on an MI355X against the library of
the commit BEFORE a change of that kernel's tile form or walk that must not move a result bit (the library comes from
``STGCN_LIB``, as everywhere); tests/test_stem_short_tile_gpu.py imports ``cases()``, ``run()`` and ``digest()`` and compares.

    STGCN_LIB=path/to/libstgcn_hip.so python tests/golden/make_stem_short_tile_digests.py --commit <hash> [--out file.json]

Shapes: 300 clips of 17 x 22 (600 tiles over 256 workgroups: a workgroup's tiles begin and end inside clips) and one headline
clip (180 x 22: fifteen full tiles and one of 120 pixels), each with (N,C,T,V) and (N,T,V,C) results.  A digest covers the result
tensor only.  Every case runs twice here and is written only if both runs agree.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "st-gcn-altformer_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

C, S, K = 128, 3, 9
BF16X3, OUT_NTVC = 1, 0x80
SHAPES = ((300, 17, 22), (1, 180, 22))        # (N, T, V)
FAMILY = "stem_bf16_v6_kernel"


def cases():
    """Every case as a dict with a unique ``id``, in a fixed order."""
    return [dict(N=N, T=T, V=V, flags=fl, id=f"{FAMILY}-N{N}-T{T}-V{V}-bf16x3{tag}")
            for N, T, V in SHAPES for tag, fl in (("", 0), ("-ontvc", OUT_NTVC))]


_inputs = {}


def inputs(c):
    """The operands of a shape, drawn once on the CPU from a generator seeded by the shape and shared (unchanged) by its cases."""
    import torch
    key = (c["N"], c["T"], c["V"])
    if key not in _inputs:
        N, T, V = key
        g = torch.Generator().manual_seed((N * 131 + T) * 131 + V)
        r = lambda *s: torch.randn(*s, generator=g)            # noqa: E731
        u = lambda *s: torch.rand(*s, generator=g) + 0.5       # noqa: E731
        ic = C // 4
        _inputs[key] = dict(x=r(N, 3, T, V), Wt=r(C, C, K) / (K * C) ** 0.5, t_scale=u(C), t_shift=r(C) * 0.1,
                            A=torch.rand(S, V, V, generator=g) * 0.1, Wa=r(S, ic, 3) * 0.3, ba=r(S, ic) * 0.1, Wb=r(S, ic, 3) * 0.3,
                            bb=r(S, ic) * 0.1, Wd=r(S, C, 3) / 3 ** 0.5, bd=r(S, C) * 0.1, Wdown=r(C, 3) / 3 ** 0.5,
                            bdown=r(C) * 0.1, bn=[u(C), r(C) * 0.1], dbn=[u(C), r(C) * 0.1])
    return _inputs[key]


def run(c, dev):
    """The result tensor of one case."""
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    got = _capi.lib().stgcn_stem_kernel_name(3, C, c["T"], c["V"], K, S, BF16X3 | c["flags"]).decode()
    assert got == FAMILY, f"{c['id']}: served by {got!r}"
    p = {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in inputs(c).items()}
    prep = F.stem_prepare(p["Wd"], p["bd"], p["Wdown"], p["bdown"], *p["bn"], *p["dbn"], p["Wt"], p["t_scale"], math=BF16X3)
    out, _ = F.stem_forward(p["x"], p["A"], p["Wa"], p["ba"], p["Wb"], p["bb"], prep, p["t_shift"], C, K, math=BF16X3,
                            out_bf16=False, channels_last_out=bool(c["flags"] & OUT_NTVC))
    return out


def digest(result):
    r = result.detach().contiguous() if result.is_contiguous() else result.detach().permute(0, 2, 3, 1).contiguous()   # (memory order)
    return hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library is recorded")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "stem_short_tile_digests.json"))
    args = ap.parse_args()
    from stgcn_amd import _capi
    dev = torch.device("cuda:0")
    digests = {}
    for c in cases():
        first, second = digest(run(c, dev)), digest(run(c, dev))
        if first != second:
            print(f"NOT WRITTEN {c['id']}: two runs of the same library disagree", flush=True)
            continue
        digests[c["id"]] = first
        print(c["id"], first[:16], flush=True)
    doc = {"commit": args.commit, "library": os.path.basename(_capi.LIB_PATH),
           "device": f"{torch.cuda.get_device_name(0)} / {torch.cuda.get_device_properties(0).gcnArchName}",
           "rocm": torch.version.hip, "torch": torch.__version__, "digests": digests}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(digests), "of", len(cases()), "cases")


if __name__ == "__main__":
    main()
