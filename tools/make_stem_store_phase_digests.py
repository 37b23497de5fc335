#!/usr/bin/env python3
"""Records SHA-256 digests of what the fused stem's narrow three-term kernel (stem_bf16_v6_kernel, bf16x3) stores on the shapes
of tests/test_stem_store_phases_gpu.py: tests/golden/stem_store_phase_digests.json.  Run it on an MI355X against the library of
the commit BEFORE a change of that kernel's walk order or store forms that must not move a result bit (the library comes from
``STGCN_LIB``, as everywhere); the test imports ``cases()``, ``run()`` and ``digest()`` and compares.

    STGCN_LIB=path/to/libstgcn_hip.so python tools/make_stem_store_phase_digests.py --commit <hash> [--out file.json]

Shapes (V = 22): 600 clips of 24 frames (two full tiles and one of 16 pixels per clip, 1,800 tiles: runs of about seven tiles
that start inside clips), 40 clips of 180 frames (640 tiles, runs of two to three) and 3 clips of 24 frames (nine workgroups of
one tile each), each with (N,C,T,V) and (N,T,V,C) results and with fp32 and bf16 results.  Operands come from the generator of
tests/golden/make_stem_short_tile_digests.py (seeded by the shape); ``run(case, dev, variant)`` draws another input for
``variant`` > 0.  A digest covers the result tensor only.  Every case runs twice here and is written only if both runs agree.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "st-gcn-altformer_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
_spec = importlib.util.spec_from_file_location("make_stem_short_tile_digests",
                                               os.path.join(ROOT, "tests", "golden", "make_stem_short_tile_digests.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

C, S, K = base.C, base.S, base.K
BF16X3, OUT_NTVC = base.BF16X3, base.OUT_NTVC
SHAPES = ((600, 24, 22), (40, 180, 22), (3, 24, 22))        # (N, T, V)
FAMILY = base.FAMILY


def cases():
    """Every case as a dict with a unique ``id``, in a fixed order."""
    return [dict(N=N, T=T, V=V, flags=fl, out_bf16=ob, id=f"{FAMILY}-N{N}-T{T}-V{V}-bf16x3{tag}{'-obf16' if ob else ''}")
            for N, T, V in SHAPES for tag, fl in (("", 0), ("-ontvc", OUT_NTVC)) for ob in (False, True)]


_on_device = {}


def operands(c, dev, variant=0):
    """The shape's operands on the device (moved once per shape); ``variant`` > 0: the same weights with another seeded input."""
    import torch
    key = (c["N"], c["T"], c["V"], str(dev))
    if key not in _on_device:
        _on_device[key] = {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in base.inputs(c).items()}
    p = dict(_on_device[key])
    if variant:
        g = torch.Generator().manual_seed(977 * variant + c["N"] + c["T"])
        p["x"] = torch.randn(c["N"], 3, c["T"], c["V"], generator=g).to(dev)
    return p


def run(c, dev, variant=0):
    """The result tensor of one case, launched on the current stream."""
    from stgcn_amd import _capi
    from stgcn_amd import functional as F
    got = _capi.lib().stgcn_stem_kernel_name(3, C, c["T"], c["V"], K, S, BF16X3 | c["flags"]).decode()
    assert got == FAMILY, f"{c['id']}: served by {got!r}"
    p = operands(c, dev, variant)
    prep = F.stem_prepare(p["Wd"], p["bd"], p["Wdown"], p["bdown"], *p["bn"], *p["dbn"], p["Wt"], p["t_scale"], math=BF16X3)
    out, _ = F.stem_forward(p["x"], p["A"], p["Wa"], p["ba"], p["Wb"], p["bb"], prep, p["t_shift"], C, K, math=BF16X3,
                            out_bf16=c["out_bf16"], channels_last_out=bool(c["flags"] & OUT_NTVC))
    return out


def digest(result):
    import torch
    r = result.detach()
    r = r.contiguous() if r.is_contiguous() else r.permute(0, 2, 3, 1).contiguous()   # (memory order)
    if r.dtype == torch.bfloat16:
        r = r.view(torch.int16)
    return hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library is recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stem_store_phase_digests.json"))
    args = ap.parse_args()
    from stgcn_amd import _capi
    dev = torch.device("cuda:0")
    digests = {}
    for c in cases():
        for variant in (0, 1):                 # (variant 1: the second input of the two-stream case)
            if variant and c["N"] != 600:
                continue
            first, second = digest(run(c, dev, variant)), digest(run(c, dev, variant))
            key = c["id"] + ("-x1" if variant else "")
            if first != second:
                print(f"NOT WRITTEN {key}: two runs of the same library disagree", flush=True)
                continue
            digests[key] = first
            print(key, first[:16], flush=True)
    doc = {"commit": args.commit, "library": os.path.basename(_capi.LIB_PATH),
           "device": f"{torch.cuda.get_device_name(0)} / {torch.cuda.get_device_properties(0).gcnArchName}",
           "rocm": torch.version.hip, "torch": torch.__version__, "digests": digests}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(digests), "cases")


if __name__ == "__main__":
    main()
