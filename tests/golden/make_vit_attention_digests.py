"""Records SHA-256 digests of what the heads' attention entry points compute on their own, case by case:
tests/golden/vit_attention_digests.json.  Run it on an MI355X against the library of the commit BEFORE a change that must not
move a result bit of an attention kernel (the library comes from ``STGCN_LIB``, as everywhere);
tests/test_vit_attention_digests_gpu.py imports ``cases()`` and ``run()`` and compares.

    STGCN_LIB=path/to/libstgcn_hip.so python tests/golden/make_vit_attention_digests.py --commit <hash> [--out file.json]

The block digests (make_vit_block_digests.py) reach the attention kernels at L = 22, 256 and 300 with head_dim 32 (64 at
L = 22 only) and never with VIT_TRAIN_ATTN_BF16.  Here every resident kernel runs at every NT = ceil(L / 32) = 1 .. 8 with a
full and a partial last tile, on both sides of the packing switches (four pairs per workgroup up to L = 32, two up to 64, one
above) and of the bf16 backward's SPLIT instantiation (head_dim 64, L > 224); the streaming kernels run at one key, around one
and two LDS stages of 64 keys, and past the resident lengths.  B = 3 sequences of 3 heads are 9 pairs: a short last workgroup
at four and at two pairs per workgroup.

A digest covers the result tensor only (out, or dqkv).  Every case runs twice here and is written only if both runs agree.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "st-gcn-altformer_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

B, HEADS = 3, 3
HEAD_DIMS = (32, 64)
RESIDENT_L = (1, 32, 33, 64, 65, 97, 129, 161, 193, 224, 225, 256)
STREAM_L = (1, 63, 64, 65, 128, 129, 300)
FORWARD = ("vit_attention", "vit_attention_bf16", "vit_attention_train_bf16", "vit_attention_stream")
BACKWARD = ("vit_attention_backward", "vit_attention_backward_bf16", "vit_attention_backward_stream")
RESIDENT = ("vit_attention", "vit_attention_bf16", "vit_attention_train_bf16", "vit_attention_backward", "vit_attention_backward_bf16")
STREAM = ("vit_attention_stream", "vit_attention_backward_stream")


def cases():
    """Every case as a dict with a unique ``id``, in a fixed order."""
    out = []
    for entries, lengths in ((RESIDENT, RESIDENT_L), (STREAM, STREAM_L)):
        for hd in HEAD_DIMS:
            for L in lengths:
                for entry in entries:
                    out.append(dict(entry=entry, L=L, hd=hd, id=f"{entry}-L{L}-hd{hd}"))
    assert len({c["id"] for c in out}) == len(out)
    return out


_inputs = {}


def inputs(L, hd):
    """qkv (B, L, 3 * HEADS * hd), out and dout (B, L, HEADS * hd) of a shape, drawn once on the CPU from a generator seeded by
    the shape and shared (unchanged) by every case of that shape.  q and k are multiplied by 4: a peaked soft-max, as
    tests/altformer_ref.py.  ``out`` is drawn, not computed: the backward reads it as an input like the two others."""
    if (L, hd) not in _inputs:
        g = torch.Generator().manual_seed(1000 * L + hd)
        D = HEADS * hd
        qkv = torch.randn(B, L, 3 * D, generator=g)
        qkv[..., :2 * D] *= 4.0
        _inputs[(L, hd)] = (qkv, torch.randn(B, L, D, generator=g), torch.randn(B, L, D, generator=g))
    return _inputs[(L, hd)]


def run(case, dev):
    """The result tensor of one case."""
    from stgcn_amd import functional as F
    qkv, out, dout = (t.to(dev) for t in inputs(case["L"], case["hd"]))
    entry = getattr(F, case["entry"])
    if case["entry"] == "vit_attention_bf16":
        return entry(qkv.to(torch.bfloat16), HEADS).view(torch.int16)
    if case["entry"] in BACKWARD:
        return entry(qkv, out, dout, HEADS)
    return entry(qkv, HEADS)


def digest(result):
    return hashlib.sha256(result.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library is recorded")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "vit_attention_digests.json"))
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
    doc = {"commit": args.commit, "library": os.path.basename(_capi.LIB_PATH), "device": torch.cuda.get_device_name(0),
           "rocm": torch.version.hip, "torch": torch.__version__, "digests": digests}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(args.out, len(digests), "of", len(cases()), "cases")


if __name__ == "__main__":
    main()
