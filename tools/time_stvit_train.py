#!/usr/bin/env python3
"""Time TRAINING of the ST-ViT model (fused stem + ``stgcn_amd.vit.ViT`` at 180 frames x 22 joints, ``dropout = 0.1`` as the
reference builds it, in ``.train()``): the layers on the HIP training kernels against the same module on stock torch ops, in
one process, alternating, with device events.

    python tools/time_stvit_train.py [--batches 8,32,128] [--repeats 7] [--warmup 2] [--inner 4] [--sections layer,model]
                                     [--out profiles/stvit_train_times.json]
    python tools/time_stvit_train.py --ends both [--batches 8,32,128,160] [--repeats 9] [--out profiles/stvit_train_ends_times.json]

Prints ONE JSON line.  Per batch (tokens = batch x 100):

* ``layer``: forward + backward of one encoder layer at (batch, 100, 512) with its three dropouts live;
* ``model``: one training step - skeleton clips through the fused stem and the ViT, ``CrossEntropyLoss``, backward, no optimizer.

(The HIP settings lift the ViT's thresholds, so its two ends train on HIP in them as well; ``--ends`` below prices the ends alone.)
Each with the torch path and four HIP settings: training math 'f32' (the default) and 'bf16', each with 128 x 128 tiles and
with the small-tile forms (``small_tiles``: ``VIT_TILE_AUTO`` on the forward and dgrad linears).  A sample is
``max(1, --inner * 8 // batch)`` calls between two events, reported per call.  Every HIP row comes with ``torch_over_hip``
(median over median), ``spread`` (the larger (max - min) / min of the two rows), ``hip_faster_by_more_than_the_spread`` /
``hip_slower_by_more_than_the_spread`` (a difference inside the spread is a tie) and ``peak_mib`` (``max_memory_allocated``
over one call, above what was allocated before it).  ``decision`` applies the project's rule to the 'f32' model rows: the
smallest measured token count from which every measured count is faster than the torch path by more than the spread.

``--ends {hip,torch,both}`` is another run: the layers train on HIP throughout (threshold 0, small-tile forms) and what is
compared is the two ends of the ViT - patch embedding and pooled classifier - on their HIP training branch (``ends_hip``)
against the same commit with env ``STGCN_VIT_TRAIN_ENDS=0`` (``ends_torch``: torch ops under autograd, what ran before
the ends had backwards), the variable flipped between the repeats of one process.  Per batch and training math ('f32', 'bf16'): ``step`` (the
training step of stem + ViT as above), ``embed`` (forward + backward of ``ViT.embed`` alone on the stem's output in the layout
the training stem writes, against rearrange + ``nn.Linear`` + cat + add under autograd) and ``embed_channels_last`` (the same
on a channels-last copy of that output, which the kernels read and write in place), each with median, spread, the two
verdicts and ``peak_mib``.
``decision``: the rule above on the 'f32' step rows, for ``ViT.DEFAULT_HIP_TRAIN_MIN_TOKENS``.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_altformer import peak_bytes                      # noqa: E402
from time_stvit import CONFIG, Model, alternate, summary, versus    # noqa: E402  (the same model, the same way of timing)

SETTINGS = {"hip_f32_128": ("f32", False), "hip_f32_small": ("f32", True), "hip_bf16_128": ("bf16", False),
            "hip_bf16_small": ("bf16", True)}
DROPOUT = 0.1


def configure(vit, setting):
    """``setting``: 'torch' | (training math, small tiles)."""
    import stgcn_amd
    vit.force_torch = setting == "torch"
    for layer in vit.transformer.layers:
        layer.force_torch = setting == "torch"
    if setting == "torch":
        return
    math, small = setting
    stgcn_amd.set_hip_min_tokens(vit, 0)
    stgcn_amd.set_train_math(vit, math)
    for layer in vit.transformer.layers:
        layer.small_tiles = small


def decide(rows, prefix):
    """The rule on the rows {tokens: versus(...)} of the settings that start with ``prefix``: per setting the smallest measured
    count from which every measured count wins by more than the spread (None: the largest measured count does not win)."""
    out = {}
    for name in SETTINGS:
        if not name.startswith(prefix):
            continue
        best = None
        for tokens in sorted(rows, reverse=True):
            if not rows[tokens][name]["hip_faster_by_more_than_the_spread"]:
                break
            best = tokens
        out[name] = best
    return out


def ends_run(args):
    """The ``--ends`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd.vit import VIT_HIP_TRAIN_MIN_TOKENS, ViT
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Model()
    model.v = stgcn_amd.ViT(**CONFIG, dropout=DROPOUT, emb_dropout=0.0)
    model = model.to(dev).train()
    vit = model.v
    with torch.no_grad():
        vit.pos_embedding.normal_(std=0.5)
    which = {"hip": ["ends_hip"], "torch": ["ends_torch"], "both": ["ends_torch", "ends_hip"]}[args.ends]
    res = {"device": torch.cuda.get_device_name(0), "config": dict(CONFIG, dropout=DROPOUT), "repeats": args.repeats,
           "inner": args.inner, "baseline": "ends_torch: the same commit with STGCN_VIT_TRAIN_ENDS=0 (layers on HIP, ends on torch ops)",
           "defaults": {"VIT_HIP_TRAIN_MIN_TOKENS": VIT_HIP_TRAIN_MIN_TOKENS,
                        "ViT.DEFAULT_HIP_TRAIN_MIN_TOKENS": ViT.DEFAULT_HIP_TRAIN_MIN_TOKENS}, "batches": {}}
    ce = torch.nn.CrossEntropyLoss()
    steps = {}

    def env(value):
        os.environ["STGCN_VIT_TRAIN_ENDS"] = value

    for B in [int(b) for b in args.batches.split(",")]:
        per = max(1, args.inner * 8 // B)
        row = {"tokens": B * 100, "calls_per_sample": per}
        x = torch.randn(B, 180, 22, 3, device=dev)
        labels = torch.arange(B, device=dev) % CONFIG["num_classes"]
        with torch.no_grad():
            z = model.tcn0(model.gcn0(x.permute(0, 3, 1, 2)))
        z = z.detach().requires_grad_(True)            # the stem's output in the layout it writes
        row["z_channels_last"] = bool(stgcn_amd.functional._is_channels_last(z))
        zl = z.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)   # as the stem writes it in inference
        dxe = torch.randn(B, 100, CONFIG["dim"], device=dev)

        def model_step():
            model.zero_grad(set_to_none=True)
            ce(model(x), labels).backward()

        def embed_step(zin=z):
            zin.grad = None
            for p in (vit.cls_token, vit.pos_embedding, *vit.to_patch_embedding.parameters()):
                p.grad = None
            vit.embed(zin).backward(dxe)

        for math in ("f32", "bf16"):
            configure(vit, (math, True))
            env("1")
            probe = torch.empty(B, 100, CONFIG["dim"], device=dev, requires_grad=True)
            assert vit.embed_trains_on_hip(z) and vit.head_trains_on_hip(probe) and vit.trains_on_hip(z), (B, math)
            env("0")
            assert not vit.embed_trains_on_hip(z) and not vit.head_trains_on_hip(probe) and vit.trains_on_hip(z), (B, math)
            for section, fn in (("step", model_step), ("embed", embed_step), ("embed_channels_last", lambda: embed_step(zl))):
                cands = {k: ((lambda v="1" if k == "ends_hip" else "0": env(v)), fn) for k in which}
                ts = alternate(cands, args.repeats, args.warmup, per)
                out = versus(ts, base="ends_torch") if len(which) == 2 else {k: summary(v) for k, v in ts.items()}
                for k, (setup, f) in cands.items():
                    setup()
                    out[k]["peak_mib"] = round(peak_bytes(f) / 2 ** 20, 1)
                row.setdefault(section, {})[math] = out
            if len(which) == 2:
                steps.setdefault(math, {})[B * 100] = row["step"][math]["ends_hip"]
        res["batches"][str(B)] = row
        del x, z, zl, dxe
        torch.cuda.empty_cache()
    os.environ.pop("STGCN_VIT_TRAIN_ENDS", None)
    res["decision"] = {}
    for math, rows in steps.items():       # the smallest measured count from which every measured count wins by more than the spread
        best = None
        for tokens in sorted(rows, reverse=True):
            if not rows[tokens]["hip_faster_by_more_than_the_spread"]:
                break
            best = tokens
        res["decision"][math] = best
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--sections", default="layer,model")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ends", choices=("hip", "torch", "both"), default=None)
    args = ap.parse_args()
    if args.ends is not None:
        if args.batches == "8,32,128":
            args.batches = "8,32,128,160"
        args.repeats = max(args.repeats, 9)
        return ends_run(args)
    import stgcn_amd
    from stgcn_amd.altformer import DEFAULT_TRAIN_MATH, HIP_TRAIN_MIN_TOKENS
    from stgcn_amd.vit import VIT_HIP_TRAIN_MIN_TOKENS, VIT_SMALL_TILES
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Model()
    model.v = stgcn_amd.ViT(**CONFIG, dropout=DROPOUT, emb_dropout=0.0)
    model = model.to(dev).train()
    vit = model.v
    with torch.no_grad():
        vit.pos_embedding.normal_(std=0.5)
    layer = vit.transformer.layers[0]
    sections = args.sections.split(",")
    res = {"device": torch.cuda.get_device_name(0), "config": dict(CONFIG, dropout=DROPOUT), "repeats": args.repeats,
           "inner": args.inner, "default_train_math": DEFAULT_TRAIN_MATH,
           "defaults": {"VIT_HIP_TRAIN_MIN_TOKENS": VIT_HIP_TRAIN_MIN_TOKENS, "HIP_TRAIN_MIN_TOKENS": HIP_TRAIN_MIN_TOKENS,
                        "VIT_SMALL_TILES": VIT_SMALL_TILES},
           "batches": {}}
    ce = torch.nn.CrossEntropyLoss()
    by_tokens = {"layer": {}, "model": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        per = max(1, args.inner * 8 // B)
        row = {"tokens": B * 100, "calls_per_sample": per}
        tok = torch.randn(B, 100, 512, device=dev, requires_grad=True)
        dy = torch.randn(B, 100, 512, device=dev)
        x = torch.randn(B, 180, 22, 3, device=dev)
        labels = torch.arange(B, device=dev) % CONFIG["num_classes"]

        def layer_step():
            tok.grad = None
            for p in layer.parameters():
                p.grad = None
            layer(tok).backward(dy)

        def model_step():
            model.zero_grad(set_to_none=True)
            ce(model(x), labels).backward()

        for section, fn in (("layer", layer_step), ("model", model_step)):
            if section not in sections:
                continue
            cands = {"torch": (lambda: configure(vit, "torch"), fn)}
            cands.update({k: (lambda s=s: configure(vit, s), fn) for k, s in SETTINGS.items()})
            for k, s in SETTINGS.items():      # the HIP rows run on HIP, the torch row does not
                configure(vit, s)
                assert layer.trains_on_hip(tok) and all(l.trains_on_hip(tok) for l in vit.transformer.layers), k
            configure(vit, "torch")
            assert not layer.trains_on_hip(tok)
            ts = alternate(cands, args.repeats, args.warmup, per)
            row[section] = versus(ts)
            for k, (setup, f) in cands.items():
                setup()
                row[section][k]["peak_mib"] = round(peak_bytes(f) / 2 ** 20, 1)
            if section == "model":
                for k in row[section]:
                    row[section][k]["clips_per_s"] = round(B / (row[section][k]["median"] * 1e-3), 1)
            by_tokens[section][B * 100] = row[section]
        res["batches"][str(B)] = row
        del tok, dy, x
        torch.cuda.empty_cache()
    res["decision"] = {s: {"f32": decide(by_tokens[s], "hip_f32"), "bf16": decide(by_tokens[s], "hip_bf16")}
                       for s in by_tokens if by_tokens[s]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
