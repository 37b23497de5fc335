#!/usr/bin/env python3
"""Time the ST-ViT model (fused stem + ``stgcn_amd.vit.ViT`` at 180 frames x 22 joints): the HIP path of the head against the
same module forced onto stock torch ops, in one process, alternating, with device events.

    python tools/time_stvit.py [--batches 1,8,32,128] [--repeats 7] [--warmup 2] [--inner 20] [--sections embed,layer,model]
                               [--out profiles/stvit_times.json]

Prints ONE JSON line.  Per batch:

* ``embed``: the patch embedding alone on a fixed stem output - ``stgcn_vit_patch_embed`` ('f32' and 'bf16x3', on the
  contiguous and on the channels-last stem output) against torch's rearrange + ``nn.Linear`` + cat + add;
* ``layer``: one encoder layer at (batch, 100, 512) - HIP in 'mixed' and 'bf16', each with 128 x 128 tiles and with the
  small-tile forms (``set_low_latency``), against the layer's torch ops;
* ``model``: skeleton clips to logits, stem + head - the head on HIP in the same four settings (the stem writing channels-last,
  read in place) against the head on torch ops behind the same stem.

A sample is ``max(1, --inner // batch)`` calls between two events, reported per call.  Every HIP row comes with
``torch_over_hip`` (median over median), ``spread`` (the larger (max - min) / min of the two rows) and
``hip_faster_by_more_than_the_spread`` / ``hip_slower_by_more_than_the_spread``: a difference inside the spread is a tie.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))

CONFIG = dict(time_len=180, joint=22, p1=20, p2=2, num_classes=14, dim=512, depth=6, heads=8, mlp_dim=512)


def events(fn, per):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(per):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / per


def alternate(fns, repeats, warmup, per):
    """{name: [ms per call, ...]} from {name: (setup, fn)}: the candidates run in turn, ``warmup`` untimed rounds first;
    ``setup`` (the module switches of the candidate) runs before the first event, outside the timed region."""
    for _ in range(warmup):
        for setup, fn in fns.values():
            setup()
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (setup, fn) in fns.items():
            setup()
            torch.cuda.synchronize()
            out[k].append(events(fn, per))
    return out


def summary(ts):
    return {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4), "max": round(max(ts), 4),
            "spread": round((max(ts) - min(ts)) / min(ts), 4)}


def faster_by_more_than_the_spread(fast, slow):
    return statistics.median(fast) * (1 + max(summary(fast)["spread"], summary(slow)["spread"])) < statistics.median(slow)


def versus(ts, base="torch"):
    rows = {base: summary(ts[base])}
    for k, v in ts.items():
        if k == base:
            continue
        rows[k] = dict(summary(v), torch_over_hip=round(statistics.median(ts[base]) / statistics.median(v), 3),
                       spread=round(max(summary(v)["spread"], summary(ts[base])["spread"]), 4),
                       hip_faster_by_more_than_the_spread=faster_by_more_than_the_spread(v, ts[base]),
                       hip_slower_by_more_than_the_spread=faster_by_more_than_the_spread(ts[base], v))
    return rows


class Model(torch.nn.Module):
    """What the reference's ST_GCN_Trans runs with ``all_layers=False``: gcn0 -> tcn0 -> ViT."""

    def __init__(self):
        super().__init__()
        import stgcn_amd
        from stgcn_amd.graphs import SHREGraph
        A = torch.from_numpy(SHREGraph("spatial").A.astype(np.float32))
        self.gcn0 = stgcn_amd.unit_agcn(3, 128, A)
        self.tcn0 = stgcn_amd.Unit2D(128, 128, kernel_size=9)
        self.v = stgcn_amd.ViT(**CONFIG)
        stgcn_amd.enable_stem_fusion(self.gcn0, self.tcn0)

    def forward(self, x):
        return self.v(self.tcn0(self.gcn0(x.permute(0, 3, 1, 2))))


def configure(vit, setting):
    """``setting``: 'torch' | (math, tiles) with tiles '128' | 'small'."""
    import stgcn_amd
    vit.force_torch = setting == "torch"
    for layer in vit.transformer.layers:
        layer.force_torch = setting == "torch"
    if setting == "torch":
        return
    math, tiles = setting
    stgcn_amd.set_low_latency(vit, enabled=tiles == "small", min_tokens=0)
    stgcn_amd.set_hip_min_tokens(vit, 0)
    for sub in [vit] + list(vit.transformer.layers):    # (disabling restores the ViT's default, which is the small forms)
        sub.small_tiles = tiles == "small"
    stgcn_amd.set_head_math(vit, math)


SETTINGS = {"hip_mixed_128": ("mixed", "128"), "hip_mixed_small": ("mixed", "small"), "hip_bf16_128": ("bf16", "128"),
            "hip_bf16_small": ("bf16", "small")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sections", default="embed,layer,model")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Model().to(dev).eval()
    vit = model.v
    with torch.no_grad():
        vit.pos_embedding.normal_(std=0.5)
    res = {"device": torch.cuda.get_device_name(0), "config": CONFIG, "repeats": args.repeats, "inner": args.inner, "batches": {}}
    pat, lin = vit.to_patch_embedding
    for B in [int(b) for b in args.batches.split(",")]:
        per = max(1, args.inner // B)
        row = {"tokens": B * 100, "calls_per_sample": per,
               "embed_cut": F.vit_patch_embed_cut(B, 128, 180, 22, 20, 2, 512, HEAD_MATH["mixed"], True)}
        x = torch.randn(B, 180, 22, 3, device=dev)
        with torch.no_grad():
            stgcn_amd.set_output_layout(model, "contiguous")
            z = model.tcn0(model.gcn0(x.permute(0, 3, 1, 2))).clone()
            zl = z.contiguous(memory_format=torch.channels_last)
            tok = torch.randn(B, 100, 512, device=dev)
            layer = vit.transformer.layers[0]

            def embed_hip(math, inp):
                return (lambda: None, lambda: F.vit_patch_embed(inp, lin.weight, lin.bias, vit.cls_token, vit.pos_embedding[0, :100],
                                                                pat.p1, pat.p2, HEAD_MATH[math]))
            sections = args.sections.split(",")
            ts = alternate({"torch": (lambda: configure(vit, "torch"), lambda: vit.embed(z)), "hip_f32_nchw": embed_hip("f32", z), "hip_f32_ntvc": embed_hip("f32", zl),
                            "hip_bf16x3_nchw": embed_hip("bf16x3", z), "hip_bf16x3_ntvc": embed_hip("bf16x3", zl)},
                           args.repeats if "embed" in sections else 0, args.warmup, per)
            if "embed" in sections:
                row["embed"] = versus(ts)

            def run_layer(setting):
                return (lambda: configure(vit, setting), lambda: layer(tok))
            ts = alternate(dict({"torch": run_layer("torch")}, **{k: run_layer(s) for k, s in SETTINGS.items()}),
                           args.repeats if "layer" in sections else 0, args.warmup, per)
            if "layer" in sections:
                row["layer"] = versus(ts)

            stgcn_amd.set_output_layout(model, "channels_last")

            def run_model(setting):
                return (lambda: configure(vit, setting), lambda: model(x))
            ts = alternate(dict({"torch": run_model("torch")}, **{k: run_model(s) for k, s in SETTINGS.items()}),
                           args.repeats if "model" in sections else 0, args.warmup, per)
            configure(vit, SETTINGS["hip_mixed_128"])
            assert vit.uses_hip(zl), "the HIP rows did not run on HIP"
            if "model" in sections:
                row["model"] = versus(ts)
                for k in row["model"]:
                    row["model"][k]["clips_per_s"] = round(B / (row["model"][k]["median"] * 1e-3), 1)
        res["batches"][str(B)] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
