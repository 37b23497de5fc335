#!/usr/bin/env python3
"""Time training of the AltFormer heads: forward + backward of one transformer block at every stage of both heads, and one
training step (forward, CrossEntropyLoss, backward, no optimizer) of the whole ST / TS models in ``.train()`` with stochastic
depth on - the HIP training path against the torch-op path of the same module, in one process, alternating, device events.

    python tools/time_altformer_train.py [--batch 32] [--repeats 7] [--warmup 2] [--out profiles/altformer_train_times.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_altformer_train.py --stages-only --repeats 5

    python tools/time_altformer_train.py --frames 500 [--batch 32] [--out profiles/altformer_long_train_times.json]

``--frames T`` (T > 256) times training on long clips instead, where the blocks train on HIP only after
``set_long_training`` (the streaming attention forward and backward): forward + backward of one block at the ST temporal stage
(``batch`` sequences of T, D = 512) and the TS temporal stage (``batch`` x 22 sequences of T, D = 256), and one training step
of the whole ST and TS models at ``num_frame = T``, each alternating ``set_long_training`` on and off in one process.  Off is
the torch-op path such blocks take by default, with ``torch.cuda.max_memory_allocated`` of each.

    python tools/time_altformer_train.py --train-math bf16 [--batch 32] [--out profiles/altformer_train_bf16_times.json]

``--train-math bf16`` times the opt-in bf16 training arithmetic (``set_train_math(model, 'bf16')``) against the two it would
replace, all three on the HIP training path, alternating in one process: forward + backward of one block at every stage and one
training step of the whole ST and TS models in 'f32' (the default), 'bf16x3' and 'bf16', with medians, spread and
``torch.cuda.max_memory_allocated``; and, per launch, the weight gradient (fp32 and bf16 kernel) and the dgrad (f32, bf16x3,
bf16 form of the linear kernel) of the four linears of every stage through ``functional.vit_linear_backward``.
``bf16_faster``: the bf16 median is below BOTH other medians by more than the largest of the three spreads.

    python tools/time_altformer_train.py --train-attention bf16 [--batch 32] [--out profiles/altformer_train_bf16_attn_times.json]

``--train-attention bf16`` times the opt-in bf16 training attention (``set_train_attention_math(model, 'bf16')``) on top of the
bf16 training arithmetic: 'bf16' training math without the switch (``base``: the code that runs without this mode, the baseline)
and with it (``attn``), alternating in one process - forward + backward of one block at every stage, the attention forward and
backward of every stage per launch (fp32 kernel against bf16 kernel), and one training step of the whole ST and TS models.
``attn_faster`` / ``attn_slower``: the medians differ by more than the larger of the two spreads.  ``base_vs_recorded``
compares the baseline's stage medians with profiles/altformer_train_bf16_times.json where that file is there.

    python tools/time_altformer_train.py --small [--batch 32] [--joints 22] [--out FILE]

``--small`` times the small training calls (``set_low_latency_training(model, train_min_tokens=0)``: tile forms picked by
call size, both forms of the weight-gradient kernels) against the two paths they would replace, alternating in one process:
``torch`` (the torch-op path), ``hip`` (the HIP path with the switch off: 128 x 128 forms everywhere, what ran before there was
a switch) and ``small`` (the switch on).  Forward + backward of one block at every stage, with the form and split count of the
stage's four weight gradients, and one training step of the whole ST and TS models with every block on the path under test, and on the two paths a user gets
without lifting a threshold: ``default`` (the switch off, ``HIP_TRAIN_MIN_TOKENS``: smaller stages on torch ops) and
``small_default`` (``set_low_latency_training(model)``: the switch on from ``LOW_LATENCY_TRAIN_MIN_TOKENS``).
``--joints 46`` runs the whole models on the LMDHG shape (180 x 46).  ``small_faster_than_torch``, ``small_faster_than_hip`` /
``small_slower_than_hip``: the medians differ by more than the larger of the two spreads.  ``low_latency_train_min_tokens``:
the smallest stage from which every measured stage has ``small_faster_than_torch`` (what ``LOW_LATENCY_TRAIN_MIN_TOKENS``
follows), null if the largest stage does not have it.

Prints ONE JSON line.  Per stage: ms of forward + backward (min, median, max, ``spread`` = (max - min) / min) of the torch
path and of the HIP path in each arithmetic ('f32', 'mixed', 'bf16x3'), the speed-up of the default arithmetic, and
``hip_faster`` = the HIP median is below the torch median by more than the larger of the two spreads (the rule
``HIP_TRAIN_MIN_TOKENS`` follows).  Whole models: ms per step and clips/s for both paths.
"""
import argparse
import json
import os
import statistics
import sys
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_altformer import STAGES, alternate, faster_by_more_than_the_spread, peak_bytes, summary   # noqa: E402  (same stages, same way of timing)

MODES = ("f32", "mixed", "bf16x3")


def long_clips(args):
    """The ``--frames`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd.altformer import DEFAULT_TRAIN_MATH, Block, set_long_training
    T, dev = args.frames, torch.device("cuda:0")
    assert T > 256, "--frames is for sequences the resident attention kernels do not take"
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    res = {"frames": T, "batch": args.batch, "repeats": args.repeats, "default_train_math": DEFAULT_TRAIN_MATH,
           "device": torch.cuda.get_device_name(0), "stages": {}, "models": {}}

    def entry(ts, mem, **more):
        med = {k: statistics.median(v) for k, v in ts.items()}
        return {**more, "hip_ms": summary(ts["hip"]), "torch_ms": summary(ts["torch"]),
                "speedup_median": round(med["torch"] / med["hip"], 3),
                "hip_faster": faster_by_more_than_the_spread(ts["hip"], ts["torch"]),
                "peak_mib_hip": round(mem["hip"] / 2 ** 20, 1), "peak_mib_torch": round(mem["torch"] / 2 ** 20, 1)}

    for name, (per_clip, D) in {f"ST temporal {T}": (1, 512), f"TS temporal (22 x {T})": (22, 256)}.items():
        B = args.batch * per_clip
        torch.manual_seed(0)
        blk = Block(D, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.1, norm_layer=norm).to(dev).train()
        x = torch.randn(B, T, D, device=dev, requires_grad=True)
        dy = torch.randn(B, T, D, device=dev)
        chooses = "hip" if blk.trains_on_hip(x) else "torch"
        blk.hip_train_min_tokens = 0

        def run(long):
            set_long_training(blk, long)
            assert blk.trains_on_hip(x) == long
            x.grad = None
            for p in blk.parameters():
                p.grad = None
            blk(x).backward(dy)
        ts = alternate({"torch": partial(run, False), "hip": partial(run, True)}, args.repeats, args.warmup)
        mem = {k: peak_bytes(partial(run, k == "hip")) for k in ("torch", "hip")}
        res["stages"][name] = entry(ts, mem, B=B, L=T, D=D, tokens=B * T, module_chooses=chooses)
        del blk, x, dy
        torch.cuda.empty_cache()
    for style in () if args.stages_only else ("ST", "TS"):
        torch.manual_seed(1)
        model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=T, num_joints=22, style=style,
                                           graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).train()
        clips = torch.randn(args.batch, T, 22, 3, device=dev)
        labels = torch.arange(args.batch, device=dev) % 14
        ce = torch.nn.CrossEntropyLoss()
        blocks = [b for b in model.modules() if isinstance(b, Block)]

        def step(long):
            set_long_training(model, long)
            model.zero_grad(set_to_none=True)
            ce(model(clips), labels).backward()
        on_hip = {}
        for long in (False, True):            # which blocks train on HIP under the default token threshold, off and on
            calls = []
            hooks = [b.register_forward_pre_hook(lambda mod, a: calls.append(bool(mod.trains_on_hip(a[0])))) for b in blocks]
            step(long)
            for hk in hooks:
                hk.remove()
            on_hip["on" if long else "off"] = sum(calls)
        ts = alternate({"torch": partial(step, False), "hip": partial(step, True)}, args.repeats, args.warmup)
        mem = {k: peak_bytes(partial(step, k == "hip")) for k in ("torch", "hip")}
        med = {k: statistics.median(v) for k, v in ts.items()}
        res["models"][style] = entry(ts, mem, blocks=len(blocks), blocks_on_hip=on_hip,
                                     clips_per_s_hip=round(args.batch / (med["hip"] * 1e-3), 1),
                                     clips_per_s_torch=round(args.batch / (med["torch"] * 1e-3), 1))
        del model, clips
        torch.cuda.empty_cache()
    return res


TRAIN_MATH_MODES = ("f32", "bf16x3", "bf16")


def train_math_bf16(args):
    """The ``--train-math bf16`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import DEFAULT_TRAIN_MATH, HEAD_TRAIN_MATH, Block, set_train_math
    dev = torch.device("cuda:0")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    res = {"train_math": "bf16", "batch": args.batch, "repeats": args.repeats, "default_train_math": DEFAULT_TRAIN_MATH,
           "bf16_flags": HEAD_TRAIN_MATH["bf16"], "device": torch.cuda.get_device_name(0), "stages": {}, "launches": {}, "models": {}}

    def entry(ts, mem, **more):
        med = {k: statistics.median(v) for k, v in ts.items()}
        margin = max(summary(v)["spread"] for v in ts.values())
        return {**more, **{f"{m}_ms": summary(ts[m]) for m in TRAIN_MATH_MODES},
                **{f"peak_mib_{m}": round(mem[m] / 2 ** 20, 1) for m in TRAIN_MATH_MODES},
                "bf16_vs_f32": round(med["f32"] / med["bf16"], 3), "bf16_vs_bf16x3": round(med["bf16x3"] / med["bf16"], 3),
                "bf16_faster": med["bf16"] * (1 + margin) < min(med["f32"], med["bf16x3"])}

    for name, (per_clip, L, D) in STAGES.items():
        B = args.batch * per_clip
        torch.manual_seed(0)
        blk = Block(D, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.1, norm_layer=norm).to(dev).train()
        blk.hip_train_min_tokens = 0
        x = torch.randn(B, L, D, device=dev, requires_grad=True)
        dy = torch.randn(B, L, D, device=dev)

        def run(mode):
            set_train_math(blk, mode)
            assert blk.trains_on_hip(x)
            x.grad = None
            for p in blk.parameters():
                p.grad = None
            blk(x).backward(dy)
        ts = alternate({m: partial(run, m) for m in TRAIN_MATH_MODES}, args.repeats, args.warmup)
        mem = {m: peak_bytes(partial(run, m)) for m in TRAIN_MATH_MODES}
        res["stages"][name] = entry(ts, mem, B=B, L=L, D=D, tokens=B * L)
        del blk, x, dy
        # the launches on their own: (M, K, Nout) of qkv, proj, fc1, fc2
        M, per = B * L, {}
        for lin, (K, Nout) in {"qkv": (D, 3 * D), "proj": (D, D), "fc1": (D, 2 * D), "fc2": (2 * D, D)}.items():
            g = torch.Generator(device=dev).manual_seed(K + Nout)
            gy = torch.randn(M, Nout, device=dev, generator=g)
            a = torch.randn(M, K, device=dev, generator=g)
            W = torch.randn(Nout, K, device=dev, generator=g) / K ** 0.5
            h = torch.randn(M, K, device=dev, generator=g) if lin == "fc2" else None      # fc2's dgrad carries GELU'
            forms = {"f32": F.MATH_F32, "bf16x3": F.MATH_BF16X3, "bf16": F.MATH_BF16X3 | F.VIT_TRAIN_BF16}
            wg = alternate({m: partial(F.vit_linear_backward, gy, a, W, need_dx=False, math=forms[m]) for m in ("f32", "bf16")},
                           args.repeats, args.warmup)
            dg = alternate({m: partial(F.vit_linear_backward, gy, a, W, h_pre=h, need_dw=False, math=forms[m]) for m in forms},
                           args.repeats, args.warmup)
            per[lin] = {"M": M, "K": K, "Nout": Nout, **{f"wgrad_{m}_ms": summary(v) for m, v in wg.items()},
                        **{f"dgrad_{m}_ms": summary(v) for m, v in dg.items()},
                        "wgrad_bf16_vs_f32": round(statistics.median(wg["f32"]) / statistics.median(wg["bf16"]), 3),
                        "dgrad_bf16_vs_f32": round(statistics.median(dg["f32"]) / statistics.median(dg["bf16"]), 3)}
            del gy, a, W, h
        res["launches"][name] = per
        torch.cuda.empty_cache()
    for style in () if args.stages_only else ("ST", "TS"):
        torch.manual_seed(1)
        model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style,
                                           graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).train()
        clips = torch.randn(args.batch, 180, 22, 3, device=dev)
        labels = torch.arange(args.batch, device=dev) % 14
        ce = torch.nn.CrossEntropyLoss()

        def step(mode):
            set_train_math(model, mode)
            model.zero_grad(set_to_none=True)
            ce(model(clips), labels).backward()
        ts = alternate({m: partial(step, m) for m in TRAIN_MATH_MODES}, args.repeats, args.warmup)
        mem = {m: peak_bytes(partial(step, m)) for m in TRAIN_MATH_MODES}
        res["models"][style] = entry(ts, mem, clips_per_s={m: round(args.batch / (statistics.median(ts[m]) * 1e-3), 1)
                                                           for m in TRAIN_MATH_MODES})
        del model, clips
        torch.cuda.empty_cache()
    return res


def train_attention_bf16(args):
    """The ``--train-attention bf16`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_TRAIN_MATH, Block, set_train_attention_math, set_train_math
    dev = torch.device("cuda:0")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    res = {"train_attention": "bf16", "train_math": "bf16", "batch": args.batch, "repeats": args.repeats,
           "base_flags": HEAD_TRAIN_MATH["bf16"], "attn_flags": HEAD_TRAIN_MATH["bf16"] | F.VIT_TRAIN_ATTN_BF16,
           "device": torch.cuda.get_device_name(0), "stages": {}, "launches": {}, "models": {}}
    recorded = {}
    path = os.path.join(ROOT, "profiles", "altformer_train_bf16_times.json")
    if os.path.exists(path):
        with open(path) as f:
            recorded = json.load(f).get("stages", {})

    def entry(ts, **more):
        med = {k: statistics.median(v) for k, v in ts.items()}
        return {**more, "base_ms": summary(ts["base"]), "attn_ms": summary(ts["attn"]),
                "speedup_median": round(med["base"] / med["attn"], 3),
                "attn_faster": faster_by_more_than_the_spread(ts["attn"], ts["base"]),
                "attn_slower": faster_by_more_than_the_spread(ts["base"], ts["attn"])}

    for name, (per_clip, L, D) in STAGES.items():
        B = args.batch * per_clip
        torch.manual_seed(0)
        blk = Block(D, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.1, norm_layer=norm).to(dev).train()
        blk.hip_train_min_tokens = 0
        set_train_math(blk, "bf16")
        x = torch.randn(B, L, D, device=dev, requires_grad=True)
        dy = torch.randn(B, L, D, device=dev)

        def run(mode):
            set_train_attention_math(blk, mode)
            assert blk.trains_on_hip(x)
            x.grad = None
            for p in blk.parameters():
                p.grad = None
            blk(x).backward(dy)
        ts = alternate({"base": partial(run, "f32"), "attn": partial(run, "bf16")}, args.repeats, args.warmup)
        more = {}
        if name in recorded and recorded[name].get("B") == B:
            more["base_vs_recorded"] = round(statistics.median(ts["base"]) / recorded[name]["bf16_ms"]["median"], 3)
        res["stages"][name] = entry(ts, B=B, L=L, D=D, tokens=B * L, **more)
        del blk, x, dy
        # the two attention launches on their own
        heads = 8
        g = torch.Generator(device=dev).manual_seed(L + D)
        qkv = torch.randn(B, L, 3 * D, device=dev, generator=g)
        dout = torch.randn(B, L, D, device=dev, generator=g)
        out = F.vit_attention(qkv, heads)
        fw = alternate({"base": partial(F.vit_attention, qkv, heads), "attn": partial(F.vit_attention_train_bf16, qkv, heads)},
                       args.repeats, args.warmup)
        bw = alternate({"base": partial(F.vit_attention_backward, qkv, out, dout, heads),
                        "attn": partial(F.vit_attention_backward_bf16, qkv, out, dout, heads)}, args.repeats, args.warmup)
        res["launches"][name] = {"pairs": B * heads, "L": L, "head_dim": D // heads, "forward": entry(fw), "backward": entry(bw)}
        del qkv, dout, out
        torch.cuda.empty_cache()
    for style in () if args.stages_only else ("ST", "TS"):
        torch.manual_seed(1)
        model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style,
                                           graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).train()
        set_train_math(model, "bf16")
        clips = torch.randn(args.batch, 180, 22, 3, device=dev)
        labels = torch.arange(args.batch, device=dev) % 14
        ce = torch.nn.CrossEntropyLoss()

        def step(mode):
            set_train_attention_math(model, mode)
            model.zero_grad(set_to_none=True)
            ce(model(clips), labels).backward()
        ts = alternate({"base": partial(step, "f32"), "attn": partial(step, "bf16")}, args.repeats, args.warmup)
        res["models"][style] = entry(ts, clips_per_s={m: round(args.batch / (statistics.median(ts[m]) * 1e-3), 1) for m in ts})
        del model, clips
        torch.cuda.empty_cache()
    return res


def small_calls(args):
    """The ``--small`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import DEFAULT_TRAIN_MATH, HIP_TRAIN_MIN_TOKENS, LOW_LATENCY_TRAIN_MIN_TOKENS, Block, set_low_latency_training
    dev = torch.device("cuda:0")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    res = {"small": True, "batch": args.batch, "joints": args.joints, "repeats": args.repeats, "default_train_math": DEFAULT_TRAIN_MATH,
           "hip_train_min_tokens": HIP_TRAIN_MIN_TOKENS, "low_latency_train_min_tokens_constant": LOW_LATENCY_TRAIN_MIN_TOKENS,
           "device": torch.cuda.get_device_name(0), "stages": {}, "models": {}}
    PATHS = ("torch", "hip", "small")

    def switch(module, path):
        for b in module.modules():
            if isinstance(b, Block):
                b.force_torch = path == "torch"
        set_low_latency_training(module, False)
        if path in ("small", "small_default"):
            set_low_latency_training(module, train_min_tokens=0 if path == "small" else None)
        else:
            for b in module.modules():
                if isinstance(b, Block):            # 'hip': every block on the 128 x 128 kernels, however few tokens
                    b.hip_train_min_tokens = HIP_TRAIN_MIN_TOKENS if path == "default" else 0

    def entry(ts, **more):
        med = {k: statistics.median(v) for k, v in ts.items()}
        return {**more, **{f"{k}_ms": summary(v) for k, v in ts.items()},
                "small_vs_torch": round(med["torch"] / med["small"], 3), "small_vs_hip": round(med["hip"] / med["small"], 3),
                "hip_vs_torch": round(med["torch"] / med["hip"], 3),
                "small_faster_than_torch": faster_by_more_than_the_spread(ts["small"], ts["torch"]),
                "small_faster_than_hip": faster_by_more_than_the_spread(ts["small"], ts["hip"]),
                "small_slower_than_hip": faster_by_more_than_the_spread(ts["hip"], ts["small"])}

    for name, (per_clip, L, D) in STAGES.items():
        B = args.batch * per_clip
        torch.manual_seed(0)
        blk = Block(D, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.1, norm_layer=norm).to(dev).train()
        x = torch.randn(B, L, D, device=dev, requires_grad=True)
        dy = torch.randn(B, L, D, device=dev)

        def run(path):
            switch(blk, path)
            assert blk.trains_on_hip(x) == (path != "torch") and blk.small_tiles_train == (path == "small")
            x.grad = None
            for p in blk.parameters():
                p.grad = None
            blk(x).backward(dy)
        ts = alternate({p: partial(run, p) for p in PATHS}, args.repeats, args.warmup)
        M = min(B * L, (32768 // L) * L)             # the rows of one slab of whole sequences
        plans = {lin: F.vit_wgrad_plan(M, K, Nout, F.VIT_WGRAD_SMALL)
                 for lin, (K, Nout) in {"qkv": (D, 3 * D), "proj": (D, D), "fc1": (D, 2 * D), "fc2": (2 * D, D)}.items()}
        res["stages"][name] = entry(ts, B=B, L=L, D=D, tokens=B * L, wgrad_tile_splits_direct=plans)
        del blk, x, dy
        torch.cuda.empty_cache()
    order = sorted(res["stages"].values(), key=lambda e: e["tokens"])
    cut = None
    for e in reversed(order):
        if not e["small_faster_than_torch"]:
            break
        cut = e["tokens"]
    res["low_latency_train_min_tokens"] = cut
    graph = {22: "graph.SHRE", 46: "graph.LMDHG"}[args.joints]
    for style in () if args.stages_only else ("ST", "TS"):
        torch.manual_seed(1)
        model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=args.joints, style=style,
                                           graph=graph, graph_args={"labeling_mode": "spatial"}).to(dev).train()
        clips = torch.randn(args.batch, 180, args.joints, 3, device=dev)
        labels = torch.arange(args.batch, device=dev) % 14
        ce = torch.nn.CrossEntropyLoss()

        def step(path):
            switch(model, path)
            model.zero_grad(set_to_none=True)
            ce(model(clips), labels).backward()
        ts = alternate({p: partial(step, p) for p in PATHS + ("default", "small_default")}, args.repeats, args.warmup)
        res["models"][style] = entry(ts, clips_per_s={p: round(args.batch / (statistics.median(ts[p]) * 1e-3), 1) for p in ts},
                                     small_default_vs_default=round(statistics.median(ts["default"]) / statistics.median(ts["small_default"]), 3),
                                     small_default_faster_than_default=faster_by_more_than_the_spread(ts["small_default"], ts["default"]),
                                     small_vs_default=round(statistics.median(ts["default"]) / statistics.median(ts["small"]), 3),
                                     small_faster_than_default=faster_by_more_than_the_spread(ts["small"], ts["default"]))
        del model, clips
        torch.cuda.empty_cache()
    return res


def emit(res, out):
    line = json.dumps(res)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stages-only", action="store_true")
    ap.add_argument("--frames", type=int, default=None, help="time training at this many frames (> 256) instead")
    ap.add_argument("--train-math", choices=["bf16"], default=None,
                    help="time this opt-in training arithmetic against 'f32' and 'bf16x3' instead")
    ap.add_argument("--train-attention", choices=["bf16"], default=None,
                    help="time the opt-in bf16 training attention on top of 'bf16' training math, against that math alone")
    ap.add_argument("--small", action="store_true",
                    help="time the small training calls (set_low_latency_training) against the torch path and the 128-form HIP path")
    ap.add_argument("--joints", type=int, choices=[22, 46], default=22, help="--small: joints of the whole models (46: LMDHG)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    if args.small:
        return emit(small_calls(args), args.out)
    if args.train_attention is not None:
        return emit(train_attention_bf16(args), args.out)
    if args.train_math is not None:
        return emit(train_math_bf16(args), args.out)
    if args.frames is not None:
        return emit(long_clips(args), args.out)
    import stgcn_amd
    from stgcn_amd.altformer import DEFAULT_TRAIN_MATH, HIP_TRAIN_MIN_TOKENS, Block, set_head_math, set_hip_min_tokens
    dev = torch.device("cuda:0")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    res = {"batch": args.batch, "repeats": args.repeats, "default_train_math": DEFAULT_TRAIN_MATH,
           "hip_train_min_tokens": HIP_TRAIN_MIN_TOKENS, "device": torch.cuda.get_device_name(0), "stages": {}, "models": {}}
    for name, (per_clip, L, D) in STAGES.items():
        B = args.batch * per_clip
        torch.manual_seed(0)
        blk = Block(D, 8, mlp_ratio=2., qkv_bias=True, drop_path=0.1, norm_layer=norm).to(dev).train()
        x = torch.randn(B, L, D, device=dev, requires_grad=True)
        dy = torch.randn(B, L, D, device=dev)
        chooses = "hip" if blk.trains_on_hip(x) else "torch"
        blk.hip_train_min_tokens = 0

        def run(mode):
            blk.force_torch = mode == "torch"
            if mode != "torch":
                set_head_math(blk, mode)
                assert blk.trains_on_hip(x)
            x.grad = None
            for p in blk.parameters():
                p.grad = None
            blk(x).backward(dy)
        ts = alternate({m: partial(run, m) for m in ("torch",) + MODES}, args.repeats, args.warmup)
        tor, hip = ts["torch"], ts[DEFAULT_TRAIN_MATH]
        margin = max(summary(tor)["spread"], summary(hip)["spread"])
        res["stages"][name] = {
            "B": B, "L": L, "D": D, "tokens": B * L, "module_chooses": chooses, "torch_ms": summary(tor),
            **{f"hip_{m}_ms": summary(ts[m]) for m in MODES},
            "speedup_median": round(statistics.median(tor) / statistics.median(hip), 3),
            "hip_faster": statistics.median(hip) * (1 + margin) < statistics.median(tor)}
        del blk, x, dy
        torch.cuda.empty_cache()
    for style in () if args.stages_only else ("ST", "TS"):
        torch.manual_seed(1)
        model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style,
                                           graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).train()
        clips = torch.randn(args.batch, 180, 22, 3, device=dev)
        labels = torch.arange(args.batch, device=dev) % 14
        ce = torch.nn.CrossEntropyLoss()
        blocks = [b for b in model.modules() if isinstance(b, Block)]

        def step(path):
            for b in blocks:
                b.force_torch = path == "torch"
            if path == "hip_all":
                set_hip_min_tokens(model, 0)
            elif path == "hip":
                for b in blocks:
                    b.hip_train_min_tokens = HIP_TRAIN_MIN_TOKENS
            model.zero_grad(set_to_none=True)
            ce(model(clips), labels).backward()
        ts = alternate({p: partial(step, p) for p in ("torch", "hip", "hip_all")}, args.repeats, args.warmup)
        med = {k: statistics.median(v) for k, v in ts.items()}
        res["models"][style] = {
            "torch_ms": summary(ts["torch"]), "hip_ms": summary(ts["hip"]), "hip_every_block_ms": summary(ts["hip_all"]),
            "speedup_median": round(med["torch"] / med["hip"], 3),
            "clips_per_s_hip": round(args.batch / (med["hip"] * 1e-3), 1),
            "clips_per_s_torch": round(args.batch / (med["torch"] * 1e-3), 1)}
        del model
        torch.cuda.empty_cache()
    emit(res, args.out)


if __name__ == "__main__":
    main()
