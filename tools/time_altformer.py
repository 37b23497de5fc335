#!/usr/bin/env python3
"""Time the AltFormer heads: the HIP path of every stage's transformer block and of the whole ST / TS models against the
torch-op path of the same module, in one process, alternating, with device events.

    python tools/time_altformer.py [--batch 32] [--repeats 7] [--warmup 2] [--tiles 128|auto|64|32|sweep]
                                   [--out profiles/altformer_times.json]
    python tools/time_altformer.py --frames 500 [--batch 32] [--out profiles/altformer_long_times.json]
    python tools/time_altformer.py --math bf16 [--batch 32] [--out profiles/altformer_bf16_times.json]
    python tools/time_altformer.py --attention split [--out profiles/altformer_split_attention_times.json]
    python tools/time_altformer.py --head whole [--batches 1,32] [--out profiles/altformer_whole_head_times.json]

Prints ONE JSON line.  Per stage (a Block at the stage's shape, batch ``--batch``): ms of the HIP path (default arithmetic,
and 'f32' / 'bf16x3' for comparison) and of the torch path (min, median, max over the repeats; ``spread`` = (max - min) / min of
the torch path and of the HIP path, the noise the comparison has to be read against), the block's FLOPs counted from the
shapes, and per launch (the four linears in the arithmetic the default uses for them, the attention) ms, achieved TFLOP/s and
the share of the relevant peak: 155 TFLOP/s for the fp32 matrix cores (measured), 2500 / 3 for bf16x3.  Whole models: the
reference's SHREC configuration (14 classes, 180 frames, 22 joints) from skeleton clips to logits, stem + head, clips/s.

``--tiles`` sets the tile form of the linears (STGCN_VIT_TILE_*) on every HIP row; ``sweep`` times all four forms of every
stage and launch in the same alternation (``tiles`` per stage: block ms per form, the forms ``auto`` picked for the four
linears, ms per launch per form, the attention's share of the ``auto`` block) and adds ``low_latency`` per model: the
default policy (at one clip: every block on torch ops), ``set_low_latency`` eager, and the same forward captured in a graph
and replayed.

``--frames T`` (T > 256) times the long-clip stages instead, where the attention is the streaming kernel: the ST temporal stage
(``batch`` sequences of T, D = 512) and the TS temporal stage for 22 and 46 joints (``batch`` x V sequences of T, D = 256),
HIP against torch path with ``torch.cuda.max_memory_allocated`` of each; per launch the streaming kernel at L = T for head_dim
32 and 64 next to the resident kernel at L = 256 in the same alternation (ms, TFLOP/s, their ratio); and the whole ST and TS
models at ``num_frame = T``.

``--math bf16`` times the opt-in bf16 block mode (``set_head_math(m, 'bf16')``) against the default arithmetic ('mixed') in the
same alternation: per stage the block in both, per launch the five launches of both (the bf16 ones on the bf16 tensors the
mode keeps between them), and the whole ST and TS models under the module's default policy.  Every ratio is median over
median and comes with ``spread``, the larger (max - min) / min of the two rows, and ``bf16_faster_by_more_than_the_spread``.

``--attention split`` times the split attention kernel (``STGCN_VIT_ATTN_SPLIT``) against the resident one in the same
alternation, at every batch of ``--batches`` (1, 2, 4, 8, 32) for the three stage shapes with two key tiles or more (L 180 at
head_dim 64 and 32, L 46 at head_dim 64; ``batch`` sequences of 8 heads): the attention launch alone
(``stgcn_vit_attention`` / ``stgcn_vit_attention_split``), the block with and without the flag ('mixed', auto tiles), and the
whole one-clip ST and TS models under ``set_low_latency(min_tokens=0)``, eager and captured, with and without
``split_attention``.  A launch or block sample is ``--inner`` (20) calls between two events, reported per call.  Every row
has ``spread`` and ``split_faster_by_more_than_the_spread`` / ``split_slower_by_more_than_the_spread``.

``--head whole`` times the one-call head (``set_whole_head``, ``stgcn_altformer_head_forward``) against the per-block path in
the same alternation, at every batch of ``--batches`` (default 1,32), styles ST and TS: the head alone on a fixed stem output
and the whole model from skeleton clips, each eager and captured in a graph.  The per-block arm is the policy a user has
without the switch: ``set_low_latency(model, min_tokens=0)`` at fewer than 8 clips, the default thresholds from there on.  A
sample is ``max(1, --inner // batch)`` forwards between two events, reported per forward.  Every row has ``spread`` and
``whole_faster_by_more_than_the_spread`` / ``whole_slower_by_more_than_the_spread``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd"))

PEAK_F32 = 155.0            # TFLOP/s, v_mfma_f32_32x32x2_f32, measured
PEAK_BF16X3 = 2500.0 / 3    # three bf16 products per fp32 product

# stage: (sequences per clip, L, D) - the heads of the reference's three scripts (SHREC, DHG: V = 22; LMDHG: V = 46)
STAGES = {
    "ST spatial SHREC (180 x 22)": (180, 22, 256),
    "ST spatial DHG (150 x 22)": (150, 22, 256),
    "ST temporal 180": (1, 180, 512),
    "ST temporal 150": (1, 150, 512),
    "TS temporal LMDHG (46 x 180)": (46, 180, 256),
    "TS temporal (22 x 180)": (22, 180, 256),
    "TS spatial 46": (1, 46, 512),
    "TS spatial 22": (1, 22, 512),
}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, repeats, warmup):
    """{name: [ms, ...]}: the candidates run in turn, ``warmup`` untimed rounds first."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(events(fn))
    return out


def summary(ts):
    return {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4), "max": round(max(ts), 4),
            "spread": round((max(ts) - min(ts)) / min(ts), 4)}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def faster_by_more_than_the_spread(fast, slow):
    return statistics.median(fast) * (1 + max(summary(fast)["spread"], summary(slow)["spread"])) < statistics.median(slow)


def long_clips(args):
    """The ``--frames`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import DEFAULT_HEAD_MATH, Block
    from functools import partial
    T, dev = args.frames, torch.device("cuda:0")
    assert T > 256, "--frames is for sequences the resident attention kernel does not take"
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    res = {"frames": T, "batch": args.batch, "repeats": args.repeats, "default_math": DEFAULT_HEAD_MATH,
           "device": torch.cuda.get_device_name(0), "stages": {}, "attention": {}, "models": {}}
    stages = {f"ST temporal {T}": (1, 512), f"TS temporal (22 x {T})": (22, 256), f"TS temporal two-hand (46 x {T})": (46, 256)}
    with torch.no_grad():
        for name, (per_clip, D) in stages.items():
            B, heads = args.batch * per_clip, 8
            torch.manual_seed(0)
            blk = Block(D, heads, mlp_ratio=2., qkv_bias=True, norm_layer=norm).to(dev).eval()
            x = torch.randn(B, T, D, device=dev)
            chooses = "hip" if blk.uses_hip(x) else "torch"
            blk.hip_min_tokens = 0

            def run(torch_path):
                blk.force_torch = torch_path
                return blk(x)
            ts = alternate({"torch": partial(run, True), "hip": partial(run, False)}, args.repeats, args.warmup)
            mem = {k: peak_bytes(partial(run, k == "torch")) for k in ("torch", "hip")}
            blk.force_torch = False
            M, hd = B * T, D // heads
            flops = 2 * M * D * 3 * D + 4 * B * heads * T * T * hd + 2 * M * D * D + 2 * 2 * M * D * 2 * D
            res["stages"][name] = {
                "B": B, "L": T, "D": D, "tokens": M, "module_chooses": chooses, "gflop": round(flops / 1e9, 2),
                "attention_gflop": round(4 * B * heads * T * T * hd / 1e9, 2),
                "hip_ms": summary(ts["hip"]), "torch_ms": summary(ts["torch"]),
                "speedup_median": round(statistics.median(ts["torch"]) / statistics.median(ts["hip"]), 3),
                "hip_faster_by_more_than_the_spread": faster_by_more_than_the_spread(ts["hip"], ts["torch"]),
                "peak_mib_hip": round(mem["hip"] / 2 ** 20, 1), "peak_mib_torch": round(mem["torch"] / 2 ** 20, 1)}
            del x, blk
            torch.cuda.empty_cache()
        # per launch: the streaming kernel at L = T and the resident kernel at L = 256, the same number of (sequence, head) pairs
        B, heads = args.batch * 22, 8
        for hd in (32, 64):
            qs, qr = (torch.randn(B, L, 3 * heads * hd, device=dev) for L in (T, 256))
            lt = alternate({"stream": lambda: F.vit_attention_stream(qs, heads), "resident": lambda: F.vit_attention(qr, heads),
                            "stream_at_256": lambda: F.vit_attention_stream(qr, heads)}, args.repeats, args.warmup)
            tf = {k: 4 * B * heads * L * L * hd / (statistics.median(lt[k]) * 1e-3) / 1e12
                  for k, L in (("stream", T), ("resident", 256), ("stream_at_256", 256))}
            res["attention"][f"head_dim {hd}"] = {
                "B": B, "heads": heads, "stream_L": T, "resident_L": 256, "ms": {k: summary(t) for k, t in lt.items()},
                "tflops": {k: round(v, 1) for k, v in tf.items()}, "share_of_peak": {k: round(v / PEAK_F32, 3) for k, v in tf.items()},
                "stream_over_resident_tflops": round(tf["stream"] / tf["resident"], 3),
                "stream_over_resident_tflops_at_256": round(tf["stream_at_256"] / tf["resident"], 3)}
            del qs, qr
        for style in ("ST", "TS"):
            torch.manual_seed(1)
            model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=T, num_joints=22, style=style,
                                               graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).eval()
            clips = torch.randn(args.batch, T, 22, 3, device=dev)
            blocks = [b for b in model.modules() if isinstance(b, Block)]

            def run_model(torch_path):
                for b in blocks:
                    b.force_torch = torch_path
                return model(clips)
            calls = []
            hooks = [b.register_forward_pre_hook(lambda mod, a: calls.append(bool(mod.uses_hip(a[0])))) for b in blocks]
            run_model(False)
            for hk in hooks:
                hk.remove()
            ts = alternate({"torch": partial(run_model, True), "hip": partial(run_model, False)}, args.repeats, args.warmup)
            mem = {k: peak_bytes(partial(run_model, k == "torch")) for k in ("torch", "hip")}
            res["models"][style] = {"hip_ms": summary(ts["hip"]), "torch_ms": summary(ts["torch"]),
                                    "blocks_on_hip_default_policy": sum(calls), "blocks": len(calls),
                                    "speedup_median": round(statistics.median(ts["torch"]) / statistics.median(ts["hip"]), 3),
                                    "clips_per_s_hip": round(args.batch / (statistics.median(ts["hip"]) * 1e-3), 1),
                                    "clips_per_s_torch": round(args.batch / (statistics.median(ts["torch"]) * 1e-3), 1),
                                    "peak_mib_hip": round(mem["hip"] / 2 ** 20, 1), "peak_mib_torch": round(mem["torch"] / 2 ** 20, 1)}
            del model, clips
            torch.cuda.empty_cache()
    return res


def bf16_mode(args):
    """The ``--math bf16`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import DEFAULT_HEAD_MATH, HEAD_MATH, Block, set_head_math
    from functools import partial
    dev = torch.device("cuda:0")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    assert DEFAULT_HEAD_MATH == "mixed"
    res = {"math": "bf16", "against": DEFAULT_HEAD_MATH, "batch": args.batch, "repeats": args.repeats, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "stages": {}, "models": {}}

    def versus(base, bf16):
        spread = max(summary(base)["spread"], summary(bf16)["spread"])
        return {"mixed_ms": summary(base), "bf16_ms": summary(bf16),
                "mixed_over_bf16": round(statistics.median(base) / statistics.median(bf16), 3), "spread": round(spread, 4),
                "bf16_faster_by_more_than_the_spread": faster_by_more_than_the_spread(bf16, base)}
    with torch.no_grad():
        for name, (per_clip, L, D) in STAGES.items():
            B = args.batch * per_clip
            M, hidden, heads = B * L, 2 * D, 8
            torch.manual_seed(0)
            blk = Block(D, heads, mlp_ratio=2., qkv_bias=True, norm_layer=norm).to(dev).eval()
            x = torch.randn(B, L, D, device=dev)
            blk.hip_min_tokens = 0

            def run(mode):
                set_head_math(blk, mode)
                return blk(x)
            ts = alternate({m: partial(run, m) for m in ("mixed", "bf16")}, args.repeats, args.warmup)
            err = (run("bf16") - run("mixed")).abs().max().item() / run("mixed").abs().max().item()
            a, m = blk.attn, blk.mlp
            ln1, ln2 = (blk.norm1.weight, blk.norm1.bias, 1e-6), (blk.norm2.weight, blk.norm2.bias, 1e-6)
            qkv = F.vit_linear(x, a.qkv.weight, a.qkv.bias, ln=ln1, math=F.MATH_F32)
            att = F.vit_attention(qkv, heads, a.scale)
            h = F.vit_linear(x, m.fc1.weight, m.fc1.bias, ln=ln2, gelu=True, math=F.MATH_BF16X3)
            qkv_b, att_b, h_b = qkv.bfloat16(), att.bfloat16(), h.bfloat16()
            parts = alternate({
                "qkv mixed": lambda: F.vit_linear(x, a.qkv.weight, a.qkv.bias, ln=ln1, math=F.MATH_F32),
                "qkv bf16": lambda: F.vit_linear_bf16(x, a.qkv.weight, a.qkv.bias, ln=ln1, y_bf16=True),
                "attention mixed": lambda: F.vit_attention(qkv, heads, a.scale),
                "attention bf16": lambda: F.vit_attention_bf16(qkv_b, heads, a.scale),
                "proj mixed": lambda: F.vit_linear(att, a.proj.weight, a.proj.bias, residual=x, math=F.MATH_BF16X3),
                "proj bf16": lambda: F.vit_linear_bf16(att_b, a.proj.weight, a.proj.bias, residual=x),
                "fc1 mixed": lambda: F.vit_linear(x, m.fc1.weight, m.fc1.bias, ln=ln2, gelu=True, math=F.MATH_BF16X3),
                "fc1 bf16": lambda: F.vit_linear_bf16(x, m.fc1.weight, m.fc1.bias, ln=ln2, gelu=True, y_bf16=True),
                "fc2 mixed": lambda: F.vit_linear(h, m.fc2.weight, m.fc2.bias, residual=x, math=F.MATH_BF16X3),
                "fc2 bf16": lambda: F.vit_linear_bf16(h_b, m.fc2.weight, m.fc2.bias, residual=x),
            }, args.repeats, args.warmup)
            flops = {"qkv": 2 * M * D * 3 * D, "attention": 4 * B * heads * L * L * (D // heads), "proj": 2 * M * D * D,
                     "fc1": 2 * M * D * hidden, "fc2": 2 * M * hidden * D}
            launches = {}
            for k, fl in flops.items():
                launches[k] = versus(parts[k + " mixed"], parts[k + " bf16"])
                launches[k]["gflop"] = round(fl / 1e9, 3)
                launches[k]["bf16_tflops"] = round(fl / (min(parts[k + " bf16"]) * 1e-3) / 1e12, 1)
            res["stages"][name] = dict(versus(ts["mixed"], ts["bf16"]), B=B, L=L, D=D, tokens=M,
                                       gflop=round(sum(flops.values()) / 1e9, 2), bf16_vs_mixed_max_err=float(f"{err:.3e}"),
                                       launches=launches)
            del x, blk, qkv, att, h, qkv_b, att_b, h_b
            torch.cuda.empty_cache()
        for style in ("ST", "TS"):
            torch.manual_seed(1)
            model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style,
                                               graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).eval()
            clips = torch.randn(args.batch, 180, 22, 3, device=dev)

            def run_model(mode):
                set_head_math(model, mode)
                return model(clips)
            blocks = [b for b in model.modules() if isinstance(b, Block)]
            calls = []
            hooks = [b.register_forward_pre_hook(lambda mod, a: calls.append(bool(mod.uses_hip(a[0])))) for b in blocks]
            run_model("bf16")
            for hk in hooks:
                hk.remove()
            ts = alternate({m: partial(run_model, m) for m in ("mixed", "bf16")}, args.repeats, args.warmup)
            lm, lb = run_model("mixed"), run_model("bf16")
            res["models"][style] = dict(versus(ts["mixed"], ts["bf16"]), blocks_on_hip_default_policy=sum(calls), blocks=len(calls),
                                        clips_per_s_mixed=round(args.batch / (statistics.median(ts["mixed"]) * 1e-3), 1),
                                        clips_per_s_bf16=round(args.batch / (statistics.median(ts["bf16"]) * 1e-3), 1),
                                        bf16_vs_mixed_max_logit_err=float(f"{(lb - lm).abs().max().item() / lm.abs().max().item():.3e}"),
                                        argmax_equal=bool(torch.equal(lb.argmax(1), lm.argmax(1))))
            del model, clips
            torch.cuda.empty_cache()
    big = [v for v in res["stages"].values() if v["tokens"] >= 100000]
    res["stages_of_100k_tokens_and_more"] = len(big)
    res["bf16_faster_at_all_of_them"] = all(v["bf16_faster_by_more_than_the_spread"] for v in big)
    assert HEAD_MATH["bf16"] == F.VIT_BF16
    return res


def split_attention(args):
    """The ``--attention split`` run (see the module docstring)."""
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import DEFAULT_HEAD_MATH, HEAD_MATH, Block
    from functools import partial
    dev = torch.device("cuda:0")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    batches = [int(b) for b in args.batches.split(",")]
    heads, n = 8, args.inner
    shapes = {"ST temporal (L 180, head_dim 64)": (180, 512), "TS temporal (L 180, head_dim 32)": (180, 256),
              "TS spatial LMDHG (L 46, head_dim 64)": (46, 512)}
    res = {"attention": "split", "batches": batches, "repeats": args.repeats, "warmup": args.warmup, "launches_per_sample": n,
           "device": torch.cuda.get_device_name(0), "block_math": DEFAULT_HEAD_MATH + " | VIT_TILE_AUTO", "launch": {}, "block": {},
           "models": {}}

    def versus(base, split, per=1):
        spread = max(summary(base)["spread"], summary(split)["spread"])
        return {"resident_ms": summary([t / per for t in base]), "split_ms": summary([t / per for t in split]),
                "resident_over_split": round(statistics.median(base) / statistics.median(split), 3), "spread": round(spread, 4),
                "split_faster_by_more_than_the_spread": faster_by_more_than_the_spread(split, base),
                "split_slower_by_more_than_the_spread": faster_by_more_than_the_spread(base, split)}

    def times(fn):
        for _ in range(n):
            fn()
    with torch.no_grad():
        for name, (L, D) in shapes.items():
            hd = D // heads
            res["launch"][name], res["block"][name] = {}, {}
            torch.manual_seed(0)
            blk = Block(D, heads, mlp_ratio=2., qkv_bias=True, norm_layer=norm).to(dev).eval()
            a, m = blk.attn, blk.mlp
            params = ((blk.norm1.weight, blk.norm1.bias), (a.qkv.weight, a.qkv.bias), (a.proj.weight, a.proj.bias),
                      (blk.norm2.weight, blk.norm2.bias), (m.fc1.weight, m.fc1.bias), (m.fc2.weight, m.fc2.bias))
            math = HEAD_MATH[DEFAULT_HEAD_MATH] | F._capi.VIT_TILE_AUTO
            for B in batches:
                qkv = torch.randn(B, L, 3 * D, device=dev)
                lt = alternate({"resident": partial(times, lambda: F.vit_attention(qkv, heads)),
                                "split": partial(times, lambda: F.vit_attention_split(qkv, heads))}, args.repeats, args.warmup)
                res["launch"][name][f"batch {B}"] = dict(versus(lt["resident"], lt["split"], n), pairs=B * heads,
                                                         workgroups_resident=-(-B * heads // max(1, 4 // -(-L // 32))),
                                                         workgroups_split=B * heads * -(-L // 32))
                x = torch.randn(B, L, D, device=dev)
                form = F.vit_block_attention_form(B, L, D, heads, 2 * D, math | F.VIT_ATTN_SPLIT)
                bt = alternate({"resident": partial(times, lambda: F.vit_block_forward(x, *params, heads, 1e-6, a.scale, math)),
                                "split": partial(times, lambda: F.vit_block_forward(x, *params, heads, 1e-6, a.scale, math | F.VIT_ATTN_SPLIT))},
                               args.repeats, args.warmup)
                res["block"][name][f"batch {B}"] = dict(versus(bt["resident"], bt["split"], n), pairs=B * heads, flagged_call_runs=form)
                del qkv, x
            del blk
        for style in ("ST", "TS"):
            torch.manual_seed(1)
            model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style,
                                               graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).eval()
            clip = torch.randn(1, 180, 22, 3, device=dev)

            def run_eager(split):
                stgcn_amd.set_low_latency(model, min_tokens=0, split_attention=split)
                return model(clip)
            graphs, ins, outs = {}, {}, {}               # a graph's static input lives as long as the graph is replayed
            for split in (False, True):
                want = run_eager(split).clone()          # also warms the modules' caches
                torch.cuda.synchronize()
                ins[split] = clip.clone()
                graphs[split] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[split]):
                    outs[split] = model(ins[split])
                graphs[split].replay()
                torch.cuda.synchronize()
                assert torch.equal(outs[split], want), f"{style}: the replay differs from the eager result (split {split})"
            blocks = [b for b in model.modules() if isinstance(b, Block)]
            forms = []
            hooks = [b.register_forward_pre_hook(lambda mod, ar: forms.append(F.vit_block_attention_form(
                ar[0].shape[0], ar[0].shape[1], ar[0].shape[2], mod.attn.num_heads, mod.mlp.fc1.out_features,
                mod._hip_flags(ar[0], train=False)))) for b in blocks]
            run_eager(True)
            for hk in hooks:
                hk.remove()
            tl = alternate({"eager": partial(run_eager, False), "eager_split": partial(run_eager, True),
                            "captured": graphs[False].replay, "captured_split": graphs[True].replay}, args.repeats, args.warmup)
            err = (outs[True] - outs[False]).abs().max().item() / outs[False].abs().max().item()
            res["models"][style] = {"clips": 1, "blocks": len(forms), "blocks_on_the_split_kernel": forms.count("resident_split"),
                                    "eager": versus(tl["eager"], tl["eager_split"]), "captured": versus(tl["captured"], tl["captured_split"]),
                                    "split_vs_resident_max_logit_err": float(f"{err:.3e}"),
                                    "argmax_equal": bool(torch.equal(outs[True].argmax(1), outs[False].argmax(1)))}
            stgcn_amd.set_low_latency(model, False)
            del model, graphs, ins, outs
            torch.cuda.empty_cache()
    below = [v for rows in res["launch"].values() for v in rows.values() if v["pairs"] < 256]
    res["split_faster_at_every_launch_below_256_pairs"] = all(v["split_faster_by_more_than_the_spread"] for v in below)
    res["split_slower_at_some_launch_below_256_pairs"] = any(v["split_slower_by_more_than_the_spread"] for v in below)
    return res


def whole_head(args):
    """The ``--head whole`` run (see the module docstring)."""
    import stgcn_amd
    from functools import partial
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    res = {"head": "whole", "batches": batches, "repeats": args.repeats, "warmup": args.warmup, "inner": args.inner,
           "device": torch.cuda.get_device_name(0), "rows": {}}

    def versus(base, whole, per):
        spread = max(summary(base)["spread"], summary(whole)["spread"])
        return {"per_block_ms": summary([t / per for t in base]), "whole_ms": summary([t / per for t in whole]),
                "per_block_over_whole": round(statistics.median(base) / statistics.median(whole), 3), "spread": round(spread, 4),
                "whole_faster_by_more_than_the_spread": faster_by_more_than_the_spread(whole, base),
                "whole_slower_by_more_than_the_spread": faster_by_more_than_the_spread(base, whole)}
    with torch.no_grad():
        for style in ("ST", "TS"):
            torch.manual_seed(1)
            model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style,
                                               graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).eval()
            head = model.modelA if style == "ST" else model.modelB
            for N in batches:
                n = max(1, args.inner // N)
                stgcn_amd.set_low_latency(model, N < 8, min_tokens=0 if N < 8 else None)
                clip = torch.randn(N, 180, 22, 3, device=dev)
                stgcn_amd.set_whole_head(model, False)
                z = model.tcn0(model.gcn0(clip.permute(0, 3, 1, 2))).clone()
                subjects = {"head": (head, z), "model": (model, clip)}
                row = {"clips": N, "forwards_per_sample": n,
                       "per_block_policy": "set_low_latency(min_tokens=0)" if N < 8 else "default thresholds"}
                for what, (mod, x) in subjects.items():
                    def run_eager(whole, mod=mod, x=x):
                        stgcn_amd.set_whole_head(model, whole)
                        for _ in range(n):
                            out = mod(x)
                        return out
                    graphs, ins, outs = {}, {}, {}
                    for whole in (False, True):
                        want = run_eager(whole).clone()
                        assert head.runs_whole(z) == whole
                        torch.cuda.synchronize()
                        ins[whole] = x.clone()
                        graphs[whole] = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graphs[whole]):
                            for _ in range(n):
                                outs[whole] = mod(ins[whole])
                        graphs[whole].replay()
                        torch.cuda.synchronize()
                        assert torch.equal(outs[whole], want), f"{style} {what}: the replay differs from the eager result"
                    tl = alternate({"eager": partial(run_eager, False), "eager_whole": partial(run_eager, True),
                                    "captured": graphs[False].replay, "captured_whole": graphs[True].replay}, args.repeats, args.warmup)
                    err = (outs[True] - outs[False]).abs().max().item() / outs[False].abs().max().item()
                    row[what] = {"eager": versus(tl["eager"], tl["eager_whole"], n),
                                 "captured": versus(tl["captured"], tl["captured_whole"], n),
                                 "whole_vs_per_block_max_logit_err": float(f"{err:.3e}"),
                                 "argmax_equal": bool(torch.equal(outs[True].argmax(1), outs[False].argmax(1)))}
                    del graphs, ins, outs
                res["rows"][f"{style} batch {N}"] = row
                stgcn_amd.set_whole_head(model, False)
                stgcn_amd.set_low_latency(model, False)
                del z, clip
                torch.cuda.empty_cache()
            del model, head
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", choices=["whole"], default=None,
                    help="time the one-call head (set_whole_head) against the per-block path: head alone and whole model")
    ap.add_argument("--attention", choices=["split"], default=None,
                    help="time the split attention kernel against the resident one: launch, block and one-clip models")
    ap.add_argument("--batches", default=None,
                    help="--attention split: the batches of the launch and block rows (default 1,2,4,8,32); --head whole: the "
                         "batches of every row (default 1,32)")
    ap.add_argument("--inner", type=int, default=20, help="--attention split: launches (or block calls) per timed sample")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiles", choices=["128", "auto", "64", "32", "sweep"], default="128")
    ap.add_argument("--frames", type=int, default=None, help="time the long-clip stages at this many frames (> 256) instead")
    ap.add_argument("--math", choices=["bf16"], default=None, help="time the opt-in bf16 block mode against the default arithmetic")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    if args.batches is None:
        args.batches = "1,32" if args.head is not None else "1,2,4,8,32"
    if args.frames is not None or args.math is not None or args.attention is not None or args.head is not None:
        line = json.dumps(long_clips(args) if args.frames is not None else bf16_mode(args) if args.math is not None
                          else split_attention(args) if args.attention is not None else whole_head(args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    import stgcn_amd
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import DEFAULT_HEAD_MATH, HEAD_MATH, Block, set_head_math
    from functools import partial
    dev = torch.device("cuda:0")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    res = {"batch": args.batch, "repeats": args.repeats, "default_math": DEFAULT_HEAD_MATH, "device": torch.cuda.get_device_name(0),
           "stages": {}, "models": {}}
    TILE = {"128": 0, "auto": F._capi.VIT_TILE_AUTO, "64": F._capi.VIT_TILE_64, "32": F._capi.VIT_TILE_32}
    sweep = args.tiles == "sweep"
    tile = TILE["128" if sweep else args.tiles]
    res["tiles"] = args.tiles
    flags = HEAD_MATH[DEFAULT_HEAD_MATH]
    math_rest = flags & F._capi.MATH_MASK | tile
    math_qkv = (F.MATH_F32 | tile) if flags & F._capi.VIT_QKV_F32 else math_rest
    with torch.no_grad():
        for name, (per_clip, L, D) in STAGES.items():
            B = args.batch * per_clip
            M, hidden, heads = B * L, 2 * D, 8
            torch.manual_seed(0)
            blk = Block(D, heads, mlp_ratio=2., qkv_bias=True, norm_layer=norm).to(dev).eval()
            x = torch.randn(B, L, D, device=dev)
            chooses = "hip" if blk.uses_hip(x) else "torch"      # what the module does at this size on its own
            blk.hip_min_tokens = 0                               # the stage rows time the kernels whatever the policy says

            def run(mode):
                blk.force_torch = mode == "torch"
                if mode != "torch":
                    set_head_math(blk, HEAD_MATH[mode] | tile)
                return blk(x)
            ts = alternate({m: partial(run, m) for m in ("torch", DEFAULT_HEAD_MATH, "f32", "bf16x3")}, args.repeats, args.warmup)
            blk.force_torch = False
            if sweep:
                def run_form(form):
                    blk.force_torch = form == "torch"
                    if form != "torch":
                        set_head_math(blk, flags | TILE[form])
                    return blk(x)
                form_ts = alternate({f: partial(run_form, f) for f in ("torch", "128", "auto", "64", "32")}, args.repeats, args.warmup)
                blk.force_torch = False
            a, m = blk.attn, blk.mlp
            ln1, ln2 = (blk.norm1.weight, blk.norm1.bias, 1e-6), (blk.norm2.weight, blk.norm2.bias, 1e-6)
            qkv = F.vit_linear(x, a.qkv.weight, a.qkv.bias, ln=ln1, math=math_qkv)
            att = F.vit_attention(qkv, heads, a.scale)
            h = F.vit_linear(x, m.fc1.weight, m.fc1.bias, ln=ln2, gelu=True, math=math_rest)
            parts = alternate({
                "qkv": lambda: F.vit_linear(x, a.qkv.weight, a.qkv.bias, ln=ln1, math=math_qkv),
                "attention": lambda: F.vit_attention(qkv, heads, a.scale),
                "proj": lambda: F.vit_linear(att, a.proj.weight, a.proj.bias, residual=x, math=math_rest),
                "fc1": lambda: F.vit_linear(x, m.fc1.weight, m.fc1.bias, ln=ln2, gelu=True, math=math_rest),
                "fc2": lambda: F.vit_linear(h, m.fc2.weight, m.fc2.bias, residual=x, math=math_rest),
            }, args.repeats, args.warmup)
            flops = {"qkv": 2 * M * D * 3 * D, "attention": 4 * B * heads * L * L * (D // heads), "proj": 2 * M * D * D,
                     "fc1": 2 * M * D * hidden, "fc2": 2 * M * hidden * D}
            launches = {}
            for k, t in parts.items():
                f32 = k == "attention" or (k == "qkv" and math_qkv == F.MATH_F32) or (k != "qkv" and math_rest == F.MATH_F32)
                tf = flops[k] / (min(t) * 1e-3) / 1e12
                launches[k] = {"ms": summary(t), "gflop": round(flops[k] / 1e9, 3), "tflops": round(tf, 1),
                               "arithmetic": "f32" if f32 else "bf16x3",
                               "share_of_peak": round(tf / (PEAK_F32 if f32 else PEAK_BF16X3), 3)}
            hip, tor = ts[DEFAULT_HEAD_MATH], ts["torch"]
            swept = None
            if sweep:
                lin = {"qkv": (x, a.qkv.weight, a.qkv.bias, dict(ln=ln1), math_qkv), "proj": (att, a.proj.weight, a.proj.bias, dict(residual=x), math_rest),
                       "fc1": (x, m.fc1.weight, m.fc1.bias, dict(ln=ln2, gelu=True), math_rest), "fc2": (h, m.fc2.weight, m.fc2.bias, dict(residual=x), math_rest)}
                fns = {f"{k} {f}": partial(F.vit_linear, xi, W, b, math=mt | TILE[f], **kw) for k, (xi, W, b, kw, mt) in lin.items()
                       for f in ("128", "auto", "64", "32")}
                fns["attention"] = lambda: F.vit_attention(qkv, heads, a.scale)
                lt = alternate(fns, args.repeats, args.warmup)
                slab_m = min(B, max(1, 32768 // L)) * L     # the block walks slabs of whole sequences; the plan sees a slab's rows
                med = {f: statistics.median(form_ts[f]) for f in form_ts}
                # the margin of a comparison of two medians: the larger of the two spreads (as hip_not_slower above)
                swept = {"block_ms": {f: summary(t) for f, t in form_ts.items()},
                         "auto_forms": {k: "x".join(map(str, F.vit_linear_tile(slab_m, W.shape[1], W.shape[0], TILE["auto"])))
                                        for k, (xi, W, b, kw, mt) in lin.items()},
                         "launch_ms": {k: summary(t) for k, t in lt.items()},
                         "auto_vs_128": round(med["128"] / med["auto"], 3),
                         "auto_not_slower_than_128": med["auto"] <= med["128"] * (1 + max(summary(form_ts["auto"])["spread"], summary(form_ts["128"])["spread"])),
                         "auto_vs_torch": round(med["torch"] / med["auto"], 3),
                         "auto_beats_torch": med["auto"] * (1 + max(summary(form_ts["auto"])["spread"], summary(form_ts["torch"])["spread"])) < med["torch"],
                         "attention_share_of_auto_block": round(statistics.median(lt["attention"]) / med["auto"], 3)}
            res["stages"][name] = {
                "B": B, "L": L, "D": D, "tokens": M, "module_chooses": chooses, "gflop": round(sum(flops.values()) / 1e9, 2),
                "hip_ms": summary(hip), "torch_ms": summary(tor), "hip_f32_ms": summary(ts["f32"]),
                "hip_bf16x3_ms": summary(ts["bf16x3"]), "speedup_median": round(statistics.median(tor) / statistics.median(hip), 3),
                "hip_not_slower": statistics.median(hip) <= statistics.median(tor) * (1 + summary(hip)["spread"]),
                "tflops_block": round(sum(flops.values()) / (min(hip) * 1e-3) / 1e12, 1), "launches": launches}
            if swept:
                res["stages"][name]["tiles"] = swept
        for style in ("ST", "TS"):
            torch.manual_seed(1)
            model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style,
                                               graph="graph.SHRE", graph_args={"labeling_mode": "spatial"}).to(dev).eval()
            clips = torch.randn(args.batch, 180, 22, 3, device=dev)
            blocks = [b for b in model.modules() if isinstance(b, Block)]

            def run_model(torch_path):
                for b in blocks:
                    b.force_torch = torch_path
                    if not torch_path and not sweep:
                        set_head_math(b, flags | tile)
                return model(clips)
            ts = alternate({"torch": partial(run_model, True), "hip": partial(run_model, False)}, args.repeats, args.warmup)
            stem = alternate({"stem": lambda: model.tcn0(model.gcn0(clips.permute(0, 3, 1, 2)))}, args.repeats, args.warmup)["stem"]
            res["models"][style] = {"hip_ms": summary(ts["hip"]), "torch_ms": summary(ts["torch"]), "stem_ms": summary(stem),
                                    "speedup_median": round(statistics.median(ts["torch"]) / statistics.median(ts["hip"]), 3),
                                    "clips_per_s_hip": round(args.batch / (statistics.median(ts["hip"]) * 1e-3), 1),
                                    "clips_per_s_torch": round(args.batch / (statistics.median(ts["torch"]) * 1e-3), 1)}
            if sweep:
                # the module's own policies (force_torch off): default thresholds, set_low_latency eager, and that forward as a graph
                # low latency with min_tokens=0: the rows that LOW_LATENCY_MIN_TOKENS is read from must not depend on it
                def run_policy(low):
                    for b in blocks:
                        b.force_torch = False
                    stgcn_amd.set_low_latency(model, low, min_tokens=0 if low else None)
                    return model(clips)

                def blocks_on_hip(low):
                    calls = []
                    hooks = [b.register_forward_pre_hook(lambda mod, a: calls.append(bool(mod.uses_hip(a[0])))) for b in blocks]
                    run_policy(low)
                    for hk in hooks:
                        hk.remove()
                    return sum(calls), len(calls)
                on_default, on_low = blocks_on_hip(False), blocks_on_hip(True)
                assert on_low[0] == on_low[1], f"low latency left blocks on the torch path: {on_low}"
                torch.cuda.synchronize()
                static_in = clips.clone()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static_out = model(static_in)
                graph.replay()
                torch.cuda.synchronize()
                same = torch.equal(static_out, run_policy(True))
                tl = alternate({"default": partial(run_policy, False), "low_latency": partial(run_policy, True), "captured": graph.replay},
                               args.repeats, args.warmup)
                stgcn_amd.set_low_latency(model, False)
                med = {k: statistics.median(t) for k, t in tl.items()}
                res["models"][style]["low_latency"] = {
                    "default_policy_ms": summary(tl["default"]), "low_latency_eager_ms": summary(tl["low_latency"]),
                    "low_latency_captured_ms": summary(tl["captured"]), "replay_equals_eager": same,
                    "blocks_on_hip_default": on_default[0], "blocks_on_hip_low_latency": on_low[0], "blocks": on_low[1],
                    "eager_vs_default": round(med["default"] / med["low_latency"], 3),
                    "captured_vs_default": round(med["default"] / med["captured"], 3)}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
