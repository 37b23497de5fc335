#!/usr/bin/env python3
"""Time the HIP gcn_unit_attention at the LMDHG STR shapes (N = 32, V = 46; LMDHG/ST_TR/LMDHG_ST_TR.py): eval forward and
training forward + backward.

Without --math: against a torch-op fp32 restatement of the same math (same process, same GPU).  Prints one JSON line: per
shape {hip_eval_ms, torch_eval_ms, hip_train_ms, torch_train_ms}.

With --math f32,bf16x3: the unit's arithmetics (set_st_attention_math) against each other.  Per shape and pass the
arithmetics alternate inside one process in --blocks blocks of --iters iterations each, after a warm-up per arithmetic; reported
per arithmetic: the median block and the spread (min, max) between blocks, and per pair the verdict - "faster" / "slower" only
where the two ranges of blocks do not overlap, else "tie".  --out writes the JSON to a file as well."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "st-gcn-altformer_amd"), os.path.join(ROOT, "tests")]

import torch                                  # noqa: E402

import st_attention_ref as R                  # noqa: E402
from stgcn_amd import gcn_unit_attention, set_st_attention_math      # noqa: E402

SHAPES = [(131, 256, 300), (256, 256, 150), (256, 512, 150), (512, 512, 75)]
N, V = 32, 46


def timed(fn, warmup=2, iters=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def unit(cin, cout, dev):
    sd = R.make_state(cin, cout, V, 1)
    m = gcn_unit_attention(cin, cout, torch.zeros(3, V, V), **R.unit_kwargs(V))
    m.load_state_dict(sd)
    return m.to(dev), sd


def against_torch(dev):
    res = {}
    for cin, cout, T in SHAPES:
        m, sd = unit(cin, cout, dev)
        x = torch.randn(N, cin, T, V, device=dev)
        sdd = {k: (v.to(dev).float().requires_grad_(True) if v.is_floating_point() else v.to(dev)) for k, v in sd.items()}
        mask = torch.bernoulli(0.5 * torch.ones(N * T * R.NH * V, device=dev))
        r = {}
        m.eval()
        with torch.no_grad():
            r["hip_eval_ms"] = timed(lambda: m(x))
            r["torch_eval_ms"] = timed(lambda: R.forward64(sdd, x, False))
        m.train()
        xg = x.clone().requires_grad_(True)
        r["hip_train_ms"] = timed(lambda: m(xg).sum().backward())
        r["torch_train_ms"] = timed(lambda: R.forward64(sdd, xg, True, mask)[0].sum().backward())
        res[f"{cin}->{cout},T={T}"] = {k: round(v, 3) for k, v in r.items()}
        del m, x, xg, sdd
        torch.cuda.empty_cache()
    return {"tool": "time_st_attention", "N": N, "V": V, "shapes": res}


def between_arithmetics(dev, modes, blocks, iters, shapes):
    res = {}
    for cin, cout, T in shapes:
        m, _ = unit(cin, cout, dev)
        x = torch.randn(N, cin, T, V, device=dev)
        xg = x.clone().requires_grad_(True)
        dy = torch.randn(N, cout, T, V, device=dev)

        def eval_pass():
            with torch.no_grad():
                m(x)

        def train_pass():
            m(xg).backward(dy)

        entry = {}
        for what, fn, training in (("eval", eval_pass, False), ("train", train_pass, True)):
            m.train(training)
            for mode in modes:                       # warm-up per arithmetic and pass
                set_st_attention_math(m, mode)
                timed(fn, warmup=2, iters=1)
            ms = {mode: [] for mode in modes}
            for _ in range(blocks):                  # the arithmetics alternate
                for mode in modes:
                    set_st_attention_math(m, mode)
                    ms[mode].append(timed(fn, warmup=1, iters=iters))
            r = {mode: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                 for mode, v in ms.items()}
            if "f32" in ms:
                for mode in modes:
                    if mode != "f32":
                        faster, slower = max(ms[mode]) < min(ms["f32"]), min(ms[mode]) > max(ms["f32"])
                        r[f"{mode}_vs_f32"] = {"speedup": round(statistics.median(ms["f32"]) / statistics.median(ms[mode]), 3),
                                               "verdict": "faster" if faster else "slower" if slower else "tie"}
            entry[what] = r
        res[f"{cin}->{cout},T={T}"] = entry
        del m, x, xg, dy
        torch.cuda.empty_cache()
    return {"tool": "time_st_attention", "N": N, "V": V, "math": modes, "blocks": blocks, "iters": iters,
            "device": torch.cuda.get_device_name(dev), "shapes": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--math", default=None, help="comma-separated arithmetics to compare, e.g. f32,bf16x3")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shapes", default=None, help="indices into the four shapes, e.g. 0,3 (default: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.math is None:
        out = against_torch(dev)
    else:
        shapes = SHAPES if a.shapes is None else [SHAPES[int(i)] for i in a.shapes.split(",")]
        out = between_arithmetics(dev, a.math.split(","), a.blocks, a.iters, shapes)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
