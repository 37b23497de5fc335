#!/usr/bin/env python3
"""Time the HIP gcn_unit_attention against a torch-op fp32 restatement of the same math (same process, same GPU) at the
LMDHG STR shapes (N = 32, V = 46; LMDHG/ST_TR/LMDHG_ST_TR.py): eval forward and training forward + backward.
Prints one JSON line: per shape {hip_eval_ms, torch_eval_ms, hip_train_ms, torch_train_ms}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "st-gcn-altformer_amd"), os.path.join(ROOT, "tests")]

import torch                                  # noqa: E402

import st_attention_ref as R                  # noqa: E402
from stgcn_amd import gcn_unit_attention      # noqa: E402

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


def main():
    dev = torch.device("cuda:0")
    res = {}
    for cin, cout, T in SHAPES:
        sd = R.make_state(cin, cout, V, 1)
        m = gcn_unit_attention(cin, cout, torch.zeros(3, V, V), **R.unit_kwargs(V))
        m.load_state_dict(sd)
        m = m.to(dev)
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
    print(json.dumps({"tool": "time_st_attention", "N": N, "V": V, "shapes": res}))


if __name__ == "__main__":
    main()
