#!/usr/bin/env python3
"""In-kernel cycle stamps of KF6 at the headline shape, all eight slots of the full and of the short tile form (diagnostic library only; V6_STAMP / V6_ACC in csrc/kf6.h).

    STGCN_LIB=.../libstgcn_hip_abl.so python tools/stamps_kf6.py

tools/stamps.py names the slots of the v4 kernel; in KF6 slots 4-7 split the main loop by kind of pair.  Mean, minimum and
maximum over the stamped waves (workgroups 0-7, four waves each), cycles summed over a wave's tiles and per tile.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd")); sys.path.insert(0, ROOT)
import torch
import bench
import stgcn_amd
dev = torch.device("cuda:0")
x = bench.synthetic_clips(256, 180, 22, 0).to(dev)
gcn, tcn = bench.build_stem(22, "SHRE", "bf16x3")
gcn, tcn = gcn.to(dev).eval(), tcn.to(dev).eval()
stgcn_amd.enable_stem_fusion(gcn, tcn)
buf = torch.zeros(8 * 8 * 8, dtype=torch.int64, device=dev)
with torch.no_grad():
    for _ in range(50): tcn(gcn(x))
    torch.cuda.synchronize()
    os.environ["STGCN_ABLATE"] = "0"
    os.environ["STGCN_DBG_PTR"] = hex(buf.data_ptr())
    tcn(gcn(x)); torch.cuda.synchronize()
raw = buf.cpu().view(8, 8, 8).double()
names = ["0 chunk-0 phase + barrier", "1 main loop", "2 pair-end wait + barrier (inside 1)", "3 epilogue",
         "4 pairs 1,2,5,6,7,8 (inside 1)", "5 pair 3 (no producer)", "6 pair 4 (no producer)", "7 pair 0 (3 producer blocks)"]
# rows 0-3 of a workgroup: its waves' full tiles; rows 4-7: their short tiles (a clip's last tile of at most 128 pixels, narrow
# three-term form; all zero in a library without the short form, which then runs 16 full-cost tiles per workgroup)
short = raw[:, 4:]
has_short = bool(short.sum() > 0)
forms = [("full tiles", raw[:, :4], 15.0 if has_short else 16.0)] + ([("short tiles", short, 1.0)] if has_short else [])
per_tile = {}
for form, t, tiles in forms:
    print(f"{form}: {tiles:.0f} per workgroup at 256 clips on 256 CUs; cycles per wave, summed over those tiles, and per tile")
    for i, nm in enumerate(names):
        v = t[:, :, i]
        print(f"  {nm:40s} mean {v.mean():11.0f}  per tile {v.mean() / tiles:9.0f}   min {v.min():11.0f} max {v.max():11.0f}")
    per_tile[form] = sum(t[:, :, i].mean().item() for i in (0, 1, 3)) / tiles
    print(f"  chunk 0 + main loop + epilogue, per tile: {per_tile[form]:.0f}")
if has_short:
    print(f"short / full, chunk 0 + main loop + epilogue: {per_tile['short tiles'] / per_tile['full tiles']:.3f}")
    work = (raw[:, :4, 0] + raw[:, :4, 1] + raw[:, :4, 3] + short[:, :, 0] + short[:, :, 1] + short[:, :, 3]).max(dim=1).values
    print(f"stamped cycles per workgroup 0-7 (slowest wave; feature phases not stamped): min {work.min():.0f} max {work.max():.0f} "
          f"spread {100 * (work.max() - work.min()) / work.mean():.2f} %")
else:
    work = (raw[:, :4, 0] + raw[:, :4, 1] + raw[:, :4, 3]).max(dim=1).values
    print(f"stamped cycles per workgroup 0-7 (slowest wave; feature phases not stamped): min {work.min():.0f} max {work.max():.0f} "
          f"spread {100 * (work.max() - work.min()) / work.mean():.2f} %")
