#!/usr/bin/env python3
"""In-kernel cycle stamps of KF6 at the headline shape, all eight slots of the full and of the short tile form (diagnostic library only; V6_STAMP / V6_ACC in csrc/kf6.h).

    STGCN_LIB=.../libstgcn_hip_abl.so python tools/stamps_kf6.py [--clips N] [--ntvc]

tools/stamps.py names the slots of the v4 kernel; in KF6 slots 4-7 split the main loop by kind of pair.  Mean, minimum and
maximum over the stamped waves (workgroups 0-15, four waves each), cycles summed over a wave's tiles and per tile.  The tiles a
stamped workgroup walks come from the library's own walk (stgcn_stem_walk_run), so any clip count can be stamped: with
--clips 1, 2, 4, 8, 16 the launch has 16 x N workgroups of one tile each, which all reach their epilogue together (the store
concurrency sweep of profiles/store_phase_concurrency.txt).
"""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn-altformer_amd")); sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=256)
ap.add_argument("--ntvc", action="store_true", help="(N,T,V,C) output instead of (N,C,T,V)")
args = ap.parse_args()
import torch
import bench
import stgcn_amd
dev = torch.device("cuda:0")
N, T, V, NWG = args.clips, 180, 22, 16
x = bench.synthetic_clips(N, T, V, 0).to(dev)
gcn, tcn = bench.build_stem(V, "SHRE", "bf16x3")
gcn, tcn = gcn.to(dev).eval(), tcn.to(dev).eval()
stgcn_amd.enable_stem_fusion(gcn, tcn)
if args.ntvc: stgcn_amd.set_output_layout(tcn, "channels_last")
buf = torch.zeros(NWG * 8 * 8, dtype=torch.int64, device=dev)
with torch.no_grad():
    for _ in range(50): tcn(gcn(x))
    torch.cuda.synchronize()
    os.environ["STGCN_ABLATE"] = "0"
    os.environ["STGCN_DBG_PTR"] = hex(buf.data_ptr())
    tcn(gcn(x)); torch.cuda.synchronize()
raw = buf.cpu().view(NWG, 8, 8).double()
names = ["0 chunk-0 phase + barrier", "1 main loop", "2 pair-end wait + barrier (inside 1)", "3 epilogue",
         "4 pairs 1,2,5,6,7,8 (inside 1)", "5 pair 3 (no producer)", "6 pair 4 (no producer)", "7 pair 0 (3 producer blocks)"]
# rows 0-3 of a workgroup: its waves' full tiles; rows 4-7: their short tiles (a clip's last tile of at most 128 pixels, narrow
# three-term form; all zero in a library without the short form, which then runs full-cost tiles only)
short = raw[:, 4:]
has_short = bool(short.sum() > 0)
# the tiles of each stamped workgroup, from the library's walk
tpc = -(-T * V // 256)
G = min(N * tpc, torch.cuda.get_device_properties(0).multi_processor_count)
nwg = min(NWG, G)
lib = stgcn_amd.lib()
nfull, nshort = torch.zeros(NWG), torch.zeros(NWG)
for b in range(nwg):
    first, end = ctypes.c_int(), ctypes.c_int()
    assert lib.stgcn_stem_walk_run(b, G, N, tpc, 1 if has_short else 0, ctypes.byref(first), ctypes.byref(end)) == 0
    ns = sum(1 for t in range(first.value, end.value) if has_short and (t + 1) % tpc == 0)
    nshort[b], nfull[b] = ns, end.value - first.value - ns
print(f"{N} clips of {T} x {V}, {'(N,T,V,C)' if args.ntvc else '(N,C,T,V)'} output: {G} workgroups, {N * tpc} tiles; stamped: workgroups 0-{nwg - 1}")
forms = [("full tiles", raw[:, :4], nfull)] + ([("short tiles", short, nshort)] if has_short else [])
per_tile = {}
for form, t, cnt in forms:
    w = cnt > 0
    if not bool(w.any()):
        continue
    tiles = cnt[w].double().view(-1, 1)
    print(f"{form}: {int(cnt.sum())} in the stamped workgroups ({int(cnt[w].min())} to {int(cnt[w].max())} each); cycles per wave, summed over those tiles, and per tile")
    for i, nm in enumerate(names):
        v = t[w][:, :, i]
        pt = v / tiles
        print(f"  {nm:40s} mean {v.mean():11.0f}  per tile {v.sum() / (4 * tiles.sum()):9.0f}   per tile min {pt.min():9.0f} max {pt.max():9.0f}")
    per_tile[form] = sum(t[w][:, :, i].sum().item() for i in (0, 1, 3)) / (4 * tiles.sum().item())
    print(f"  chunk 0 + main loop + epilogue, per tile: {per_tile[form]:.0f}")
    # the epilogue slot by store-phase class (blockIdx.x >> 3) & 1: workgroups 0-7 and 8-15
    for cls in (0, 1):
        sel = w.clone(); sel[:8] &= cls == 0; sel[8:] &= cls == 1
        if bool(sel.any()):
            print(f"  3 epilogue, workgroups {8 * cls}-{8 * cls + 7}: per tile {t[sel][:, :, 3].sum() / (4 * cnt[sel].sum()):9.0f}")
if len(per_tile) == 2:
    print(f"short / full, chunk 0 + main loop + epilogue: {per_tile['short tiles'] / per_tile['full tiles']:.3f}")
work = (raw[:nwg, :4, 0] + raw[:nwg, :4, 1] + raw[:nwg, :4, 3] + short[:nwg, :, 0] + short[:nwg, :, 1] + short[:nwg, :, 3]).max(dim=1).values
print(f"stamped cycles per workgroup 0-{nwg - 1} (slowest wave; feature phases not stamped): min {work.min():.0f} max {work.max():.0f} "
      f"spread {100 * (work.max() - work.min()) / work.mean():.2f} %")
