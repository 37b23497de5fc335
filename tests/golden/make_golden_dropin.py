#!/usr/bin/env python3
"""Drop-in fixture FROM THE IMPORTED REFERENCE: what tests/test_dropin_recipe.py holds the shim to.

    python tests/golden/make_golden_dropin.py /path/to/ST-GCN-AltFormer

Build container only (see make_golden.py for the rules: the reference is imported as it lies, only data is written).
Writes dropin_reference.json:
  * imports      every name the reference's files import ``from model.net`` / ``from model.unit_agcn``;
  * state_dicts  (key, shape, dtype) in state_dict order of the stem (``gcn0.*`` / ``tcn0.*``) of the reference's
                 ST_GCN_AltFormer (constructor call of SHREC/ST_TS/train_sttran.py:75-82) and of two TCN_GCN_units
                 (model/ST_TR/ST_TR_new.py:285-372: 64->64, and 64->128 at stride 2).
Harness-side shim: timm is not installed; the three names the reference imports from it are stubbed.
"""
import json
import os
import re
import sys
import types

import numpy as np
import torch

REF = os.path.abspath(sys.argv[1])
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_reference.json")


class _DropPath(torch.nn.Module):
    def __init__(self, drop_prob=0.0):
        super().__init__()

    def forward(self, x):
        return x


_layers = types.ModuleType("timm.models.layers")
_layers.DropPath, _layers.trunc_normal_ = _DropPath, torch.nn.init.trunc_normal_
_layers.to_2tuple = lambda v: v if isinstance(v, tuple) else (v, v)
_timm, _models = types.ModuleType("timm"), types.ModuleType("timm.models")
_timm.models, _models.layers = _models, _layers
sys.modules.update({"timm": _timm, "timm.models": _models, "timm.models.layers": _layers})
sys.path.insert(0, REF)

from model.AltFormer.ST_GCN_AltFormer import ST_GCN_AltFormer   # noqa: E402  (reference)
from model.ST_TR.ST_TR_new import TCN_GCN_unit                  # noqa: E402  (reference)


def imported_names():
    wanted = {"model.net": set(), "model.unit_agcn": set()}
    for dirpath, _, files in os.walk(REF):
        for fn in files:
            if not fn.endswith(".py"):
                continue
            for line in open(os.path.join(dirpath, fn), errors="replace"):
                m = re.match(r"\s*from (model\.net|model\.unit_agcn) import (.+)", line)
                if m:
                    wanted[m.group(1)] |= {n.strip() for n in m.group(2).split("#")[0].split(",") if n.strip()}
    return {k: sorted(v) for k, v in wanted.items()}


def layout(sd, prefixes=("",)):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items() if k.startswith(prefixes)]


def main():
    torch.manual_seed(7)
    net = ST_GCN_AltFormer(channel=3, backbone_in_c=128, num_frame=180, num_joints=22, num_class=14, style='ST',
                           graph='graph.SHRE', graph_args=dict([('labeling_mode', 'spatial')]))
    assert type(net.gcn0).__module__ == "model.unit_agcn" and type(net.tcn0).__module__ == "model.net"
    A = torch.from_numpy(net.graph.A.astype(np.float32))
    kw = dict(attention=False, only_attention=False, tcn_attention=False, only_temporal_attention=False, relative=False,
              device=0, attention_3=False, dv=0.25, dk=0.25, Nh=8, num=4, dim_block1=10, dim_block2=30, dim_block3=75,
              num_point=22, weight_matrix=2, more_channels=False, drop_connect=True, starting_ch=64, all_layers=False,
              adjacency=False, data_normalization=True, visualization=False, skip_conn=True)
    u0, u1 = TCN_GCN_unit(64, 64, A.clone(), **kw), TCN_GCN_unit(64, 128, A.clone(), stride=2, **kw)
    doc = {"imports": imported_names(),
           "state_dicts": {"stem": layout(net.state_dict(), ("gcn0.", "tcn0.")),
                           "u0": layout(u0.state_dict()), "u1": layout(u1.state_dict())}}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
