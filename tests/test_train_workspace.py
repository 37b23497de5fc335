"""CPU test of the workspace sizes: every non-stem size query against tests/golden/train_workspace.json.

The Python wrappers allocate exactly what a `*_ws_bytes` query returns and the entry point carves its regions out of that
allocation, so the sizes are part of the library's contract.  The fixture (written by tests/golden/make_train_workspace.py)
pins them to the byte, row by row, over a grid that reaches every path of the training plans.
"""
import json
import os

from _util import GOLDEN


def test_size_queries_match_workspace_fixture():
    from stgcn_amd import _capi
    lib = _capi.lib()
    with open(os.path.join(GOLDEN, "train_workspace.json")) as fh:
        fx = json.load(fh)
    assert fx["sections"] == {
        "agcn_fwd": {"args": ["N", "Cin", "Cout", "T", "V", "S", "materialise"], "queries": ["stgcn_agcn_train_ws_bytes"]},
        "agcn_bwd": {"args": ["N", "Cin", "Cout", "T", "V", "S", "recompute"], "queries": ["stgcn_agcn_backward_ws_bytes"]},
        "tcn": {"args": ["N", "Cin", "Cout", "T", "V", "K", "stride", "flags"],
                "queries": ["stgcn_tcn_train_ws_bytes", "stgcn_tcn_backward_ws_bytes"]},
        "st_attention": {"args": ["N", "Cin", "Cout", "dk", "T", "V", "heads", "pass"], "queries": ["stgcn_st_attention_ws_bytes"]},
        "vit_block": {"args": ["B", "L", "D", "hidden"], "queries": ["stgcn_vit_block_ws_bytes"]},
    }
    bad, total = [], 0
    for section, sec in fx["sections"].items():
        n = len(sec["args"])
        for row in fx["rows"][section]:
            call = [fx["flag_sets"][a] if isinstance(a, str) else a for a in row[:n]]
            got = row[:n] + [getattr(lib, fn)(*call) for fn in sec["queries"]]
            if got != row:
                bad.append(f"{section}: want {row}\n      got  {got}")
        total += len(fx["rows"][section])
    assert total > 3000
    assert not bad, f"{len(bad)} of {total} rows differ:\n" + "\n".join(bad[:20])
