"""CPU test of the fused stem's dispatch: the library's stem queries against tests/golden/stem_dispatch.json.

Which kernel serves a shape, and the prep-blob and workspace sizes that go with it, are host decisions; the fixture
(written by tests/golden/make_stem_dispatch.py) pins them row by row over a grid of flags and shapes.
"""
import json
import os

from _util import GOLDEN


def test_stem_queries_match_dispatch_fixture():
    from stgcn_amd import _capi
    lib = _capi.lib()
    with open(os.path.join(GOLDEN, "stem_dispatch.json")) as fh:
        fx = json.load(fh)
    assert fx["columns"] == ["flags", "Cin", "C", "T", "V", "K", "S", "supported", "kernel", "features", "prep_bytes",
                             "ws_bytes_n0", "ws_bytes_n1"]
    n0, n1 = fx["ws_n"]
    bad = []
    for row in fx["rows"]:
        f, cin, C, T, V, K, S = row[:7]
        fl = fx["flag_sets"][f]
        got = [f, cin, C, T, V, K, S,
               lib.stgcn_stem_supported(cin, C, T, V, K, S, fl),
               lib.stgcn_stem_kernel_name(cin, C, T, V, K, S, fl).decode(),
               lib.stgcn_stem_features_used(cin, C, T, V, K, S, fl),
               lib.stgcn_stem_prep_bytes(cin, C, K, S, fl),
               lib.stgcn_stem_ws_bytes(n0, cin, C, T, V, K, S, fl),
               lib.stgcn_stem_ws_bytes(n1, cin, C, T, V, K, S, fl)]
        if got != row:
            bad.append(f"want {row}\n      got  {got}")
    assert len(fx["rows"]) > 1000
    assert not bad, f"{len(bad)} of {len(fx['rows'])} rows differ:\n" + "\n".join(bad[:20])
