"""Host-side tests of the ST-TR spatial attention drop-in (gcn_unit_attention): layout, seeded init, refusals, C ABI
surface and the INTEGRATION.md §1 recipe for ``from model.ST_TR.gcn_attention import gcn_unit_attention``.  No GPU."""
import ctypes
import os
import re
import textwrap

import numpy as np
import pytest
import torch

import st_attention_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "st_attention_reference.npz")
CASES = {"v22_256_256": (22, 256, 256, 6), "v46_131_256": (46, 131, 256, 4), "v46_256_512": (46, 256, 512, 2),
         "v22_512_512": (22, 512, 512, 2)}
ABI_NAMES = ["stgcn_st_attention_supported", "stgcn_st_attention_ws_bytes", "stgcn_st_attention_forward",
             "stgcn_st_attention_forward_train", "stgcn_st_attention_backward"]


def _fixture():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _incidence(V):
    g = torch.Generator().manual_seed(V)
    return (torch.rand(3, V, V, generator=g) > 0.8).float()


def _unit(cin, cout, V, **over):
    from stgcn_amd import gcn_unit_attention
    kw = R.unit_kwargs(V)
    kw.update(over)
    return gcn_unit_attention(cin, cout, _incidence(V), **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_state_dict_layout_matches_reference(name):
    V, cin, cout, _ = CASES[name]
    z = _fixture()
    m = _unit(cin, cout, V)
    got = [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in m.state_dict().items()]
    assert got == list(z[f"{name}/layout"])
    m.load_state_dict(R.make_state(cin, cout, V, 1), strict=True)
    assert not hasattr(m, "A") and "incidence" not in dict(m.named_buffers())
    assert m.incidence.shape == (3, V, V) and m.attention_conv.A.shape == (V, V)
    assert m.attention_conv.dk == cout // 4 and m.attention_conv.dv == cout and m.attention_conv.Nh == 8


@pytest.mark.parametrize("name", sorted(CASES))
def test_seeded_init_equals_reference(name):
    V, cin, cout, _ = CASES[name]
    z = _fixture()
    torch.manual_seed(1234)
    m = _unit(cin, cout, V)
    for k, v in m.state_dict().items():
        a = v.double().numpy().reshape(-1)
        key = f"{name}/init/{k}"
        if key + "@idx" in z:
            np.testing.assert_array_equal(a[z[key + "@idx"]].astype(np.float32), z[key + "@val"], err_msg=key)
        else:
            np.testing.assert_array_equal(a.astype(z[key].dtype), z[key], err_msg=key)


@pytest.mark.parametrize("option,value", [("relative", True), ("adjacency", True), ("more_channels", True),
                                          ("only_attention", False), ("data_normalization", False)])
def test_unsupported_options_are_refused(option, value):
    with pytest.raises(NotImplementedError, match=option):
        _unit(64, 128, 22, **{option: value})


def test_cpu_input_is_refused():
    m = _unit(128, 128, 22)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 128, 4, 22))


def test_attention_abi_declared_and_exported():
    from stgcn_amd import _capi
    from stgcn_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    handle = ctypes.CDLL(build())
    for n in ABI_NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _capi.PROTOTYPES and hasattr(handle, n), n
    lib = _capi.lib()
    assert _capi.ABI_VERSION >= 9
    for cout in (128, 256, 512):
        assert lib.stgcn_st_attention_supported(131, cout, cout // 4, 46, 8) == 1
    assert lib.stgcn_st_attention_supported(64, 64, 16, 22, 8) == 0          # dvh = 8
    assert lib.stgcn_st_attention_supported(256, 256, 64, 65, 8) == 0        # V > 64
    assert lib.stgcn_st_attention_ws_bytes(32, 131, 256, 64, 300, 46, 8, 0) > 32 * 131 * 300 * 46 * 4
    assert lib.stgcn_st_attention_ws_bytes(0, 131, 256, 64, 300, 46, 8, 0) == 0
    rc = lib.stgcn_st_attention_forward(*([None] * 10), 0, None, 2, 64, 64, 16, 4, 22, 8, None)
    assert rc == -1 and b"NULL" in lib.stgcn_last_error()


CALLER = {
    "model/ST_TR/ST_TR_new.py": '''
        import torch.nn as nn

        from model.ST_TR.gcn_attention import gcn_unit_attention
        from model.net import Unit2D


        class TCN_GCN_unit(nn.Module):
            def __init__(self, in_channel, out_channel, A, num_point, stride=1):
                super().__init__()
                self.gcn1 = gcn_unit_attention(in_channel, out_channel, dv_factor=0.25, dk_factor=0.25, Nh=8, complete=True,
                                               relative=False, only_attention=True, layer=0, incidence=A, bn_flag=True,
                                               last_graph=False, more_channels=False, drop_connect=True, adjacency=False,
                                               num=4, data_normalization=True, skip_conn=True, visualization=False,
                                               num_point=num_point)
                self.tcn1 = Unit2D(out_channel, out_channel, kernel_size=9, stride=stride)
    ''',
    "model/ST_TR/spatial_transformer.py": "raise ImportError('the caller tree must not need this file')\n",
    "graph/__init__.py": "",
}


def test_integration_recipe_resolves_gcn_unit_attention(tmp_path):
    import test_dropin_recipe as rec
    caller = tmp_path / "caller"
    files = dict(rec.CALLER_FILES)                   # (the block imports the stem's caller too)
    files.update(CALLER)
    for rel, src in files.items():
        f = caller / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    out = rec._run("import sys\nsys.dont_write_bytecode = True\n" + rec._integration_block(str(caller)) + textwrap.dedent(f'''
        import torch
        from model.ST_TR.ST_TR_new import TCN_GCN_unit
        import model.ST_TR.gcn_attention as ga
        assert ga.__file__.startswith({rec.SHIM!r}), ga.__file__
        assert sys.modules["model.ST_TR.ST_TR_new"].__file__.startswith({str(caller)!r})
        u = TCN_GCN_unit(131, 256, torch.zeros(3, 46, 46), 46, stride=2)
        import stgcn_amd
        assert type(u.gcn1) is stgcn_amd.gcn_unit_attention and type(u.gcn1).__module__ == "stgcn_amd.st_attention"
        assert "attention_conv.qkv_conv.weight" in u.gcn1.state_dict()
        print("ATTN-RECIPE-OK")
    '''), tmp_path, "attn_recipe.py")
    assert "ATTN-RECIPE-OK" in out
