"""INTEGRATION.md §1 executed verbatim against a stand-in for the reference's caller files.

The recipe is about ``sys.path`` order and the ``model`` namespace package, which an already-imported ``model`` in the
pytest process would mask, so it runs in a subprocess.  Round-2 review: the recipe used to fail with ``No module named
'model.AltFormer'`` because the shim's ``model/`` was a regular package shadowing the reference's namespace package.

The reference tree is not part of this repository.  What the test needs of it is recorded as data in
``tests/golden/dropin_reference.json`` (tests/golden/make_golden_dropin.py, run against the reference): the names its files
import from ``model.net`` / ``model.unit_agcn``, and the state_dict layout (key, shape, dtype in order) of its
ST_GCN_AltFormer stem (constructor call of SHREC/ST_TS/train_sttran.py:75-82) and of two TCN_GCN_units
(model/ST_TR/ST_TR_new.py:285-372).  The caller side is a stand-in tree written into tmp_path with the reference's layout:
``model/`` and its sub-packages without ``__init__.py`` (namespace packages), ``graph/`` a regular package, callers that
import ``from model.net`` / ``from model.unit_agcn`` and build gcn0 / tcn0 and gcn1 / tcn1 / down1 from those names.
In the subprocess (shim first on sys.path, the python block of INTEGRATION.md §1 as it stands) the callers import, their
modules are ``stgcn_amd.modules`` classes, and state_dicts of the reference's layout load with ``strict=True``.
No forward runs (the HIP modules refuse CPU tensors).
"""
import json
import os
import re
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "st-gcn-altformer_amd")
FIXTURE = os.path.join(ROOT, "tests", "golden", "dropin_reference.json")

# the stand-in caller tree: file -> source (model/ and its sub-packages have no __init__.py, as in the reference)
CALLER_FILES = {
    "model/AltFormer/ST_GCN_AltFormer.py": '''
        import numpy as np
        import torch
        import torch.nn as nn

        from model.net import Unit2D, import_class
        from model.unit_agcn import unit_agcn


        class ST_GCN_AltFormer(nn.Module):
            def __init__(self, channel, backbone_in_c, graph=None, graph_args=dict(), **unused):
                super().__init__()
                self.graph = import_class(graph)(**graph_args)
                self.A = torch.from_numpy(self.graph.A.astype(np.float32))
                self.gcn0 = unit_agcn(channel, backbone_in_c, self.A)
                self.tcn0 = Unit2D(backbone_in_c, backbone_in_c, kernel_size=9)
    ''',
    "model/ST_TR/ST_TR_new.py": '''
        import torch.nn as nn

        from model.net import Unit2D
        from model.unit_agcn import unit_agcn


        class TCN_GCN_unit(nn.Module):
            def __init__(self, in_channel, out_channel, A, stride=1, **unused):
                super().__init__()
                self.gcn1 = unit_agcn(in_channel, out_channel, A)
                self.tcn1 = Unit2D(out_channel, out_channel, kernel_size=9, stride=stride)
                if in_channel != out_channel or stride != 1:
                    self.down1 = Unit2D(in_channel, out_channel, kernel_size=1, stride=stride)
                else:
                    self.down1 = None
    ''',
    "graph/__init__.py": "",            # a regular package on the caller's side too, without the graphs: the shim's wins
}

BUILD = textwrap.dedent('''
    import torch
    from model.AltFormer.ST_GCN_AltFormer import ST_GCN_AltFormer
    from model.ST_TR.ST_TR_new import TCN_GCN_unit
    import numpy as np
    torch.manual_seed(7)
    net = ST_GCN_AltFormer(channel=3, backbone_in_c=128, num_frame=180, num_joints=22, num_class=14, style='ST',
                           graph='graph.SHRE', graph_args=dict([('labeling_mode', 'spatial')]))   # train_sttran.py:75-82
    A = torch.from_numpy(net.graph.A.astype(np.float32))
    units = [TCN_GCN_unit(64, 64, A.clone()), TCN_GCN_unit(64, 128, A.clone(), stride=2)]
''')


def _write_caller_tree(tmp_path):
    caller = tmp_path / "caller"
    for rel, src in CALLER_FILES.items():
        f = caller / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    return str(caller)


def _run(code, tmp_path, name):
    f = tmp_path / name
    f.write_text(code)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, str(f)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{name} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def _integration_block(caller):
    """The first python block of INTEGRATION.md §1, with its two placeholder paths filled in."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text.split("## 1.", 1)[1]
    block = re.search(r"```python\n(.*?)```", sec, re.S).group(1)
    assert "/path/to/this/repo/st-gcn-altformer_amd" in block and "/path/to/ST-GCN-AltFormer" in block, \
        "INTEGRATION.md §1 no longer carries the two placeholder paths this test fills in"
    return block.replace("/path/to/this/repo/st-gcn-altformer_amd", SHIM).replace("/path/to/ST-GCN-AltFormer", caller)


def test_integration_recipe_imports_the_reference_callers(tmp_path):
    caller = _write_caller_tree(tmp_path)
    out = _run("import sys\nsys.dont_write_bytecode = True\n" + _integration_block(caller) + BUILD + textwrap.dedent(f'''
        import json
        import model, graph, stgcn_amd
        assert list(model.__path__)[0].startswith({SHIM!r}) and any(p.startswith({caller!r}) for p in model.__path__), model.__path__
        assert ST_GCN_AltFormer.__module__ == "model.AltFormer.ST_GCN_AltFormer"
        assert sys.modules[ST_GCN_AltFormer.__module__].__file__.startswith({caller!r})       # the caller's own file
        assert sys.modules["model.net"].__file__.startswith({SHIM!r})
        assert sys.modules["model.unit_agcn"].__file__.startswith({SHIM!r})
        assert graph.__file__.startswith({SHIM!r})
        for m in (net.gcn0, net.tcn0, units[0].gcn1, units[0].tcn1, units[1].gcn1, units[1].tcn1, units[1].down1):
            assert type(m).__module__ == "stgcn_amd.modules", type(m)
        assert type(net.graph).__module__ == "stgcn_amd.graphs"
        # the quirk travels with the drop-in: the caller's A reads 1e-6 after construction (model/unit_agcn.py:37-39)
        assert float(net.A.max()) == float(net.A.min()) == float(torch.tensor(1e-6))
        # state_dicts of the reference's layout (keys, shapes, dtypes in order; seeded values) load strictly
        ref = json.load(open({FIXTURE!r}))["state_dicts"]
        gen = torch.Generator().manual_seed(11)
        for mod, key in ((net, "stem"), (units[0], "u0"), (units[1], "u1")):
            want = [(k, tuple(shape), getattr(torch, dt)) for k, shape, dt in ref[key]]
            assert [(k, tuple(v.shape), v.dtype) for k, v in mod.state_dict().items()] == want, key   # same names, same order
            sd = {{k: (torch.randn(shape, generator=gen) if dt.is_floating_point else torch.randint(0, 9, shape, generator=gen)).to(dt)
                  for k, shape, dt in want}}
            mod.load_state_dict(sd, strict=True)
            assert all(torch.equal(mod.state_dict()[k], v) for k, v in sd.items())
        # the HIP modules refuse CPU tensors instead of computing something else
        try:
            net.gcn0(torch.zeros(1, 3, 8, 22))
        except RuntimeError as e:
            assert "GPU" in str(e)
        else:
            raise AssertionError("CPU input accepted")
        print("RECIPE-OK", len(sd))
    '''), tmp_path, "b_dropin.py")
    assert "RECIPE-OK" in out


def test_shim_exports_every_name_the_reference_imports():
    """Every ``from model.net import …`` / ``from model.unit_agcn import …`` line of the reference (names recorded in
    tests/golden/dropin_reference.json) resolves in the shim (ST_TR_new.py:8 imports ``conv_init`` from model.unit_agcn
    — the kaiming fan_out one, not model/net.py's)."""
    wanted = json.load(open(FIXTURE))["imports"]
    assert wanted["model.net"] and wanted["model.unit_agcn"]
    import importlib
    for modname, names in wanted.items():
        mod = importlib.import_module(modname)
        assert mod.__file__.startswith(SHIM)
        for n in names:
            assert hasattr(mod, n), f"{modname}.{n} missing from the drop-in"
    import torch
    from model.unit_agcn import conv_init as agcn_ci
    c = torch.nn.Conv1d(4, 6, 1)
    agcn_ci(c)
    assert float(c.bias.detach().abs().max()) == 0.0          # model/unit_agcn.py:12-14 zeroes the bias; model/net.py:60-65 does not
