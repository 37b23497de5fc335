"""The fused stem's narrow three-term kernel walks its runs in two store phases (csrc/kf6.h, ``v6_order``): a workgroup with bit 3
of its index set takes the first short tile of its run first and then the rest in order, so that half of every XCD's workgroups
store while the other half is in its main loop; and the short tile stores its whole 4-pixel groups as 16 bytes.  Neither may
move a bit: the tile partition, every tile's accumulation order and every stored value are those of the in-order walk.

Shapes (V = 22, bf16x3), the smallest at which the new order runs and can go wrong:
  * 600 clips of 24 frames: two full tiles and a 16-pixel short tile per clip, 1,800 tiles, runs of about seven tiles that start
    inside clips, in both classes (the prefetch chain then crosses from a short tile back to the run's first tile mid-clip);
  * 40 clips of 180 frames: 640 tiles, runs of two to three tiles, many without a short tile;
  * 3 clips of 24 frames: nine workgroups of one tile each, class 1 never occurs.
Each at both output layouts and with fp32 and bf16 results, held bit for bit to tests/golden/stem_store_phase_digests.json
(SHA-256, recorded from the sources of the commit before the two store phases by tools/make_stem_store_phase_digests.py); a
seeded handful of clips of each shape against the float64 CPU oracle at the gate of tests/test_gpu_parity.py for bf16x3
(``MATH_GATES``); and one case launched twice on two streams with different inputs, so that two launches' phases interleave."""
import importlib.util
import json
import os

import pytest
import torch

from _util import MATH_GATES, parity_gate
from test_stem_epilogue_paths import _seeded_stem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_stem_store_phase_digests", os.path.join(ROOT, "tools", "make_stem_store_phase_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(ROOT, "tests", "golden", "stem_store_phase_digests.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(want):
    assert set(want["digests"]) == {c["id"] for c in mk.cases()} | {c["id"] + "-x1" for c in mk.cases() if c["N"] == 600}


@pytest.mark.parametrize("case", mk.cases(), ids=lambda c: c["id"])
def test_result_bits_are_those_of_the_in_order_walk(case, want, dev):
    got = mk.digest(mk.run(case, dev))
    assert got == want["digests"][case["id"]], f"{case['id']}: {got[:16]} != recorded {want['digests'][case['id']][:16]} ({want['commit']})"


def test_two_launches_on_two_streams_keep_their_bits(want, dev):
    """Two launches with different inputs on two streams: the second one's workgroups start as the first one's end, both classes of
    both launches are on the chip at once.  Each result is the one its input gives alone."""
    case = next(c for c in mk.cases() if c["N"] == 600 and not c["flags"] and not c["out_bf16"])
    mk.operands(case, dev, 0), mk.operands(case, dev, 1)      # (on the device before the streams start)
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s0):
        z0 = mk.run(case, dev, 0)
    with torch.cuda.stream(s1):
        z1 = mk.run(case, dev, 1)
    torch.cuda.synchronize()
    assert mk.digest(z0) == want["digests"][case["id"]], "first stream"
    assert mk.digest(z1) == want["digests"][case["id"] + "-x1"], "second stream"


def _handful(N, T, V, dev):
    """Seeded clip indices of a shape: five drawn at random plus, where the launch has class-1 workgroups, the clips in which the
    runs of workgroups 8 and 15 begin."""
    import ctypes
    from stgcn_amd import _capi
    g = torch.Generator().manual_seed(N * 1009 + T)
    idx = set(torch.randperm(N, generator=g)[:5].tolist())
    tpc = -(-T * V // 256)
    G = min(N * tpc, torch.cuda.get_device_properties(dev).multi_processor_count)
    first, end = ctypes.c_int(), ctypes.c_int()
    for b in (8, 15):
        if b < G:
            assert _capi.lib().stgcn_stem_walk_run(b, G, N, tpc, 1, ctypes.byref(first), ctypes.byref(end)) == 0
            idx.add(first.value // tpc)
    return sorted(idx)


_refs = {}


@pytest.mark.parametrize("layout", ["nctv", "channels_last"])
@pytest.mark.parametrize("N,T,V", mk.SHAPES)
def test_a_handful_of_clips_against_the_oracle(N, T, V, layout, dev):
    from oracle import stgcn_oracle as so
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    gcn, tcn, gp, tp, gen = _seeded_stem(V, 7300 + N + T, dev)
    key = (N, T, V)
    if key not in _refs:                           # input and reference once per shape, left unchanged
        x = torch.randn(N, 3, T, V, generator=gen)
        idx = _handful(N, T, V, dev)
        _refs[key] = (x, idx, so.stem_forward(x[idx].double(), gp.to(torch.float64), tp.to(torch.float64)))
    x, idx, ref = _refs[key]
    set_math_mode(tcn, "bf16x3")
    enable_stem_fusion(gcn, tcn)
    if layout == "channels_last":
        set_output_layout(tcn, "channels_last")
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
    gate, strict = MATH_GATES["bf16x3"]
    err = parity_gate(z[idx], ref, gate, f"fused stem N={N} T={T} V={V} bf16x3 {layout}, clips {idx}", strict=strict)
    print(f"N={N} T={T} V={V} bf16x3 {layout}, clips {idx}: max|err|/max|ref| = {err:.2e}")
