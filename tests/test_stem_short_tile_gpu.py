"""The fused stem's narrow three-term kernel gives a clip's last tile of at most 128 pixels a half-size form (a wave owns 32 pixels
instead of 64, five producer blocks per wave and chunk instead of seven or eight) and then walks the tiles in contiguous runs
balanced by cost instead of grid-stride.  A wrong pixel-to-wave map, a producer block left out or a run that skips or repeats a
tile misses parity grossly, so these shapes visit the edges of that rule: a clip that is one short tile, short tiles of exactly
128 and of 8 pixels, 129 pixels (just above the rule: the full form), a shape whose runs begin and end inside clips and behind
short tiles (rows that are not produced then hold another tile's data), two channel groups, and a joint count on the eight-block
side.  Reference: the CPU oracle in float64 at the gate of the other stem tests (``MATH_GATES`` / ``parity_gate``); two launches
on the same input must agree bit for bit.  Two of the shapes are also held to SHA-256 digests recorded from the library of the
commit before the short form existed (tests/golden/make_stem_short_tile_digests.py): it stores the same bits."""
import functools
import importlib.util
import json
import os

import pytest
import torch

from _util import MATH_GATES, parity_gate
from test_stem_epilogue_paths import _seeded_stem

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_stem_short_tile_digests", os.path.join(GOLDEN, "make_stem_short_tile_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


# (N, T, V, C, blocks the short form reads: 0 = the shape's last tile takes the full form)
SHAPES = [
    (1, 5, 22, 128, 18),      # a clip that is one short tile of 110 pixels
    (2, 17, 22, 128, 20),     # one full tile plus a short tile of 118 pixels
    (1, 8, 16, 128, 16),      # a short tile of exactly 128 pixels
    (3, 24, 16, 128, 16),     # 256 + 128 pixels
    (1, 43, 3, 128, 0),       # 129 valid pixels: just above the rule, the full form
    (2, 12, 22, 128, 13),     # a last tile of 8 pixels
    (1, 180, 22, 128, 20),    # one headline clip
    (300, 17, 22, 128, 20),   # 600 tiles, 900 cost units over 256 workgroups: runs begin and end inside clips and behind short tiles
    (2, 17, 22, 256, 0),      # two channel groups (at V = 22 they do not fit KF6's LDS budget: stem_bf16_v4_kernel serves the shape)
    (2, 17, 20, 256, 16),     # ... and on this kernel: a full tile plus a short one of 84 pixels, eight periods per tile
    (2, 17, 23, 128, 0),      # V = 23, a last tile of 135 pixels: the full form
    (2, 37, 24, 128, 20),     # the eight-block side of the producer rule (NPBW == 8) with a short last tile of 120 pixels
]


def _short_blocks(T, V, K=9):
    """The plan's rule in plain Python: blocks of 16 image rows from the short tile's first pixel to the last row a tap reads."""
    q0 = (T * V - 1) // 256 * 256
    npx, s = T * V - q0, q0 % V
    return ((s + npx - 1 + (K - 1) * V) >> 4) - (s >> 4) + 1 if npx <= 128 else 0


_cases = {}


def _case(N, T, V, C, dev):
    """Seeded stem (on the device, fp32 math, not fused yet), input and float64 oracle result of a shape; the reference is
    computed once per shape and left unchanged."""
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _seeded_stem(V, 6100 + N + T + V + C, dev, c=C)
    key = (N, T, V, C)
    if key not in _cases:
        x = torch.randn(N, 3, T, V, generator=gen)
        _cases[key] = (x, so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64)))
    return gcn, tcn, _cases[key][0], _cases[key][1]


@pytest.mark.parametrize("N,T,V,C,blocks", SHAPES)
def test_the_plan_takes_the_short_form_where_the_table_says(N, T, V, C, blocks, dev):
    from stgcn_amd import _capi
    served = _capi.lib().stgcn_stem_kernel_name(3, C, T, V, 9, 3, 1).decode() == "stem_bf16_v6_kernel"
    assert served or (C, V) in ((256, 22), (128, 23))      # (those two: stem_bf16_v4_kernel; the oracle holds them all the same)
    assert (_short_blocks(T, V) if served else 0) == blocks
    assert _capi.lib().stgcn_stem_short_tile_blocks(C, T, V, 9) == blocks


@pytest.mark.parametrize("layout", ["nctv", "channels_last"])
@pytest.mark.parametrize("N,T,V,C,blocks", SHAPES)
def test_fused_stem_short_tile(N, T, V, C, blocks, layout, dev):
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    gcn, tcn, x, ref = _case(N, T, V, C, dev)
    set_math_mode(tcn, "bf16x3")
    enable_stem_fusion(gcn, tcn)
    if layout == "channels_last":
        set_output_layout(tcn, "channels_last")
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
        z2 = tcn(gcn(x.to(dev)))
    assert z.shape == ref.shape
    gate, strict = MATH_GATES["bf16x3"]
    err = parity_gate(z, ref, gate, f"fused stem N={N} T={T} V={V} C={C} bf16x3 {layout}", strict=strict)
    print(f"N={N} T={T} V={V} C={C} bf16x3 {layout}: max|err|/max|ref| = {err:.2e}")
    assert torch.equal(z, z2), "two launches on the same input differ"


@pytest.mark.parametrize("layout", ["nctv", "channels_last"])
def test_fused_stem_short_tile_bf16_output(layout, dev):
    """bf16 results (the second instantiation of each form) on a full tile plus a short one."""
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    gcn, tcn, x, ref = _case(2, 17, 22, 128, dev)
    set_math_mode(tcn, "bf16x3")
    tcn.out_bf16 = True
    enable_stem_fusion(gcn, tcn)
    if layout == "channels_last":
        set_output_layout(tcn, "channels_last")
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
        z2 = tcn(gcn(x.to(dev)))
    assert z.dtype == torch.bfloat16
    # the result is the fp32 value rounded to bf16 (8 significant bits: half an ulp = 2^-9 relative)
    parity_gate(z.float(), ref, 2.0 ** -8, f"bf16 output {layout}", strict=False)
    assert torch.equal(z, z2), "two launches on the same input differ"


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "stem_short_tile_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", mk.cases(), ids=lambda c: c["id"])
def test_result_bits_are_those_of_the_full_form(case, want, dev):
    """The short form and the balanced walk keep every element's accumulation order: the bits the all-full-tile, grid-stride
    kernel of the fixture's commit stored."""
    assert set(want["digests"]) == {c["id"] for c in mk.cases()}
    got = mk.digest(mk.run(case, dev))
    assert got == want["digests"][case["id"]], f"{case['id']}: {got[:16]} != recorded {want['digests'][case['id']][:16]} ({want['commit']})"


@pytest.mark.parametrize("index,value", [((1, 0, 14, 5), "nan"), ((0, 2, 16, 21), "+inf")])
def test_a_non_finite_pixel_inside_a_short_tile(index, value, dev):
    """One NaN and one Inf input pixel among the 118 pixels of a short tile (frames 12 .. 16 of a 17 x 22 clip are pixels 264 ..
    373): the conditions of tests/nonfinite_cases.py — non-finite wherever the oracle's result of the planted input is."""
    import nonfinite_cases as nc
    shape = (2, 17, 22, 128)
    assert index[2] * 22 + index[3] >= 256 and _short_blocks(17, 22) > 0
    case = nc.Case("stem_fused-short_tile-2x17x22x128-bf16x3", functools.partial(nc.prepare_stem_fused, shape, "bf16x3"), "bf16x3")
    prep = case.prepare()
    run = prep.on(dev)
    xp = nc.plant(prep.x, index, value)
    nc.check(case, prep, index, value, run(xp), prep.reference(xp), f"{case.id} {value}@{index}")
