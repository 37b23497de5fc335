"""The fused stem's producer makes only the activation blocks that a tap of the tile reads: the three-term narrow kernel
starts at the block of the tile's first pixel (the image is frame-aligned, the tile is not) and runs seven blocks per wave
and chunk where no tile of the shape reads more than 28 blocks, eight from the image's first row otherwise.  A block that is
wrongly left out leaves the previous tile's rows under some tap, which misses parity grossly, so these shapes visit the edges
of that geometry: first pixels on both sides of row 16 of the image, tiles whose frame-aligned image has 28, 29 and fewer
blocks, single short tiles, the persistent walk (the rows left out then hold another tile's data), other joint counts on
either side of the rule, and two channel groups.  Reference: the CPU oracle in float64, at the gate of the other stem tests
(``MATH_GATES`` / ``parity_gate``); two launches on the same input must agree bit for bit."""
import pytest
import torch

from _util import MATH_GATES, parity_gate
from test_stem_epilogue_paths import _seeded_stem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


SHAPES = [
    (1, 180, 22, 128),    # one headline clip: 16 tiles, first pixel 0 .. 20 rows into the image (first block 0 and 1), images of 28 / 29 / 20 blocks
    (2, 38, 22, 128),     # full tiles plus a partial one
    (3, 37, 22, 128),     # ... and unaligned rows
    (70, 38, 22, 128),    # 280 tiles: the persistent walk, rows that are not produced hold the previous tile's data
    (1, 5, 22, 128),      # a single short tile
    (1, 12, 22, 128),     # a second tile of 8 pixels
    (2, 47, 21, 128),     # other joint counts on the seven-block form
    (2, 40, 20, 128),
    (1, 64, 16, 128),
    (3, 100, 8, 128),
    (2, 45, 23, 128),     # just outside it (a tile reads 29 / 30 blocks): eight blocks from the image's first row
    (2, 52, 25, 128),
    (2, 38, 22, 256),     # two channel groups, eight periods per tile
]

_cases = {}


def _case(N, T, V, C, dev):
    """Seeded stem (on the device, fp32 math, not fused yet), input and float64 oracle result of a shape; the reference is
    computed once per shape and left unchanged."""
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _seeded_stem(V, 5100 + N + T + V + C, dev, c=C)
    key = (N, T, V, C)
    if key not in _cases:
        x = torch.randn(N, 3, T, V, generator=gen)
        _cases[key] = (x, so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64)))
    return gcn, tcn, _cases[key][0], _cases[key][1]


@pytest.mark.parametrize("layout", ["nctv", "channels_last"])
@pytest.mark.parametrize("math", ["bf16x3", "bf16"])
@pytest.mark.parametrize("N,T,V,C", SHAPES)
def test_fused_stem_producer_blocks(N, T, V, C, math, layout, dev):
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    gcn, tcn, x, ref = _case(N, T, V, C, dev)
    set_math_mode(tcn, math)
    enable_stem_fusion(gcn, tcn)
    if layout == "channels_last":
        set_output_layout(tcn, "channels_last")
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
        z2 = tcn(gcn(x.to(dev)))
    assert z.shape == ref.shape
    gate, strict = MATH_GATES[math]
    err = parity_gate(z, ref, gate, f"fused stem N={N} T={T} V={V} C={C} {math} {layout}", strict=strict)
    print(f"N={N} T={T} V={V} C={C} {math} {layout}: max|err|/max|ref| = {err:.2e}")
    assert torch.equal(z, z2), "two launches on the same input differ"


@pytest.mark.parametrize("layout", ["nctv", "channels_last"])
def test_fused_stem_producer_blocks_bf16_output(layout, dev):
    """bf16 results (the second instantiation of each producer form) on one headline clip."""
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    gcn, tcn, x, ref = _case(1, 180, 22, 128, dev)
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
