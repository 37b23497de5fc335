"""The fused stem's tile tail has two forms, chosen once per tile: straight-line 16-byte stores for tiles that lie wholly
inside a clip with 16-byte aligned rows, and bounds-checked stores for a clip's last tile and for unaligned rows.  These
shapes make one launch take both (or only the checked one), walk more tiles than the chip has workgroups (the persistent
loop, with the next tile's x loads in flight behind the stores), and run single clips.  Reference: the CPU oracle in
float64, at the gate of the other stem tests (1e-4 of max|ref|, ``parity_gate``)."""
import pytest
import torch

from _util import MATH_GATES, parity_gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def _seeded_stem(V, seed, dev, c=128):
    """A 3 -> c -> c stem with random attention offsets, BatchNorm statistics and biases (so that the folded shift differs
    per channel), and its parameters in the oracle's form."""
    from stgcn_amd import Unit2D, unit_agcn
    from oracle import stgcn_oracle as so
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    A = torch.rand(3, V, V, generator=gen) * (torch.rand(3, V, V, generator=gen) < 0.15)
    gcn = unit_agcn(3, c, A.clone())
    tcn = Unit2D(c, c, kernel_size=9)
    with torch.no_grad():
        gcn.PA.data = torch.randn(3, V, V, generator=gen) * 0.05
        for m in list(gcn.modules()) + list(tcn.modules()):
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.2)
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 1.5 + 0.25)
            if isinstance(m, torch.nn.Conv2d):
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
        for cv in list(gcn.conv_a) + list(gcn.conv_b):
            cv.weight.mul_(3.0)
    gcn.A = A.clone()
    gp = so.agcn_params_from_state(gcn.state_dict(), gcn.A)
    tp = so.tcn_params_from_state(tcn.state_dict())
    return gcn.to(dev).eval(), tcn.to(dev).eval(), gp, tp, gen


SHAPES = [
    (2, 38, 22, 128),     # T*V = 836 = 3 full tiles + a partial one, rows aligned (836 % 4 == 0): both forms in one launch
    (3, 37, 22, 128),     # T*V = 814, 814 % 4 == 2: unaligned rows, every tile takes the checked form
    (2, 45, 22, 128),     # odd T: T*V = 990, 990 % 4 == 2
    (70, 38, 22, 128),    # 280 tiles: more than one per workgroup on 256 CUs, full and partial tiles mixed in each walk
    (1, 38, 22, 128),     # one clip: 4 workgroups
    (1, 180, 22, 128),    # one clip of the headline shape: 15 full tiles + a partial one
    (1, 64, 16, 128),     # T*V = 1024: every tile full and aligned, only the straight-line form
    (5, 52, 25, 128),     # V = 25: T*V = 1300 = 5 full tiles + a partial one, aligned
    (2, 38, 22, 256),     # two 128-channel groups (the second reads shift[128 ..]): full tiles + a partial one
    (2, 37, 22, 256),     # ... and unaligned rows
]


@pytest.mark.parametrize("layout", ["nctv", "channels_last"])
@pytest.mark.parametrize("math", ["bf16x3", "bf16"])
@pytest.mark.parametrize("N,T,V,C", SHAPES)
def test_fused_stem_full_and_checked_tiles(N, T, V, C, math, layout, dev):
    from stgcn_amd import enable_stem_fusion, set_math_mode, set_output_layout
    from oracle import stgcn_oracle as so
    gcn, tcn, gp, tp, gen = _seeded_stem(V, 4100 + N + T + V + C, dev, c=C)
    set_math_mode(tcn, math)
    enable_stem_fusion(gcn, tcn)
    if layout == "channels_last":
        set_output_layout(tcn, "channels_last")
    x = torch.randn(N, 3, T, V, generator=gen)
    ref = so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64))
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
        z2 = tcn(gcn(x.to(dev)))
    assert z.shape == ref.shape
    gate, strict = MATH_GATES[math]
    err = parity_gate(z, ref, gate, f"fused stem N={N} T={T} V={V} C={C} {math} {layout}", strict=strict)
    print(f"N={N} T={T} V={V} C={C} {math} {layout}: max|err|/max|ref| = {err:.2e}")
    assert torch.equal(z, z2), "two launches on the same input differ"


def test_fused_stem_bf16_output_both_forms(dev):
    """bf16 results: 8-byte stores in the straight-line form, element stores in the checked one."""
    from stgcn_amd import enable_stem_fusion, set_math_mode
    from oracle import stgcn_oracle as so
    N, T, V = 3, 38, 22
    gcn, tcn, gp, tp, gen = _seeded_stem(V, 4200, dev)
    set_math_mode(tcn, "bf16x3")
    tcn.out_bf16 = True
    enable_stem_fusion(gcn, tcn)
    x = torch.randn(N, 3, T, V, generator=gen)
    ref = so.stem_forward(x.double(), gp.to(torch.float64), tp.to(torch.float64))
    with torch.no_grad():
        z = tcn(gcn(x.to(dev)))
    assert z.dtype == torch.bfloat16
    # the result is the fp32 value rounded to bf16 (8 significant bits: half an ulp = 2^-9 relative)
    parity_gate(z.float(), ref, 2.0 ** -8, "bf16 output", strict=False)
