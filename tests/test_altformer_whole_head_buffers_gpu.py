"""The whole-head entry points under poisoned, guard-banded buffers (``hostile_allocations`` of tests/_util.py, as
tests/test_buffer_discipline_gpu.py uses it): ``vit_pool``, ``vit_pool_classify`` and the small whole head read nothing they
did not write and write nothing outside their buffers, under both fills; and a workspace eight bytes short is refused before
anything is launched.  A file of its own without graph capture: the allocation patch is process-wide."""
import pytest
import torch
import torch.nn.functional as TF

from _util import MATH_GATES, hostile_allocations, parity_gate
from test_altformer_gpu import small_head

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
FILLS = (0xFF, 0x7F)          # NaN in fp32 / fp64; a huge finite positive number that would win a maximum


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def under_both_fills(run, want, rel, what, strict=True):
    """``run()`` -> tensor, twice per fill: guards intact, finite, inside the gate, the two runs equal."""
    for fill in FILLS:
        with hostile_allocations(fill) as h:
            a = run()
            b = run()
            torch.cuda.synchronize()
            h.check()
        assert h.records, f"{what}: no allocation went through torch.empty - the case would test nothing"
        assert torch.isfinite(a).all(), f"{what} fill=0x{fill:02X}: non-finite output"
        parity_gate(a, want, rel, f"{what} fill=0x{fill:02X}", strict=strict)
        assert torch.equal(a, b), f"{what} fill=0x{fill:02X}: two runs differ"


@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("shape", [(22, 180, 256), (1030, 22, 256), (5, 3, 100)], ids=lambda s: "x".join(map(str, s)))
def test_pool(shape, mode, dev):
    from stgcn_amd import functional as F
    g = torch.Generator().manual_seed(3)
    x = -(0.5 + torch.rand(*shape, generator=g))
    want = x.double().max(dim=1).values if mode == "max" else x.double().mean(dim=1)
    xd = x.to(dev)
    under_both_fills(lambda: F.vit_pool(xd, mode), want, REL, f"vit_pool {shape} {mode}")
    if mode == "max":
        with hostile_allocations(0x7F):
            assert torch.equal(F.vit_pool(xd, "max").cpu(), x.max(dim=1).values)


@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("NLD", [(1, 180, 512), (5, 22, 512), (3, 7, 192)], ids=lambda s: "x".join(map(str, s)))
def test_pool_classify(NLD, mode, dev):
    from stgcn_amd import functional as F
    N, L, D = NLD
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, L, D, generator=g) - 1.0
    lw, lb = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, b = (torch.rand(14, D, generator=g) * 2 - 1) / D ** 0.5, torch.randn(14, generator=g)
    pooled = x.double().max(dim=1).values if mode == "max" else x.double().mean(dim=1)
    want = TF.layer_norm(pooled, (D,), lw.double(), lb.double(), 1e-5) @ W.double().T + b.double()
    xd, lwd, lbd, Wd, bd = (t.to(dev) for t in (x, lw, lb, W, b))
    under_both_fills(lambda: F.vit_pool_classify(xd, lwd, lbd, 1e-5, Wd, bd, mode=mode), want, REL, f"vit_pool_classify {NLD} {mode}")


@pytest.mark.parametrize("cls_name", ["ST", "TS"])
def test_small_whole_head(cls_name, dev):
    import stgcn_amd
    head = small_head(dev, cls_name)
    z = torch.relu(torch.randn(3, 128, 40, 22, generator=torch.Generator().manual_seed(5))).to(dev)
    with torch.no_grad():
        want = head(z)                                    # the per-block path, ordinary allocations
        stgcn_amd.set_whole_head(head)
        assert head.runs_whole(z)
        under_both_fills(lambda: head(z), want, REL, f"whole head {cls_name}")


def test_eight_bytes_short_is_refused_before_anything_is_launched(dev, monkeypatch):
    import stgcn_amd
    from stgcn_amd import StgcnError, _capi
    from stgcn_amd import functional as F
    head = small_head(dev, "ST")
    stgcn_amd.set_whole_head(head)
    z = torch.relu(torch.randn(2, 128, 40, 22, generator=torch.Generator().manual_seed(6))).to(dev)
    with torch.no_grad():
        plan = head._whole_plan(z)
    assert plan is not None
    logits = torch.full((2, 14), 7.5, device=dev)
    torch.cuda.synchronize()
    lib = _capi.lib()
    real = lib.stgcn_altformer_head_ws_bytes
    asked = []

    def eight_short(*args):
        asked.append(real(*args))
        assert asked[-1] >= 8
        return asked[-1] - 8

    monkeypatch.setattr(lib, "stgcn_altformer_head_ws_bytes", eight_short)
    with hostile_allocations(0xFF) as h:
        with pytest.raises(StgcnError) as e:
            F.altformer_head_forward(z, logits=logits, **plan)
        torch.cuda.synchronize()
        assert asked and e.value.code == -3 and "STGCN_ERR_WORKSPACE" in str(e.value), e.value
        h.check()
        assert h.records
        for i, (raw, nbytes, shape, dtype) in enumerate(h.records):
            assert bool((raw == h.fill).all()), f"allocation #{i} (shape {shape}, {dtype}) was written by a refused call"
    assert bool((logits == 7.5).all()), "the pre-filled logits were written by a refused call"
