"""tests/_util.py::skewed on the CPU: the address asked for, the values, strides and layout of the original, two poisoned
guard bands and a check that notices one changed byte on either side."""
import pytest
import torch

from _util import skewed


def _channels_last(x):
    return x.dim() == 4 and not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous()


@pytest.mark.parametrize("dtype,k", [(torch.float32, 1), (torch.float32, 2), (torch.float32, 3), (torch.bfloat16, 1),
                                     (torch.bfloat16, 2), (torch.bfloat16, 4)])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
def test_skewed_sits_where_asked_and_equals_the_original(dtype, k, layout):
    t = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(k)).to(dtype)
    if layout == "channels_last":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    s = skewed(t, k)
    assert s.data_ptr() % 16 == k * t.element_size() and s.data_ptr() % 256 == k * t.element_size()
    assert s.dtype == t.dtype and s.shape == t.shape and s.stride() == t.stride()
    assert s.is_contiguous() == t.is_contiguous() and _channels_last(s) == _channels_last(t)
    assert torch.equal(s, t) and s.data_ptr() != t.data_ptr()
    s.check()
    # the element either side is the fill, which reads as NaN in both types
    es = t.element_size()
    assert s.skew.hi - s.skew.lo == t.numel() * es and s.skew.lo >= 4096 and s.skew.raw.numel() - s.skew.hi >= 4096
    assert bool(torch.isnan(s.skew.raw[s.skew.lo - es:s.skew.lo].clone().view(dtype)).all())
    assert bool(torch.isnan(s.skew.raw[s.skew.hi:s.skew.hi + es].clone().view(dtype)).all())


@pytest.mark.parametrize("fill", [0xFF, 0x7F])
@pytest.mark.parametrize("at", ["just before", "just behind", "far before", "far behind"])
def test_check_reports_one_changed_guard_byte(fill, at):
    s = skewed(torch.arange(10, dtype=torch.float32), 1, fill=fill)
    raw, lo, hi = s.skew.raw, s.skew.lo, s.skew.hi
    s.check()
    raw[{"just before": lo - 1, "just behind": hi, "far before": 0, "far behind": raw.numel() - 1}[at]] = 0x01
    with pytest.raises(AssertionError, match="before" if "before" in at else "after"):
        s.check()
    assert torch.equal(s, torch.arange(10, dtype=torch.float32))


def test_writing_the_tensor_itself_leaves_the_guards():
    s = skewed(torch.zeros(3, 5, dtype=torch.bfloat16), 1)
    s.fill_(2.0)
    s.check()
    assert bool((s == 2).all())


def test_a_parameter_keeps_nothing_of_autograd():
    p = torch.nn.Parameter(torch.randn(4, 4))
    s = skewed(p, 3)
    assert not s.requires_grad and torch.equal(s, p.detach())
