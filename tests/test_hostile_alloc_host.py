"""Host tests of tests/_util.py::hostile_allocations, run on the CPU allocator (``devices=("cpu",)``): the evidence that the GPU
tests of tests/test_buffer_discipline_gpu.py can fail.  Every call form stgcn_amd.functional uses comes back poisoned, shaped
and aligned; a single byte changed on either side of a buffer, next to it or at the far end of a guard, is reported with the
allocation named; the two torch functions are restored whichever way the block ends."""
import pytest
import torch

from _util import hostile_allocations

GUARD = 1 << 20
REAL = (torch.empty, torch.empty_like)
FILLS = [0xFF, 0x7F]


def _forms():
    """(what, call, shape, dtype): the ways functional.py reaches torch.empty / torch.empty_like."""
    like = torch.zeros(3, 5, dtype=torch.float32)
    last = torch.zeros(4, 6, 7)
    cl = torch.zeros(2, 4, 5, 3).permute(0, 3, 1, 2)            # (N,C,T,V) view of (N,T,V,C) memory: dense, not contiguous
    return [
        ("ints", lambda: torch.empty(2, 3, 5, 7, device="cpu", dtype=torch.float32), (2, 3, 5, 7), torch.float32),
        ("one int", lambda: torch.empty(1001, device="cpu", dtype=torch.uint8), (1001,), torch.uint8),
        ("tuple", lambda: torch.empty((4, 9, 11), device="cpu", dtype=torch.bfloat16), (4, 9, 11), torch.bfloat16),
        ("star tuple", lambda: torch.empty(*(3, 7), device="cpu", dtype=torch.float32), (3, 7), torch.float32),
        ("Size sum", lambda: torch.empty(last.shape[:-1] + (13,), device="cpu", dtype=torch.float32), (4, 6, 13), torch.float32),
        ("float64 words", lambda: torch.empty((12345 + 7) // 8, device="cpu", dtype=torch.float64), (1544,), torch.float64),
        ("kwargs dict", lambda: torch.empty(2, 5, **dict(device="cpu", dtype=torch.float32)), (2, 5), torch.float32),
        ("zero elements", lambda: torch.empty(0, device="cpu", dtype=torch.float32), (0,), torch.float32),
        ("zero in a shape", lambda: torch.empty(3, 0, 4, device="cpu", dtype=torch.float64), (3, 0, 4), torch.float64),
        ("default dtype", lambda: torch.empty(6, device="cpu"), (6,), torch.float32),
        ("empty_like", lambda: torch.empty_like(like), (3, 5), torch.float32),
        ("empty_like dtype=", lambda: torch.empty_like(like, dtype=torch.bfloat16), (3, 5), torch.bfloat16),
        ("empty_like dense view", lambda: torch.empty_like(cl), (2, 3, 4, 5), torch.float32),
    ]


@pytest.mark.parametrize("fill", FILLS)
def test_every_call_form_is_poisoned_shaped_and_aligned(fill):
    with hostile_allocations(fill, guard=GUARD, devices=("cpu",)) as h:
        for i, (what, call, shape, dtype) in enumerate(_forms()):
            t = call()
            assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cpu", what
            assert t.data_ptr() % 256 == 0, what
            raw, nbytes, rshape, rdtype = h.records[i]
            assert len(h.records) == i + 1 and (rshape, rdtype) == (shape, dtype), what
            assert raw.numel() == GUARD + nbytes + GUARD and (t.data_ptr() == raw.data_ptr() + GUARD or not t.numel()), what
            assert nbytes == t.numel() * t.element_size(), what
            if what == "empty_like dense view":
                assert t.stride() == (60, 1, 15, 3), "a dense view keeps its strides, as torch.empty_like does"
            else:
                assert t.is_contiguous(), what
            assert h.holds_only_fill(t), what
            if t.numel() and t.is_floating_point():
                assert torch.isnan(t).all() if fill == 0xFF else (torch.isfinite(t).all() and (t.double() > 1e38).all()), what
        h.check()
    assert (torch.empty, torch.empty_like) == REAL


def test_other_devices_and_method_forms_are_left_alone():
    with hostile_allocations(0xFF, guard=GUARD, devices=("cuda",)) as h:
        a = torch.empty(5, device="cpu")
        b = torch.empty_like(a)
        c = torch.empty(3, device="meta")
        assert not h.records and c.device.type == "meta" and b.shape == a.shape
    with hostile_allocations(0xFF, guard=GUARD, devices=("cpu",)) as h:
        x = torch.empty(4, device="cpu")
        x.new_empty(9)
        torch.zeros(7)
        assert len(h.records) == 1


def test_in_bounds_writes_leave_the_guards_alone():
    with hostile_allocations(0x7F, guard=GUARD, devices=("cpu",)) as h:
        a = torch.empty(129, 100, device="cpu", dtype=torch.float32)
        b = torch.empty(33, device="cpu", dtype=torch.bfloat16)
        a.fill_(1.5)
        b.fill_(-2.0)
        h.check()
        assert not h.holds_only_fill(a) and (a == 1.5).all() and (b == -2.0).all()


# the three deliberate one-byte overruns (immediately before, immediately after, the far end of a guard) on the SECOND of three
# allocations, so that naming "the right allocation" means something
@pytest.mark.parametrize("where,offset,text", [
    ("just before", lambda n: GUARD - 1, "byte at start-1 of"),
    ("just after", lambda n: GUARD + n, "byte at end+0 of"),
    ("far end of the lower guard", lambda n: 0, f"byte at start-{GUARD} of"),
    ("far end of the upper guard", lambda n: GUARD + n + GUARD - 1, f"byte at end+{GUARD - 1} of")])
@pytest.mark.parametrize("fill", FILLS)
def test_one_changed_guard_byte_is_reported_with_the_allocation_named(fill, where, offset, text):
    h = hostile_allocations(fill, guard=GUARD, devices=("cpu",))
    with pytest.raises(AssertionError) as e:
        with h:
            torch.empty(7, device="cpu", dtype=torch.float32)
            t = torch.empty(3, 11, device="cpu", dtype=torch.bfloat16)      # 66 bytes: the upper guard starts unrounded
            torch.empty(5, device="cpu", dtype=torch.float64)
            t.fill_(1.0)
            raw, nbytes = h.records[1][0], h.records[1][1]
            assert nbytes == 66
            raw[offset(nbytes)] = fill ^ 0x01                               # the exit check must see it
    msg = str(e.value)
    assert "allocation #1 " in msg and "(3, 11)" in msg and "torch.bfloat16" in msg and text in msg, msg
    assert (torch.empty, torch.empty_like) == REAL
    with pytest.raises(AssertionError, match="allocation #1 "):
        h.check()                                                           # and the method alone reports the same


def test_functions_are_restored_after_an_exception():
    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with hostile_allocations(0xFF, guard=GUARD, devices=("cpu",)):
            assert torch.empty is not REAL[0] and torch.empty_like is not REAL[1]
            raise Boom()
    assert (torch.empty, torch.empty_like) == REAL
    with hostile_allocations(0xFF, guard=GUARD, devices=("cpu",)):
        pass
    assert (torch.empty, torch.empty_like) == REAL


def test_guard_must_keep_the_alignment():
    with pytest.raises(AssertionError):
        hostile_allocations(0xFF, guard=1000)
