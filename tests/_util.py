"""Shared helpers for the tests: golden loading, the parity and gradient gates, the hostile allocator and the run under it."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sub_state(g, prefix):
    """state_dict (torch tensors) of the keys that start with ``prefix``."""
    return {k[len(prefix):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(prefix)}


# arithmetic modes of the temporal-conv contraction and their gates:
#   f32 / f32_valu / bf16x3 : the fp32 contract of north_star — 1e-4 relative (both criteria below)
#   bf16                    : operands rounded to bf16; documented looser bound 1e-2*max|ref| (max-norm only)
#   f16mx                   : fused stem only (STGCN_STEM_F16MX, opt-in): fp16 x fp16 + two scaled-e4m3 residual products —
#                             inside north_star's 1e-4*max|ref| (measured 2e-5, tools/math_error_2term.py) but NOT inside the
#                             mixed allclose criterion (its error on near-zero outputs is ~2e-5*max|ref| > atol): max-norm only
MATH_GATES = {"f32": (1e-4, True), "f32_valu": (1e-4, True), "bf16x3": (1e-4, True), "bf16": (1e-2, False), "f16mx": (1e-4, False)}


def parity_gate(out, ref, rel=1e-4, what="", strict=True):
    """SURVEY §8(d) gate for fp32: max|out-ref| <= rel*max|ref| and allclose(rtol=rel, atol=rel/10*max|ref|)."""
    out = torch.as_tensor(out).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    scale = ref.abs().max().item()
    err = (out - ref).abs().max().item()
    assert err <= rel * max(scale, 1e-30), f"{what}: max abs err {err:.3e} > {rel:g} * max|ref| ({scale:.3e})"
    if strict:
        assert torch.allclose(out, ref, rtol=rel, atol=rel * 0.1 * scale), f"{what}: allclose(rtol={rel}) failed"
    return err / max(scale, 1e-30)


def gather_flat(t, idx):
    return torch.as_tensor(t).reshape(-1)[torch.as_tensor(idx)]


def grad_gate(got, ref, rel, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite gradient"
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert err <= rel * max(scale, 1e-30), f"{what}: max abs err {err:.3e} > {rel:g} * max|ref| ({scale:.3e})"


def kink_free_cotangent(y_ref, gen):
    """Random dL/dy that is zero where the reference output sits within 1e-4*max of the ReLU kink.  The gradient is
    discontinuous there: an output of 1e-6 that the fp32 path rounds to 0 flips one mask bit and moves dbeta of its
    channel by a whole |dL/dy| — a property of ReLU, not an arithmetic error — so those outputs carry no cotangent."""
    G = torch.randn(y_ref.shape, generator=gen)
    return G * (y_ref.detach() > 1e-4 * y_ref.detach().abs().max()).float()


class hostile_allocations:
    """While active, ``torch.empty`` / ``torch.empty_like`` (the module attributes: every allocation of
    stgcn_amd.functional) hand out poisoned, guard-banded memory on the listed device types.

    A request of ``nbytes`` becomes ``guard + nbytes + guard`` bytes of uint8 filled with the byte ``fill``; the caller gets the
    middle as a view of the dtype and shape it asked for, the upper guard starting at the first byte behind it.  ``check()``
    (also run on a clean exit) asserts that every guard byte of every allocation made so far still holds ``fill``.

    ``fill`` is a condition, not a measurement: 0xFF reads as NaN in fp32, fp64 and bf16 (a result that depends on what a
    buffer held before turns non-finite), 0x7F as a huge finite positive number (3.4e38 / 1.4e306 / 3.4e38) that wins a
    ``max`` or a compare-and-select, where the hardware drops a NaN.  Method forms (``x.new_empty``) are left alone; the
    patch is process-wide, so nothing else may allocate from another thread meanwhile."""

    ALIGN = 256

    def __init__(self, fill, guard=1 << 20, devices=("cuda",)):
        assert 0 <= fill <= 0xFF and guard > 0 and guard % 512 == 0, "guard: a positive multiple of 512 (keeps the 256-byte alignment)"
        self.fill, self.guard, self.devices = fill, guard, tuple(devices)
        self.records = []                 # (backing uint8 tensor, nbytes, shape, dtype) in order of creation
        self._real = None

    # -- the two replacements -------------------------------------------------------------------------------------------------
    def _guarded(self, shape, dtype, device, strides=None):
        real_empty = self._real[0]
        dtype = dtype or torch.get_default_dtype()
        shape = tuple(int(s) for s in shape)
        item = real_empty((), dtype=dtype).element_size()
        nbytes = math.prod(shape) * item
        raw = real_empty(self.guard + nbytes + self.guard, dtype=torch.uint8, device=device)
        if (raw.data_ptr() + self.guard) % self.ALIGN and raw.device.type == "cpu":
            # the host allocator aligns to 64 bytes only: take the aligned window of a slightly larger block
            raw = real_empty(raw.numel() + self.ALIGN, dtype=torch.uint8, device=device)
            off = -(raw.data_ptr() + self.guard) % self.ALIGN
            raw = raw[off:off + self.guard + nbytes + self.guard]
        raw.fill_(self.fill)
        mid = raw[self.guard:self.guard + nbytes].view(dtype)
        out = mid.view(shape) if strides is None else mid.as_strided(shape, strides)
        assert out.data_ptr() % self.ALIGN == 0, f"guarded allocation {len(self.records)} is not {self.ALIGN}-byte aligned"
        assert out.data_ptr() == raw.data_ptr() + self.guard or nbytes == 0       # (torch reports no address for zero elements)
        self.records.append((raw, nbytes, shape, dtype))
        return out

    @staticmethod
    def _dense(t):
        expect = 1
        for size, stride in sorted(zip(t.shape, t.stride()), key=lambda p: p[1]):
            if size != 1 and stride != expect:
                return False
            expect *= size
        return t.numel() > 0

    def _wants(self, device):
        return torch.device(device if device is not None else "cpu").type in self.devices

    def _empty(self, *size, dtype=None, device=None, **kw):
        if not self._wants(device) or kw.get("out") is not None or kw.get("layout", torch.strided) is not torch.strided \
                or kw.get("memory_format", torch.contiguous_format) is not torch.contiguous_format:
            return self._real[0](*size, dtype=dtype, device=device, **kw)
        if "size" in kw:
            size = (kw.pop("size"),)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])                      # a tuple, a list or a torch.Size (also a sum of them)
        out = self._guarded(size, dtype, device)
        return out.requires_grad_() if kw.get("requires_grad") else out

    def _empty_like(self, t, *, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        fmt = kw.get("memory_format", torch.preserve_format)
        if not self._wants(device) or kw.get("layout", torch.strided) is not torch.strided \
                or fmt not in (torch.preserve_format, torch.contiguous_format):
            return self._real[1](t, dtype=dtype, device=device, **kw)
        # preserve_format: a dense, non-overlapping tensor keeps its strides (torch's own rule), anything else is contiguous
        strides = t.stride() if fmt is torch.preserve_format and not t.is_contiguous() and self._dense(t) else None
        out = self._guarded(t.shape, dtype or t.dtype, device, strides)
        return out.requires_grad_() if kw.get("requires_grad") else out

    # -- the checks --------------------------------------------------------------------------------------------------------------
    def check(self):
        """Every guard byte of every allocation made so far still holds the fill."""
        for i, (raw, nbytes, shape, dtype) in enumerate(self.records):
            for lo, hi, side in ((0, self.guard, "before"), (self.guard + nbytes, raw.numel(), "after")):
                bad = raw[lo:hi] != self.fill
                if bool(bad.any()):
                    at = lo + int(bad.to(torch.uint8).argmax())
                    where = f"at start-{self.guard - at}" if side == "before" else f"at end+{at - self.guard - nbytes}"
                    raise AssertionError(f"guard overwritten: allocation #{i} (shape {shape}, {dtype}, {nbytes} bytes), first changed "
                                         f"byte {where} of the buffer (value 0x{int(raw[at]):02X}, fill 0x{self.fill:02X})")

    def holds_only_fill(self, t):
        """True if every byte of ``t`` (a tensor handed out here, still dense) is the fill: nothing was written to it."""
        return bool((t.contiguous().reshape(-1).view(torch.uint8) == self.fill).all())

    def __enter__(self):
        assert self._real is None, "hostile_allocations is not re-entrant"
        self._real = (torch.empty, torch.empty_like)
        torch.empty, torch.empty_like = self._empty, self._empty_like
        return self

    def __exit__(self, exc_type, exc, tb):
        torch.empty, torch.empty_like = self._real
        self._real = None
        if exc_type is None:
            self.check()
        return False


# ---- an operand off its allocation's alignment -------------------------------------------------------------------------------------
class Skewed:
    """What ``skewed`` keeps of one tensor: the backing bytes, where the tensor's bytes sit in them and the fill."""

    def __init__(self, raw, lo, hi, fill):
        self.raw, self.lo, self.hi, self.fill = raw, lo, hi, fill

    def check(self):
        """Both guard bands still hold nothing but the fill."""
        for a, b, side in ((0, self.lo, "before"), (self.hi, self.raw.numel(), "after")):
            bad = self.raw[a:b] != self.fill
            if bool(bad.any()):
                at = a + int(bad.to(torch.uint8).argmax())
                where = f"start-{self.lo - at}" if side == "before" else f"end+{at - self.hi}"
                raise AssertionError(f"guard of a skewed tensor overwritten {side} it: first changed byte at {where} "
                                     f"(value 0x{int(self.raw[at]):02X}, fill 0x{self.fill:02X})")


def skewed(t, k, fill=0xFF, guard=4096):
    """A tensor equal to ``t`` - same shape, dtype, device and dense strides (contiguous stays contiguous, channels-last stays
    channels-last) - whose first byte sits ``k`` elements behind a 256-byte boundary, between two guard bands of ``guard``
    bytes filled with the byte ``fill`` (0xFF: NaN in fp32 and bf16).  ``.skew.check()`` of the result asserts that both
    guards still hold the fill: a kernel that rounds the address down, or stores a vector where the row is not, writes there
    or reads a NaN from there.  Works on the CPU (the allocation is windowed to a 256-byte boundary) as on the GPU."""
    assert t.numel() > 0 and hostile_allocations._dense(t), "skewed: a dense, non-empty tensor"
    assert 0 <= fill <= 0xFF and guard > 0 and guard % 256 == 0 and 0 <= k * t.element_size() < 256
    nbytes = t.numel() * t.element_size()
    raw = torch.empty(guard + 256 + nbytes + guard + 256, dtype=torch.uint8, device=t.device)
    off = -(raw.data_ptr() + guard) % 256                    # the first byte behind the lower guard: on a 256-byte boundary
    lo = off + guard + k * t.element_size()
    raw = raw[off:lo + nbytes + guard]
    raw.fill_(fill)
    out = raw[lo - off:lo - off + nbytes].view(t.dtype).as_strided(t.shape, t.stride())
    out.copy_(t.detach())
    assert (out.data_ptr() - k * t.element_size()) % 256 == 0 and out.stride() == t.stride()
    out.skew = Skewed(raw, lo - off, lo - off + nbytes, fill)
    out.check = out.skew.check
    return out


# ---- a run under the hostile allocator --------------------------------------------------------------------------------------------
FILLS =(0xFF, 0x7F)          # NaN in fp32 / fp64 / bf16; a huge finite positive number in all three


class HostileCase:
    """``make(dev)`` prepares inputs and references OUTSIDE the hostile block and returns ``(run, gate)``: ``run()`` calls the
    entry point(s) and returns {name: output tensor}, ``gate(outputs)`` holds them to the existing test's reference and gate.
    ``bitwise``: the outputs of the two runs must be identical."""

    def __init__(self, id, make, bitwise):
        self.id, self.make, self.bitwise = id, make, bitwise


def _finite(out, what):
    for k, t in out.items():
        if t is not None and t.is_floating_point():
            assert torch.isfinite(t).all(), f"{what}: {k} is not finite under poisoned buffers"


def run_under_both_fills(case, dev):
    run, gate = case.make(dev)
    outs = []
    for fill in FILLS:
        with hostile_allocations(fill) as h:
            out = run()
            torch.cuda.synchronize()
            h.check()
        assert h.records, f"{case.id}: no allocation went through torch.empty - the case would test nothing"
        what = f"{case.id} fill=0x{fill:02X}"
        _finite(out, what)
        gate(out, what)
        outs.append(out)
    if case.bitwise:
        for k in outs[0]:
            a, b = outs[0][k], outs[1][k]
            assert (a is None) == (b is None), k
            assert a is None or torch.equal(a, b), f"{case.id}: {k} differs between the NaN-filled and the huge-filled run"


ZERO_GRAD = ("attention_conv.attn_out.bias",)     # gcn_unit_attention: analytically 0 behind a batch-statistics BatchNorm


def st_attention_train_gate(yr, g, dx, frozen):
    """The gate of a gcn_unit_attention training step {"y", "dx", "d" + parameter name} against grads64's (yr, g, dx)."""
    def gate(o, what):
        parity_gate(o["y"], yr, what=f"{what} y")
        for k in g:
            if k in ZERO_GRAD and not frozen:
                assert float(o["d" + k].abs().max()) <= 1e-4 * float(g["bn.bias"].abs().max()), f"{what} d{k}"
            else:
                parity_gate(o["d" + k], g[k], strict=False, what=f"{what} grad {k}")
        parity_gate(o["dx"], dx, strict=False, what=f"{what} dx")
    return gate
