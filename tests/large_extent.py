"""Large extents: the tiled batch and its gate (tests/test_large_extent_gpu.py, tests/test_large_extent_host.py).

A result of more than 2^31 elements has no affordable fp64 reference - and needs none.  A batch of ``n0`` clips (or sequences,
or row groups: the unit along axis 0) is made from a seed and restated in fp64 on the CPU as the entry point's own test does;
the entry point then runs on ``x0.repeat(R, 1, ...)``.  In eval mode clips are independent: clip ``n`` of the result must equal
reference clip ``n % n0``.  In training mode the batch statistics of the tiled batch are those of the small one, so outputs and
dx are periodic in the same way and the parameter gradients are ``R`` times the small batch's.  ``gate_tiled`` holds EVERY element
of the large result to the small reference, on the device, in fp64, a chunk at a time.  A store whose offset wrapped at 2^31 or
2^32 bytes or at 2^31 elements lands on other data, as long as none of those thresholds is a multiple of the clip or of the period
(``aliasing_thresholds`` names the ones that are).

A plain module: it imports no test module and needs a GPU only where a function is handed a device tensor."""
import gc

import pytest
import torch

GIB = 1 << 30
CHUNK = 1 << 27                 # elements of one compared piece: 1 GiB of doubles per temporary
GATE_BYTES = 6 * GIB            # what gate_tiled holds at its peak: the piece and the reference as doubles, index, difference, mask
HEADROOM = 2 * GIB
MAX_NEED = 48 * GIB
N0 = 7                          # clips of the small batch: coprime to every power of two
# elements at which a hand-written offset can wrap: 2^31 bytes of fp32, 2^32 bytes of fp32 (2^31 of bf16), 2^31 elements (2^32
# bytes of bf16)
THRESHOLDS = {torch.float32: (1 << 29, 1 << 30, 1 << 31), torch.bfloat16: (1 << 30, 1 << 31)}


def aliasing_thresholds(clip_elems, n0, dtype=torch.float32):
    """The thresholds that are a multiple of one clip or of the period ``n0 * clip``: a wrap by one of them would land on the
    same (clip mod n0, offset in the clip) and the tiled batch could not see it.  Empty = the shape meets the condition."""
    return [t for t in THRESHOLDS[dtype] if t % clip_elems == 0 or t % (n0 * clip_elems) == 0]


def tiles_past(limit, clip_elems, n0=N0):
    """The fewest copies of an ``n0``-clip batch whose result holds more than ``limit`` elements."""
    return limit // (n0 * clip_elems) + 1


class Extent:
    """The extent of one row of a table: ``N`` units (clips, sequences, row groups) of ``unit`` result elements each, the result
    stored as ``dtype``, the small batch of ``n0`` units.  ``named``: (name, elements) of the tensor the row is about where that is
    not the result (a block's hidden activation, which exists a slab at a time only)."""

    def __init__(self, N, unit, dtype=torch.float32, n0=N0, named=None):
        self.N, self.unit, self.dtype, self.n0 = N, tuple(unit), dtype, n0
        self.R = -(-N // n0)
        self.clip = 1
        for d in self.unit:
            self.clip *= d
        self.result = N * self.clip
        self.named = named or ("result", self.result)

    @classmethod
    def past(cls, unit, dtype=torch.float32, n0=N0, limit=1 << 31, named_per_unit=None):
        """The smallest whole number of tilings whose result (or named tensor, ``named_per_unit`` = (name, elements per unit))
        has more than ``limit`` elements."""
        clip = 1
        for d in unit:
            clip *= d
        N = n0 * tiles_past(limit, named_per_unit[1] if named_per_unit else clip, n0)
        return cls(N, unit, dtype, n0, (named_per_unit[0], N * named_per_unit[1]) if named_per_unit else None)

    def bytes(self, elems_per_unit=None, itemsize=None):
        return self.N * (self.clip if elems_per_unit is None else elems_per_unit) * \
            (itemsize or torch.empty((), dtype=self.dtype).element_size())

    def assert_large_and_alias_free(self, what):
        assert self.N % self.n0 == 0, f"{what}: {self.N} units are no whole number of {self.n0}-unit batches"
        assert self.named[1] > 1 << 31, f"{what}: {self.named[0]} has {self.named[1]} elements, not more than 2^31"
        bad = aliasing_thresholds(self.clip, self.n0, self.dtype)
        assert not bad, f"{what}: a wrap by {bad} elements lands on the same (unit mod {self.n0}, offset): unit of {self.clip} elements"


def tiled(setup, R, dev=None, n=None):
    """-> (the input of ``R`` copies of the setup's small batch - of its first ``n`` clips, if given - and the fp64 reference of
    the small batch).  The small batch is uploaded and repeated on the device; the large input never exists on the host."""
    ref = setup.reference(setup.x)
    x0 = setup.x.to(dev) if dev is not None else setup.x
    xt = x0.repeat(R, *([1] * (x0.dim() - 1)))
    return (xt if n is None else xt[:n].contiguous()), ref


def _fmt_threshold(flat, itemsize):
    past = [f"2^{b} elements" for b in (29, 30, 31, 32) if flat >= 1 << b]
    past_b = [f"2^{b} bytes" for b in (31, 32, 33) if flat * itemsize >= 1 << b]
    return f"flat index {flat} (byte {flat * itemsize}); past " + (", ".join(past[-1:] + past_b[-1:]) or "no threshold")


def gate_tiled(out, ref_small, rel, strict, what, chunk=CHUNK):
    """_util.parity_gate's two criteria for ``out`` (N, ...) against ``ref_small`` (n0, ...) repeated along axis 0, evaluated
    where ``out`` lives, in fp64, over pieces of at most ``chunk`` elements:

      max|out - ref| <= rel * max|ref|        and, where ``strict``,     |out - ref| <= rel/10 * max|ref| + rel * |ref|  everywhere

    with max|ref| of the small reference; ``out`` must be finite.  ``out`` may be any view (the stem's channels-last result):
    indices are those of the logical (N, ...) order.  A failure names the flat index of the worst element and the largest
    threshold it lies past.  Returns max|out - ref| / max|ref|."""
    assert tuple(out.shape[1:]) == tuple(ref_small.shape[1:]), f"{what}: clip shape {tuple(out.shape[1:])} vs {tuple(ref_small.shape[1:])}"
    N, n0 = out.shape[0], ref_small.shape[0]
    clip = ref_small[0].numel()
    assert N >= 1 and n0 >= 1 and clip >= 1, what
    ref = ref_small.to(device=out.device, dtype=torch.float64).reshape(-1)
    scale = max(ref.abs().max().item(), 1e-30)
    atol = rel * 0.1 * scale
    itemsize = out.element_size()
    worst, worst_at, loose_at, bad_at = 0.0, 0, None, None
    group = max(1, chunk // clip)                      # whole clips per block; a clip above ``chunk`` is cut further below
    for a in range(0, N, group):
        b = min(N, a + group)
        block = out[a:b].reshape(-1)                   # (a copy for a strided view: at most max(chunk, one clip) elements)
        for c0 in range(0, block.numel(), chunk):
            got = block[c0:c0 + chunk].double()
            flat0 = a * clip + c0
            idx = torch.arange(flat0, flat0 + got.numel(), device=out.device) % (n0 * clip)
            want = ref[idx]
            fin = torch.isfinite(got)
            if bad_at is None and not bool(fin.all()):
                bad_at = flat0 + int((~fin).to(torch.uint8).argmax())
            d = (got - want).abs()
            d = torch.where(fin, d, torch.full_like(d, float("inf")))
            m, at = d.max(0)
            if m.item() > worst:
                worst, worst_at = m.item(), flat0 + int(at)
            if strict and loose_at is None:
                over = d > atol + rel * want.abs()
                if bool(over.any()):
                    loose_at = flat0 + int(over.to(torch.uint8).argmax())
            del got, want, d, fin, idx
    assert bad_at is None, f"{what}: non-finite output at {_fmt_threshold(bad_at, itemsize)} (clip {bad_at // clip}, offset {bad_at % clip})"
    assert worst <= rel * scale, (f"{what}: max abs err {worst:.3e} > {rel:g} * max|ref| ({scale:.3e}) at {_fmt_threshold(worst_at, itemsize)} "
                                  f"(clip {worst_at // clip}, offset {worst_at % clip})")
    assert loose_at is None, (f"{what}: allclose(rtol={rel}) failed, first at {_fmt_threshold(loose_at, itemsize)} "
                              f"(clip {loose_at // clip}, offset {loose_at % clip})")
    return worst / scale


def gate_small(got, ref, rel, what, strict=False, scale=None):
    """The same criteria for a small tensor (a parameter gradient, a statistic) against its fp64 reference, on the CPU.  ``scale``:
    the max|ref| to use where the reference itself is structurally zero."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    scale = max(ref.abs().max().item() if scale is None else scale, 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{what}: max abs err {err:.3e} > {rel:g} * max|ref| ({scale:.3e})"
    if strict:
        assert torch.allclose(got, ref, rtol=rel, atol=rel * 0.1 * scale), f"{what}: allclose(rtol={rel}) failed"
    return err / scale


def need_bytes(case):
    """Device memory a case holds at its peak: what it declares for its tensors (``case.tensors`` bytes: inputs, results,
    workspaces, everything the call saves) plus the gate's temporaries."""
    need = int(case.tensors) + GATE_BYTES
    assert need <= MAX_NEED, f"{case.id}: needs {need / GIB:.1f} GiB, more than {MAX_NEED // GIB} GiB"
    return need


def skip_unless_it_fits(case):
    """Skip iff the device reports less free memory than the case needs plus 2 GiB."""
    need = need_bytes(case)
    free, _ = torch.cuda.mem_get_info()
    if free < need + HEADROOM:
        pytest.skip(f"{case.id}: needs {need / GIB:.1f} GiB + {HEADROOM // GIB} GiB headroom, {free / GIB:.1f} GiB are free")


def release():
    """Give the device memory of a finished case back: the machine is shared."""
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ---- Table A: results past 2^31 elements ------------------------------------------------------------------------------------------
# Every row: the smallest per-unit shape that still reaches the named kernel, keeps N <= 65535 where the clip rides on a grid axis,
# and meets the no-aliasing condition (tests/test_large_extent_host.py asserts it for every row); N = the fewest whole tilings of
# the 7-unit batch past 2^31 elements.  At C = 128 and N <= 65535 a clip needs T * V >= 257.
# (math, C, T, V, input layout, output layout, bf16 output, kernel)
A_STEM = [("f32", 128, 12, 22, "nctv", "nctv", False, "stem_mfma_f32_kernel"),
          ("bf16x3", 128, 12, 22, "nctv", "nctv", False, "stem_bf16_v6_kernel"),
          ("bf16x3", 128, 12, 22, "nctv", "ntvc", True, "stem_bf16_v6_kernel"),
          ("f16mx", 128, 12, 22, "ntvc", "nctv", False, "stem_f16mx_kernel"),            # the STGCN_IN_NTVC row
          ("bf16x3", 128, 12, 25, "nctv", "nctv", False, "stem_bf16_v4_kernel"),
          ("bf16x3", 256, 3, 52, "nctv", "nctv", False, "stem_mfma_bf16_kernel")]        # 128 channels: no covered clip of 257 pixels
# (Cin, Cout, K, stride, T, V, math, bf16 output, along V, kernel).  The eight-wave kernel serves no 128 -> 128 clip of 257 pixels
# or more (the one-wave kernel takes them): its row has 16 input channels, the smallest such shape of TCN_SHAPES' family.
A_TCN = [(128, 128, 9, 1, 12, 22, "f32", False, False, "tcn_mfma_f32_kernel"),
         (128, 128, 9, 1, 12, 22, "bf16x3", False, False, "tcn_bf16_v6_kernel"),
         (128, 128, 9, 1, 12, 22, "bf16x3", True, False, "tcn_bf16_v6_kernel"),
         (128, 128, 9, 1, 12, 22, "f32_valu", False, False, "tcn_valu_kernel"),
         (128, 128, 9, 1, 12, 22, "f32_valu", False, True, "tcn_valu_joint_axis_kernel"),
         (128, 128, 9, 1, 7, 46, "bf16x3", False, False, "tcn_mfma_bf16_kernel"),
         (16, 128, 9, 1, 37, 7, "bf16x3", False, False, "tcn_bf16_v4_kernel"),
         (64, 128, 9, 2, 24, 22, "f32", False, False, "tcn_mfma_f32_kernel")]
A_AGCN = (3, 128, 12, 22)                                       # (Cin, Cout, T, V)
# (math, LayerNorm + bias + GELU, residual): y (M, 1024) from x (M, 64); the unit is a group of three rows, 3072 elements - one
# row is 2^10 elements, which every threshold is a multiple of
A_LINEAR = [("f32", True, False), ("bf16x3", False, True), ("bf16", False, False)]
LINEAR_K, LINEAR_NOUT, LINEAR_GROUP = 64, 1024, 3
# (form, L, head_dim) at 8 heads: out (B, L, 256); L = 3 is the shortest sequence whose 768 elements no threshold is a multiple
# of; the streaming form also at the shortest length only it covers
A_ATTENTION = [("resident", 3, 32), ("stream", 3, 32), ("split", 3, 32), ("stream", 257, 32)]
A_BLOCK = (3, 256, 8, 512)                                      # (L, D, heads, hidden): B * L * hidden crosses 2^31
A_TCN_TRAIN = (128, 128, 9, 1, 12, 22, "bf16x3")
A_AGCN_TRAIN = (3, 128, 12, 22)
A_ST_ATTENTION = [(3, 128, 12, 22, None), (3, 128, 12, 22, "bf16x3")]      # (Cin, Cout, T, V, math): the smallest covered width
# (L, D, heads, hidden): the narrowest block - what a training step saves grows with 5 D + 2 hidden floats a token, 21 GiB here
A_BLOCK_TRAIN = (3, 64, 2, 512)
A_HEAD = (6, 22)                # (T, V) of entry_points.small_head: N * T * V * 256 stage-1 tokens; the result is (N, 14) logits
# (C, T, V, p1, p2, E): the plan refuses a result of 2^31 elements, so this one crosses 2^30 (2^31 and 2^32 bytes) and its input z
# 2^31 elements; seven tokens of 64
A_PATCH = (32, 8, 6, 4, 2, 64)
A_POOL_CLASSIFY = (9, 64, 14)   # (L, D, classes): the input crosses, one workgroup of 1024 threads per clip: N < 2^22
POOL_CLASSIFY_CLIPS = 1 << 22


def _tcn_unit(cout, K, stride, T, V, along_v):
    pad = (K - 1) // 2
    out = lambda n: (n + 2 * pad - K) // stride + 1       # noqa: E731
    return (cout, T, out(V)) if along_v else (cout, out(T), V)


def stem_id(r):
    return f"stem-{r[0]}-C{r[1]}-{r[2]}x{r[3]}-in_{r[4]}-out_{r[5]}" + ("-bf16" if r[6] else "")


def tcn_id(r):
    return "tcn-" + "x".join(map(str, r[:6])) + f"-{r[6]}" + ("-bf16out" if r[7] else "") + ("-alongV" if r[8] else "")


def table_a():
    """{row id: Extent} of every row of Table A."""
    bf = lambda b: torch.bfloat16 if b else torch.float32       # noqa: E731
    t = {}
    for r in A_STEM:
        t[stem_id(r)] = Extent.past((r[1], r[2], r[3]), bf(r[6]))
    for r in A_TCN:
        t[tcn_id(r)] = Extent.past(_tcn_unit(r[1], r[2], r[3], r[4], r[5], r[8]), bf(r[7]))
    t["agcn_forward-" + "x".join(map(str, A_AGCN))] = Extent.past(A_AGCN[1:])
    for math, epi, res in A_LINEAR:
        t[f"vit_linear-{math}" + ("-ln_gelu" if epi else "") + ("-residual" if res else "")] = Extent.past((LINEAR_GROUP, LINEAR_NOUT))
    for form, L, hd in A_ATTENTION:
        t[f"vit_attention-{form}-L{L}-hd{hd}"] = Extent.past((L, 8 * hd))
    L, D, heads, hidden = A_BLOCK
    t["vit_block_forward-" + "x".join(map(str, A_BLOCK))] = Extent.past((L, D), named_per_unit=("hidden activation", L * hidden))
    t["tcn_train-" + "x".join(map(str, A_TCN_TRAIN))] = Extent.past(_tcn_unit(*A_TCN_TRAIN[1:6], False))
    t["agcn_train-" + "x".join(map(str, A_AGCN_TRAIN))] = Extent.past(A_AGCN_TRAIN[1:])
    for r in A_ST_ATTENTION:
        t["st_attention_forward-" + "x".join(map(str, r[:4])) + "-" + (r[4] or "f32")] = Extent.past((r[1], r[2], r[3]))
    L, D, heads, hidden = A_BLOCK_TRAIN
    t["vit_block_train-" + "x".join(map(str, A_BLOCK_TRAIN))] = Extent.past((L, D), named_per_unit=("hidden activation", L * hidden))
    t["altformer_head_forward-%dx%d" % A_HEAD] = Extent.past((14,), named_per_unit=("stage-1 tokens", A_HEAD[0] * A_HEAD[1] * 256))
    C, T, V, p1, p2, E = A_PATCH
    tokens = (T // p1) * (V // p2) + 1
    N = N0 * tiles_past(1 << 30, tokens * E)
    t["vit_patch_embed-" + "x".join(map(str, A_PATCH))] = Extent(N, (tokens, E), named=("input z", N * C * T * V))
    L, D, classes = A_POOL_CLASSIFY
    t["vit_pool_classify-" + "x".join(map(str, A_POOL_CLASSIFY))] = Extent.past((classes,), named_per_unit=("input x", L * D))
    return t


# ---- Table B: the clip limit, on the smallest clips --------------------------------------------------------------------------------
MAX_CLIPS = 65535               # kMaxGridClips (csrc/common.h)
