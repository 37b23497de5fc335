"""The case table and the helpers of the stream contract ("Streams"): everything an entry point does is ordered on
the stream it is given, nothing it does waits on the host, and every entry point can be captured into a graph.  Shared by
tests/test_stream_order_host.py (the decoy cannot pass, every stream-taking entry point of include/stgcn_hip.h is accounted
for; no GPU) and tests/test_stream_order_gpu.py (the held stream, the replay, the control).  Not a conftest.py: a plain module.

A case is a row of tests/nonfinite_cases.py - one per family and arithmetic, the table's own shapes - or one of the setups
of tests/entry_points.py the table predates; both give ``x``, ``reference(x)`` and ``on(dev) -> run(x)``.

THE HELD STREAM (``held_run``).  The decoy is the clean input rolled by one along its unit axis and multiplied by -0.5.  After a
warm-up on the decoy a non-blocking side stream is kept busy by a chain of matmuls; behind that hold go ``run(decoy)``, a copy of
the clean input into the same device tensor, ``run`` again and an event.  If the hold's end event has not completed once the
last call is enqueued, all of both calls was enqueued while none of it could run: a launch, memset or torch op that went to
another stream ran ahead of its producers (it read the decoy, the decoy's stale intermediates, or - an off-stream memset
behind atomics - zeroed twice before either call added), and a host wait inside the call ended the hold.  The second result is
held to ``reference(clean)`` with the case's gates.  Every buffer is allocated and valid throughout: a failing case gives wrong
numbers, never a fault.

GATES.  Inference rows keep the gates of their row (``prep.gate`` / ``prep.gates``).  The training rows of the non-finite table
owe that contract condition (a) only, so their ``gate`` was never applied to a gradient; here they get the gates of the entry
point's own test, given with their rows below (gradients: the max-norm criterion; the graph conv's and the temporal conv's
steps use the kink-free cotangent of their own tests, from the same setups, because a random cotangent on a ReLU output that
fp32 rounds to the other side of zero moves a gradient by a whole |dL/dy|).  Gradients that are analytically zero - a bias in
front of a batch-statistics BatchNorm, conv_a's bias under the soft-max - are rounding noise on both sides: they are named in
``no_dependence`` with the outputs that cannot depend on ``x``, and checked only through the others.

The stem's training step (stem_train-bf16x3 of the non-finite table) is no row: it is unit_agcn's and Unit2D's steps one after
the other, both of which are rows, and its own test already captures it into a graph."""
import functools
import math
import os
import re
import time

import torch

import entry_points as ep
import nonfinite_cases as nf
from _util import MATH_GATES, parity_gate
from entry_points import TRAIN_STRICT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stgcn_hip.h")

# The hold: at least HOLD_FACTOR times the slowest case's host time to enqueue its two calls (profiles/stream_order_enqueue_times.txt;
# the factor covers host jitter on a shared machine).  The condition ``hold_end.query() is False`` guards every case, not this number.
HOLD_FACTOR = 4
SLOWEST_ENQUEUE_MS = 5.0          # measured 4.15 ms (agcn_train-moment_form: two module steps with a deepcopy and autograd each)
HOLD_MS = max(HOLD_FACTOR * SLOWEST_ENQUEUE_MS, 100.0)     # the floor: what an idle-stream measurement does not see (a busy host)
HOLD_N = 4096                     # the hold's matmuls are (HOLD_N x HOLD_N) fp32

# Cases whose wrapper must wait on the host: id -> reason.  At most three, none a whole family.
EXEMPT = {}
assert len(EXEMPT) <= 3

GRAD = (1e-4, False)              # _util.grad_gate / agcn_compare_grads / st_attention_train_gate: max-norm only


def stream_entry_points(text=None):
    """Every function of include/stgcn_hip.h with a ``void *stream`` parameter, in the header's order."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(stgcn_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
            if re.search(r"void\s*\*\s*stream\b", m.group(2))]


# The modules stage their parameters on their first call (the warm-up): these may be recorded beyond a case's declaration.
STAGING = frozenset({"stgcn_bn_fold", "stgcn_tcn_pack", "stgcn_stem_prepare"})

# Entry points no case is needed for: name -> (the covering case, or None, and one line of reason).
COVERED_THROUGH = {
    "stgcn_stem_forward_prepared": ("stem_fused-3x37x22x128-f32", "the one-shot form: stgcn_stem_attention then stgcn_stem_tail_prepared "
                                    "on the same stream, the two calls F.stem_forward makes"),
    "stgcn_stem_prepare": ("stem_fused-3x37x22x128-f32", "packs parameters once per module; its operands are no activation a case can "
                           "make late, its blob is what every stem case reads"),
    "stgcn_vit_linear_bf16": ("vit_block-3x33x256-bf16", "a wrapper round launch_linear with STGCN_MATH_BF16, the call the bf16 block "
                              "makes for its four linears"),
    "stgcn_vit_attention_bf16": ("vit_block-3x33x256-bf16", "a wrapper round launch_attention_bf16, the bf16 block's attention"),
    "stgcn_vit_attention_train_bf16": ("vit_block_train-3x33x256-f32-attention_bf16", "a wrapper round launch_attention_train_bf16, the "
                                       "training forward's attention under VIT_TRAIN_ATTN_BF16"),
    "stgcn_vit_attention_backward_bf16": ("vit_block_train-3x33x256-f32-attention_bf16", "a wrapper round launch_attention_backward_bf16, "
                                          "the block backward's attention under VIT_TRAIN_ATTN_BF16"),
}


class StreamCase:
    """``case``: anything with ``prepare() -> nonfinite_cases.Prepared``.  ``symbols``: the stream-taking entry points ``run``
    calls (the GPU file records the real ones and compares).  ``replay``: no existing test captures this path, so the replay
    test does.  ``no_dependence``: {output: reason} - not compared, see the module docstring.  ``gates``: {output: (rel, strict)}
    over the row's own, ``gate`` for the rest."""

    def __init__(self, id, case, symbols, replay, no_dependence=None, gate=None, gates=None):
        self.id, self.case, self.symbols, self.replay = id, case, frozenset(symbols), replay
        self.no_dependence, self._gate, self._gates = dict(no_dependence or {}), gate, dict(gates or {})

    def prepare(self):
        return self.case.prepare()

    def gate_of(self, prep, name):
        if name in self._gates:
            return self._gates[name]
        if self._gate is not None:
            return self._gate
        return prep.gates.get(name, prep.gate)


class _Own:
    """A row of this file: ``prepare`` from a setup of tests/entry_points.py, made once."""

    def __init__(self, make, *args, gate=MATH_GATES["f32"], on=None):
        self._make, self._args, self._gate, self._on = make, args, gate, on

    @functools.lru_cache(maxsize=None)
    def prepare(self):
        s = self._make(*self._args)
        on = s.on if self._on is None else functools.partial(self._on, s)
        return nf.Prepared(s.x, [], s.reference, on, self._gate)


CASES = []
_TABLE = {c.id: c for c in nf.CASES}


def row(id, symbols, replay, **kw):
    """A row of the non-finite table."""
    CASES.append(StreamCase(id, _TABLE[id], symbols, replay, **kw))


def own(id, symbols, replay, make, *args, gate=MATH_GATES["f32"], on=None, **kw):
    CASES.append(StreamCase(id, _Own(make, *args, gate=gate, on=on), symbols, replay, **kw))


ZERO = "analytically zero: rounding noise on both sides"
FC2_BIAS = {"dmlp.fc2.bias": "the sum of the cotangent (times the branch's factors) over the tokens: it does not read x"}
_AGCN_ZERO = {f"d{p}_b{i}": ZERO for p in "ad" for i in range(3)}


def _build():
    # ---- inference -------------------------------------------------------------------------------------------------------------
    agcn = {"stgcn_agcn_forward", "stgcn_agcn_attention"}
    row("agcn-2x3x64x9x25", agcn, True)
    row("agcn-2x16x32x5x7", agcn, True)                     # agcn_expand_generic_kernel
    tcn = {"stgcn_tcn_pack", "stgcn_tcn_forward_packed", "stgcn_tcn_forward"}
    packs = lambda s, dev: s.on(dev, pack_every_run=True)       # noqa: E731  (stgcn_tcn_pack inside the held calls)
    for ci, co, K, st, T, V, N, m, ob, av in [s for s in ep.TCN_SHAPES if s[:6] == (128, 128, 9, 1, 41, 22)] + ep.TCN_SHAPES[15:18]:
        CASES.append(StreamCase(f"tcn-{ci}x{co}x{K}x{st}x{T}x{V}x{N}-{m}" + ("-bf16out" if ob else "") + ("-alongV" if av else ""),
                                _Own(ep.tcn, ci, co, K, st, T, V, N, m, ob, av, on=packs,
                                     gate=(nf.BF16_OUT_GATE, False) if ob else MATH_GATES[m]),
                                tcn - ({"stgcn_tcn_forward"} if av else set()), True))
    stem = {"stgcn_stem_attention", "stgcn_stem_tail_prepared"}
    for m in ep.STEM_MATHS:
        row(f"stem_fused-3x37x22x128-{m}", stem, False)
    row("stem_two_stage-3x37x22x128-f32", {"stgcn_agcn_forward", "stgcn_tcn_forward_packed"}, True)
    row("patch_embed-ST-nctv", {"stgcn_patch_embed"}, False)
    row("patch_embed-TS-ntvc", {"stgcn_patch_embed"}, False)
    row("st_attention-2x131x128x12x22", {"stgcn_st_attention_forward"}, True)
    row("vit_linear-129x96x100-f32", {"stgcn_vit_linear"}, False)
    row("vit_linear-129x96x100-bf16x3", {"stgcn_vit_linear"}, False)
    row("vit_attention-resident-3x33-hd32", {"stgcn_vit_attention"}, False)
    row("vit_attention-stream-2x257-hd32", {"stgcn_vit_attention_stream"}, False)
    row("vit_attention-split-2x33-hd32", {"stgcn_vit_attention_split"}, False)
    for m in ("f32", "mixed", "bf16"):
        row(f"vit_block-3x33x256-{m}", {"stgcn_vit_block_forward"}, False)
    row("vit_pool-3x33x256-mean", {"stgcn_vit_pool"}, False)
    row("vit_pool-3x33x256-max", {"stgcn_vit_pool"}, False)
    row("vit_pool_classify-3x65x256x14-max", {"stgcn_vit_pool_classify"}, False)
    row("head-ST-whole", {"stgcn_altformer_head_forward"}, False)
    model = {"stgcn_stem_attention", "stgcn_stem_tail_prepared", "stgcn_patch_embed", "stgcn_vit_block_forward"}
    row("model-ST-per_block", model, False)
    row("model-TS-bf16", model, False)
    own("bn_fold-70", {"stgcn_bn_fold"}, True, ep.bn_fold, 70, no_dependence={"scale": "the scale does not read the running mean"})
    # the ST-ViT forward's embedding (stvit_ref.py)
    own("vit_patch_embed-a_K256_rows18-nchw-f32", {"stgcn_vit_patch_embed"}, True, ep.vit_patch_embed, "a_K256_rows18", "nchw", "f32")
    own("vit_patch_embed-a_K256_rows18-ntvc-bf16x3", {"stgcn_vit_patch_embed"}, True, ep.vit_patch_embed, "a_K256_rows18", "ntvc", "bf16x3")
    # ST-TR's unit under bf16x3 (st_attention_math_ref.py)
    own("st_attention_math-eval_k131_tv75-bf16x3", {"stgcn_st_attention_forward_math"}, True, ep.st_attention_math, "eval_k131_tv75")
    own("wx_product-skip-bf16x3", {"stgcn_wx_product"}, True, ep.wx_product, "skip")
    own("step_stats-300x28", {"stgcn_step_stats"}, True, ep.step_stats, 300, 28, gates={"probe": (1e-4, False)})
    # ---- training --------------------------------------------------------------------------------------------------------------
    agcn_train = {"stgcn_agcn_forward_train", "stgcn_agcn_backward_train"}

    def same_module(s, dev):
        """The setup's own module in every run, its state put back from device copies first.  (The setup's default, a deep copy
        per run, is a module on its first call each time: staging one uploads the constant adjacency from the host, a host
        wait that belongs to a module's first call and not to a training step.)"""
        run, m = s.on(dev, fresh=False), s.module
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}

        def step(x):
            m.load_state_dict(state)
            out = run(x)
            out["bn.running_mean"], out["bn.running_var"] = m.bn.running_mean.clone(), m.bn.running_var.clone()
            if m._has_down():
                out["down.running_mean"], out["down.running_var"] = m.down[1].running_mean.clone(), m.down[1].running_var.clone()
            return out
        return step
    own("agcn_train-moment_form-3x128-3x20x22", agcn_train, False, ep.agcn_train, 3, 128, 3, 20, 22, False, True, on=same_module, gate=GRAD, gates={"y": MATH_GATES["f32"], "P": MATH_GATES["f32"]}, no_dependence={**_AGCN_ZERO, "ddown_b": ZERO})
    own("agcn_train-generic-64x64-2x12x22-dx", agcn_train, True, ep.agcn_train, 64, 64, 2, 12, 22, True, True, on=same_module, gate=GRAD, gates={"y": MATH_GATES["f32"], "P": MATH_GATES["f32"]}, no_dependence=_AGCN_ZERO)
    tcn_train = {"stgcn_tcn_forward_train", "stgcn_tcn_backward_train"}
    for (ci, co, K, st, N, T, V), m in [((64, 128, 9, 1, 2, 21, 22), "bf16x3"), ((64, 128, 9, 2, 2, 21, 22), "bf16x3"),
                                        ((32, 64, 2, 1, 2, 7, 22), "bf16x3"), ((32, 64, 9, 1, 2, 7, 22), "f32_valu")]:
        own(f"tcn_train-{ci}x{co}x{K}x{st}x{N}x{T}x{V}-{m}", tcn_train, True, ep.tcn_train, ci, co, K, st, N, T, V, m, True, True,
            gate=GRAD, gates={"y": MATH_GATES[m]})       # (dbias, analytically zero, is in no reference)
    for m in ("bf16x3", "f32_valu"):
        row(f"tcn_saved-64x128x9x1x2x21x22-{m}", {"stgcn_tcn_forward_train"}, True)
    st_train = {"stgcn_st_attention_forward_train", "stgcn_st_attention_backward"}
    row("st_attention_train-2x131x128x12x22", st_train, True, gate=GRAD, gates={"y": MATH_GATES["f32"]},
        no_dependence={"dattention_conv.attn_out.bias": ZERO})
    own("st_attention_math-c512_v46-bf16x3-train", st_train, True, ep.st_attention_math, "c512_v46", gate=GRAD,
        gates={"y": MATH_GATES["f32"]}, no_dependence={"dattention_conv.attn_out.bias": ZERO})
    block_train = {"stgcn_vit_block_forward_train", "stgcn_vit_block_backward"}
    for m in ("f32", "bf16x3", "bf16"):
        row(f"vit_block_train-3x33x256-{m}", block_train, True,
            gate=MATH_GATES["bf16"] if m == "bf16" else (MATH_GATES["f32"][0], TRAIN_STRICT[m]), no_dependence=FC2_BIAS)
    row("vit_block_train-3x33x256-f32-attention_bf16", block_train, True, no_dependence=FC2_BIAS)
    row("vit_block_train-2x257x256-f32-streaming", block_train, True, no_dependence=FC2_BIAS)
    drop = {"stgcn_vit_block_forward_train_drop", "stgcn_vit_block_backward_drop"}
    own("vit_block_train_drop-odd-f32", drop, True, ep.vit_block_train_drop, "odd", "f32", no_dependence=FC2_BIAS)
    own("vit_block_train_small-5x46x256-f32", drop, True, ep.vit_block_train_small, 5, 46, 256, "f32", no_dependence=FC2_BIAS)
    own("vit_linear_backward-129x512x512-bf16x3", {"stgcn_vit_linear_backward"}, True, ep.vit_linear_backward, 129, 512, 512, "bf16x3")
    own("vit_layernorm_backward-7x260", {"stgcn_vit_layernorm_backward"}, True, ep.vit_layernorm_backward, 7, 260)
    own("vit_attention_backward-3x65-hd32", {"stgcn_vit_attention", "stgcn_vit_attention_backward"}, True, ep.vit_attention_backward, 3, 65, 32)
    own("vit_attention_backward_stream-2x257-hd32", {"stgcn_vit_attention_stream", "stgcn_vit_attention_backward_stream"}, True,
        ep.vit_attention_backward, 2, 257, 32, "stream")
    own("vit_patch_embed_backward-a_K256_rows18-ntvc-bf16x3", {"stgcn_vit_patch_embed_backward"}, True, ep.vit_patch_embed_backward,
        "a_K256_rows18", "ntvc", "bf16x3", gate=(1e-4, TRAIN_STRICT["bf16x3"]))
    own("vit_pool_classify_backward-small-cls", {"stgcn_vit_pool_classify_backward"}, True, ep.vit_pool_classify_backward, "small", "cls",
        no_dependence={"dbias": "the sum of dlogits over the clips: it does not read x",
                       "dln_bias": "the sum of dlogits W over the clips: it does not read x"})


_build()
CASES = [c for c in CASES if c.id not in EXEMPT]
assert len({c.id for c in CASES}) == len(CASES)


# ---- the decoy ------------------------------------------------------------------------------------------------------------------
def decoy(x):
    """The clean input with its unit axis (axis 0) rolled by one and multiplied by -0.5; where that axis has length one the last
    axis is reversed instead.  Finite, and of the same shape."""
    y = torch.roll(x, 1, 0) if x.shape[0] > 1 else torch.flip(x, (-1,))
    return (y * -0.5).contiguous()


def distances(case, clean_ref, other_ref, prep):
    """[(name, distance, gate scale)] over the compared outputs: max|other - clean| against rel * max|clean|."""
    out = []
    for name, r in clean_ref.items():
        if name in case.no_dependence:
            continue
        rel, _ = case.gate_of(prep, name)
        r, o = r.detach().double(), other_ref[name].detach().double()
        out.append((name, (o - r).abs().max().item(), rel * max(r.abs().max().item(), 1e-30)))
    return out


# ---- comparing a result with the reference ------------------------------------------------------------------------------------------
def mismatches(case, prep, out, ref, what):
    """The outputs of ``out`` that miss their gate against ``ref`` (the case's own gates through _util.parity_gate), as messages;
    prints each figure first."""
    bad = []
    for name, r in ref.items():
        if name in case.no_dependence:
            continue
        o = out.get(name)
        if o is None:
            bad.append(f"{what}: output {name} is missing")
            continue
        rel, strict = case.gate_of(prep, name)
        o, r = o.detach().double().cpu().reshape(r.shape), r.detach().double()
        err = (o - r).abs().max().item() / max(r.abs().max().item(), 1e-30)
        print(f"{what} {name}: max|err| / max|ref| = {err:.3e} (gate {rel:g}{', both criteria' if strict else ''})")
        try:
            parity_gate(o, r, rel, f"{what} {name}", strict)
        except AssertionError as e:
            bad.append(str(e))
    return bad


# ---- the hold and the held run ------------------------------------------------------------------------------------------------------
class Hold:
    """Plain torch work that keeps a stream busy for about ``ms``: a chain of fp32 matmuls on scratch tensors allocated here,
    its length from one timed matmul."""

    def __init__(self, dev, ms=HOLD_MS, n=HOLD_N):
        g = torch.Generator(device=dev).manual_seed(1)
        self.a = torch.randn(n, n, device=dev, generator=g) / math.sqrt(n)
        self.b = torch.randn(n, n, device=dev, generator=g) / math.sqrt(n)
        self.c = torch.empty(n, n, device=dev)
        torch.matmul(self.a, self.b, out=self.c)
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(4):
            torch.matmul(self.a, self.b, out=self.c)
        t1.record()
        t1.synchronize()
        self.matmul_ms = t0.elapsed_time(t1) / 4
        self.ms = ms
        self.count = max(4, int(math.ceil(ms / self.matmul_ms)))

    def enqueue(self):
        """The chain on the current stream, and the event behind it."""
        for _ in range(self.count):
            torch.matmul(self.a, self.b, out=self.c)
        end = torch.cuda.Event()
        end.record()
        return end


def held_run(run, clean, dev, hold, what):
    """Steps 2 - 5 of the module docstring for ``run(x) -> {name: tensor}`` and the clean CPU input: returns the second call's
    outputs after the side stream's event has been waited for.  Fails (no skip, no retry) if the hold ended before the last
    enqueue: the case is then inconclusive."""
    clean_dev = clean.to(dev)
    xd = decoy(clean).to(dev)
    run(xd.detach())                                    # warm-up on the default stream: lazy loading, stale workspaces of the decoy
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                       # and on the side stream, whose blocks the held calls reuse: the same decoy
        run(xd.detach())
    side.synchronize()
    with torch.cuda.stream(side):
        hold_end = hold.enqueue()
        t0 = time.perf_counter()
        run(xd.detach())
        with torch.no_grad():
            xd.copy_(clean_dev)                         # the late input, ordered on the side stream
        out = run(xd.detach())
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        done = torch.cuda.Event()
        done.record()
    held = not hold_end.query()                         # before any synchronisation
    print(f"{what}: enqueued both calls in {enqueue_ms:.2f} ms behind a hold of {hold.count} matmuls (~{hold.count * hold.matmul_ms:.0f} ms); "
          f"hold_end.query() = {not held}")
    done.synchronize()
    torch.cuda.synchronize(dev)
    assert held, (f"{what}: inconclusive - the hold had ended when the last call was enqueued ({enqueue_ms:.2f} ms for both calls): "
                  "a host wait inside the call, or a hold too short for this machine")
    return out


class Recorder:
    """For the duration of the block, stgcn_amd._capi hands out a proxy of the loaded library that notes every symbol looked up
    on it (``_capi.call`` and ``_capi.lib()`` both go through the module's handle); the binding itself is unchanged."""

    def __init__(self):
        self.names = set()

    def __enter__(self):
        from stgcn_amd import _capi
        self._capi, self._real, rec = _capi, _capi.lib(), self

        class Proxy:
            def __getattr__(self, name):
                rec.names.add(name)
                return getattr(rec._real, name)
        _capi._lib = Proxy()
        return self

    def __exit__(self, *exc):
        self._capi._lib = self._real
        return False
