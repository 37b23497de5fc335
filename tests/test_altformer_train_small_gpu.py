"""GPU tests of the small training calls of the heads' blocks (``STGCN_VIT_WGRAD_SMALL``, ``set_low_latency_training``):
both forms of both weight-gradient kernels against fp64 - exactly, on small integers, and at the standing
gates on random inputs -, the row factors through ``stgcn_vit_block_backward_drop``, a block and the whole model through the
modules, what must not move with the switch off, and the flagged linear backward under poisoned, guard-banded buffers and with
a NaN in its input."""
import functools

import pytest
import torch

import altformer_ref as ar
import altformer_train_ref as tr
from _util import MATH_GATES, HostileCase, load_golden, parity_gate, run_under_both_fills
from entry_points import TRAIN_STRICT, hipF, run_block
from test_altformer_gpu import whole_model
from test_altformer_train_gpu import PinnedMax, check_stem_grads, compare_grads, set_force_torch, step

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
# (relative bound, both criteria) per arithmetic of the weight gradient: the project's standing gates
GATES = {"f32": MATH_GATES["f32"], "bf16": MATH_GATES["bf16"]}
# (M, K, Nout): one token and one partial tile; M off the chunk, K and Nout off 64; several splits with a ragged last one; the
# two products of the TS head's spatial stage at batch 32
SHAPES = [(1, 32, 4), (70, 96, 100), (333, 160, 196), (704, 512, 512), (704, 512, 1536)]
WEIGHTS = ("attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "mlp.fc1.weight", "mlp.fc1.bias",
           "mlp.fc2.weight", "mlp.fc2.bias")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


def wgrad_math(arith, small=True):
    from stgcn_amd import _capi
    return (_capi.VIT_TRAIN_BF16 if arith == "bf16" else 0) | (_capi.VIT_WGRAD_SMALL if small else 0)


# ---- 1. both forms of both kernels through stgcn_vit_linear_backward ------------------------------------------------------------
def test_the_shapes_reach_both_forms_more_than_one_split_and_a_direct_store():
    from stgcn_amd import _capi
    F = hipF()
    plans = [F.vit_wgrad_plan(*s, _capi.VIT_WGRAD_SMALL) for s in SHAPES]
    print("plans (tile, splits, direct):", dict(zip(SHAPES, plans)))
    assert all(p[0] == 64 for p in plans[:4])
    assert any(p[1] > 1 for p in plans) and any(p[2] for p in plans)
    assert F.vit_wgrad_plan(333, 160, 196, _capi.VIT_WGRAD_SMALL)[1] > 1 and 333 % 32 != 0, "a ragged last split"


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "no_db"])
@pytest.mark.parametrize("arith", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_small_integers_come_out_exact(shape, arith, with_db, dev):
    """dY and A are integers in [-2, 2]: every product and every partial sum (at most 4 M = 2,816 < 2^24 in magnitude) is exact
    in fp32 and the operands are exact in bf16, so dW and db equal the fp64 result whatever the form, the split and the order."""
    F = hipF()
    M, K, Nout = shape
    g = torch.Generator(device=dev).manual_seed(7 * M + K + Nout)
    dy = torch.randint(-2, 3, (M, Nout), generator=g, device=dev).float()
    a = torch.randint(-2, 3, (M, K), generator=g, device=dev).float()
    W = torch.zeros(Nout, K, device=dev)
    for small in (True, False):
        _, dW, db = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=with_db, math=wgrad_math(arith, small))
        assert torch.equal(dW.double(), dy.double().T @ a.double()), f"{shape} {arith} small={small}: dW"
        assert (db is None) == (not with_db)
        if with_db:
            assert torch.equal(db.double(), dy.double().sum(0)), f"{shape} {arith} small={small}: db"


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "no_db"])
@pytest.mark.parametrize("arith", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_inputs_hold_the_gates_and_agree_with_the_unflagged_call(shape, arith, with_db, dev):
    F = hipF()
    M, K, Nout = shape
    rel, strict = GATES[arith]
    g = torch.Generator(device=dev).manual_seed(M + K + Nout)
    dy = torch.randn(M, Nout, generator=g, device=dev) * (0.25 + 3.75 * torch.rand(M, 1, generator=g, device=dev))
    a = torch.randn(M, K, generator=g, device=dev) + 0.5
    W = torch.zeros(Nout, K, device=dev)
    want_w, want_b = (dy.double().T @ a.double()).cpu(), dy.double().sum(0).cpu()
    _, dW, db = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=with_db, math=wgrad_math(arith))
    _, dW0, db0 = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=with_db, math=wgrad_math(arith, small=False))
    what = f"{shape} {arith}"
    print(f"{what} dW vs fp64: {parity_gate(dW, want_w, rel, what + ' dW', strict):.3e}",
          f"vs unflagged: {parity_gate(dW, dW0, rel, what + ' dW vs the unflagged call', strict):.3e}")
    if with_db:
        print(f"{what} db vs fp64: {parity_gate(db, want_b, rel, what + ' db', strict):.3e}",
              f"vs unflagged: {parity_gate(db, db0, rel, what + ' db vs the unflagged call', strict):.3e}")
    _, dW2, db2 = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=with_db, math=wgrad_math(arith))
    assert torch.equal(dW, dW2) and (db is None or torch.equal(db, db2)), "two runs are bit-identical"


# ---- 2. row factors through stgcn_vit_block_backward_drop -------------------------------------------------------------------
def small_word(mode):
    from stgcn_amd import _capi
    from stgcn_amd.altformer import HEAD_TRAIN_MATH
    return HEAD_TRAIN_MATH[mode] | _capi.VIT_TILE_AUTO | _capi.VIT_WGRAD_SMALL


def drop_pair(blk, x, dy, math, s1=None, s2=None, drop=(None, None, None)):
    """A Block's training step through the functional ``_drop`` pair -> (y, {"x" and tr.PARAMS: gradient})."""
    F = hipF()
    ps = [None if p is None else p.detach() for p in blk._weights()]
    args = (blk.attn.num_heads, blk.norm1.eps, blk.attn.scale, math, s1, s2)
    y, saved = F.vit_block_forward_train(x, ps, *args, drop=drop)
    g = F.vit_block_backward(x, ps, saved, dy, *args, drop=drop)
    return y, {"x": g["x"], **{k: g[n] for k, n in zip(tr.PARAMS, F.VIT_BLOCK_PARAMS)}}


def seeded_block(D, seed, qkv_bias=True):
    from stgcn_amd.altformer import Block
    torch.manual_seed(seed)
    blk = Block(dim=D, num_heads=ar.HEADS, mlp_ratio=2., qkv_bias=qkv_bias, norm_layer=ar.norm_layer())
    ar.prepare_block(blk, seed)
    return blk.eval()


def seeded_io(B, L, D, seed):
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, L, D, generator=g)
    x = (x * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)).contiguous()
    return x, torch.randn(B, L, D, generator=torch.Generator().manual_seed(seed + 21))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,L", [(3, 22), (5, 46)], ids=["3x22", "5x46"])
def test_row_factors_with_a_dropped_sequence(B, L, mode, dev):
    """66 and 230 tokens at D = 256: sequences of 22 and 46 tokens cross the chunks of 32 and (at 230 tokens, where the qkv
    product has two splits of 128) the split boundary, and one sequence of each branch has the factor 0."""
    from stgcn_amd import _capi
    F = hipF()
    D, seed = 256, 9300 + L
    assert F.vit_wgrad_plan(B * L, D, D, _capi.VIT_WGRAD_SMALL)[0] == 64
    assert B * L == 66 or (F.vit_wgrad_plan(230, D, 3 * D, _capi.VIT_WGRAD_SMALL)[1] == 2 and 128 % L != 0)
    blk = seeded_block(D, seed)
    x, dy = seeded_io(B, L, D, seed)
    s1, s2 = tr.make_scales(B, seed)
    assert (s1 == 0).any() and (s2 == 0).any() and (s1 > 1).any()
    want_y, want = tr.grads64(x, blk.state_dict(), dy, scale=blk.attn.scale, s1=s1, s2=s2)
    blk = blk.to(dev)
    y, g = drop_pair(blk, x.to(dev), dy.to(dev), small_word(mode), s1.to(dev), s2.to(dev))
    rel, strict = GATES[mode]
    what = f"{B}x{L} {mode} masked"
    print(f"{what} y: {parity_gate(y, want_y, rel, what + ' y', strict):.3e}")
    for k, v in want.items():
        print(f"{what} d{k}: {parity_gate(g[k], v, rel, f'{what} d{k}', strict):.3e}")


# ---- 3. one block through the module ----------------------------------------------------------------------------------------
# the six cases of the gradient fixture, one sequence of 180 tokens at D = 512, and two sequences of 22 at D = 256
EXTRA_CASES = {"one_sequence_L180_D512": (1, 180, 512, 9201), "two_sequences_L22_D256": (2, 22, 256, 9202)}
BLOCK_NAMES = sorted(ar.BLOCK_CASES) + sorted(EXTRA_CASES)
BLOCK_GATES = {"f32": (REL, TRAIN_STRICT["f32"]), "mixed": (REL, TRAIN_STRICT["mixed"]), "bf16": MATH_GATES["bf16"]}


@functools.lru_cache(maxsize=None)
def block_case(name):
    """(block on the CPU, x, dy, fp64 y, fp64 gradients) of a case: made once, shared by the arithmetic modes, never changed."""
    from stgcn_amd.altformer import Block
    if name in ar.BLOCK_CASES:
        blk, x, dy = ar.build_block(Block, name), ar.make_input(name), tr.make_dy(name)
    else:
        B, L, D, seed = EXTRA_CASES[name]
        blk = seeded_block(D, seed)
        x, dy = seeded_io(B, L, D, seed)
    want_y, want = tr.grads64(x, blk.state_dict(), dy, scale=blk.attn.scale)
    return blk, x, dy, want_y, want


def test_the_fixture_cases_are_the_ones_meant():
    ref = load_golden("altformer_train_reference")
    assert len(ar.BLOCK_CASES) == 6 and all(f"case.{n}.dy_idx" in ref for n in ar.BLOCK_CASES)


@pytest.mark.parametrize("mode", sorted(BLOCK_GATES))
@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_block_through_the_module(name, mode, dev):
    import copy
    from stgcn_amd import _capi
    from stgcn_amd.altformer import set_low_latency_training, set_train_math
    cpu, x, dy, want_y, want = block_case(name)
    blk = copy.deepcopy(cpu).to(dev)
    set_train_math(blk, mode)
    xd, dyd = x.to(dev), dy.to(dev)
    blk.hip_train_min_tokens = 0
    probe = xd.clone().requires_grad_(True)
    assert blk.trains_on_hip(probe) and blk._hip_flags(probe, train=True) & _capi.VIT_WGRAD_SMALL == 0
    y0, g0 = tr.module_grads(blk, xd, dyd)
    set_low_latency_training(blk, train_min_tokens=0)
    assert blk.small_tiles_train and blk.trains_on_hip(probe) and blk._hip_flags(probe, train=True) & _capi.VIT_WGRAD_SMALL
    y1, g1 = tr.module_grads(blk, xd, dyd)
    y2, g2 = tr.module_grads(blk, xd, dyd)
    rel, strict = BLOCK_GATES[mode]
    what = f"{name} {mode} small"
    print(f"{what} y: {parity_gate(y1, want_y, rel, what + ' y', strict):.3e}")
    assert torch.equal(y1, y0) and torch.equal(y1, y2), "the forward's forms agree bit for bit"
    for k, v in want.items():
        if g1[k] is None:
            assert k == "attn.qkv.bias" and blk.attn.qkv.bias is None
            continue
        print(f"{what} d{k}: {parity_gate(g1[k], v, rel, f'{what} d{k}', strict):.3e}")
        assert torch.equal(g1[k], g2[k]), f"{what}: d{k} differs between two runs"
        if k in WEIGHTS:
            parity_gate(g1[k], g0[k], rel, f"{what} d{k} vs the switch-off run", strict)
        else:
            assert torch.equal(g1[k], g0[k]), f"{what}: d{k} is not the switch-off run's"


def test_trains_on_hip_at_704_tokens(dev):
    from stgcn_amd.altformer import HIP_TRAIN_MIN_TOKENS, Block, set_low_latency, set_low_latency_training
    blk = Block(512, 8, mlp_ratio=2., qkv_bias=True).to(dev)
    x = torch.zeros(32, 22, 512, device=dev, requires_grad=True)
    assert blk.hip_train_min_tokens == HIP_TRAIN_MIN_TOKENS and not blk.trains_on_hip(x)
    set_low_latency_training(blk, train_min_tokens=0)
    assert blk.trains_on_hip(x)
    set_low_latency(blk, enabled=False)
    assert not blk.trains_on_hip(x)


# ---- 4. the whole model -----------------------------------------------------------------------------------------------------
@pytest.fixture
def pinned_max(monkeypatch):
    from stgcn_amd import altformer
    pin = PinnedMax()
    monkeypatch.setattr(altformer, "max_over_tokens", pin)
    return pin


@pytest.mark.parametrize("style", ["ST", "TS"])
def test_whole_model_step_at_two_clips(style, dev, pinned_max):
    """2 clips of 180 x 22 (the second stage of a head has 360 or 44 tokens): every block on the HIP training path with the
    switch on, every parameter gradient against the same model with its blocks on torch ops."""
    import torch.nn as nn
    from stgcn_amd import _capi
    from stgcn_amd.altformer import Block, set_low_latency_training
    model, g = whole_model(style, dev, policy="default")
    set_low_latency_training(model, train_min_tokens=0)
    model.train()
    x = torch.from_numpy(g["skeleton"][:2]).to(dev)
    labels = torch.arange(2, device=dev) % 14
    ce = nn.CrossEntropyLoss()
    ran, words = [], []
    blocks = [m for m in model.modules() if isinstance(m, Block)]

    def note(mod, args):
        ran.append(mod.trains_on_hip(args[0]))
        words.append(mod._hip_flags(args[0], train=True))
    hooks = [m.register_forward_pre_hook(note) for m in blocks]
    out, _, grads = step(model, x, 5, lambda o: ce(o, labels), need_dz=False)
    for h in hooks:
        h.remove()
    assert len(ran) == 12 and all(ran), "every block reports trains_on_hip"
    assert all(w & _capi.VIT_WGRAD_SMALL and w & _capi.VIT_TILE_MASK == _capi.VIT_TILE_AUTO for w in words)
    set_force_torch(model, True)
    pinned_max.second_run()
    out_t, _, grads_t = step(model, x, 5, lambda o: ce(o, labels), need_dz=False)
    print(f"whole model {style} small logits: {parity_gate(out, out_t, REL, f'whole model {style} logits'):.3e}")
    check_stem_grads(grads, grads_t, True)
    stem = ("gcn0.", "tcn0.")
    compare_grads({k: v for k, v in grads.items() if not k.startswith(stem)},
                  {k: v for k, v in grads_t.items() if not k.startswith(stem)}, f"whole model {style} small")


# ---- 5. what must not move --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ts_spatial_L22_D512", "st_spatial_L22_D256"])
def test_with_the_switch_off_a_block_runs_the_older_pair_bit_for_bit(name, dev):
    import copy
    cpu, x, dy, _, _ = block_case(name)
    blk = copy.deepcopy(cpu).to(dev)
    blk.hip_train_min_tokens = 0
    xd, dyd = x.to(dev), dy.to(dev)
    assert blk.small_tiles_train is False
    y, g = tr.module_grads(blk, xd, dyd)
    y_direct, g_direct = run_block(blk, xd, dyd, "f32")        # stgcn_vit_block_forward_train / stgcn_vit_block_backward
    assert torch.equal(y, y_direct)
    for k, v in g_direct.items():
        assert (v is None and g[k] is None) or torch.equal(g[k], v), k


def test_the_tile_field_alone_still_moves_no_gradient_bit(dev):
    """The ST-ViT layers' entry points (the ``_drop`` pair, with masks) across STGCN_VIT_TILE_AUTO / _64 / _32 and no tile field,
    the new bit clear: the field selects forward and dgrad forms only, and those agree bit for bit."""
    from stgcn_amd import _capi
    B, L, D, seed = 7, 22, 256, 9400
    blk = seeded_block(D, seed).to(dev)
    x, dy = (t.to(dev) for t in seeded_io(B, L, D, seed))
    gen = torch.Generator(device=dev).manual_seed(seed)
    drop = tuple((torch.rand(B, L, w, device=dev, generator=gen) > 0.1).float() / 0.9 for w in (D, 2 * D, D))
    base = None
    for tile in (0, _capi.VIT_TILE_AUTO, _capi.VIT_TILE_64, _capi.VIT_TILE_32):
        y, g = drop_pair(blk, x, dy, tile, drop=drop)
        if base is None:
            base = (y, g)
            continue
        assert torch.equal(y, base[0])
        for k, v in g.items():
            assert torch.equal(v, base[1][k]), f"tile {tile:#x}: d{k}"


# ---- 6. poisoned, guard-banded buffers and a non-finite input ---------------------------------------------------------------
def make_linear_backward_small(M, K, Nout, arith, dev):
    F = hipF()
    rel, strict = GATES[arith]
    g = torch.Generator(device=dev).manual_seed(M + K + Nout + 1)
    dy = torch.randn(M, Nout, generator=g, device=dev)
    a = torch.randn(M, K, generator=g, device=dev) + 0.5
    W = (torch.rand(Nout, K, generator=g, device=dev) * 2 - 1) / K ** 0.5
    want = {"dx": (dy.double() @ W.double()).cpu(), "dW": (dy.double().T @ a.double()).cpu(), "db": dy.double().sum(0).cpu()}

    def run():
        out = dict(zip(("dx", "dW", "db"), F.vit_linear_backward(dy, a, W, math=wgrad_math(arith))))
        _, out["dW_without_db"], none = F.vit_linear_backward(dy, a, W, need_dx=False, need_db=False, math=wgrad_math(arith))
        assert none is None
        return out

    def gate(o, what):
        for k, v in o.items():
            parity_gate(v, want["dW" if k == "dW_without_db" else k], rel, f"{what} {k}", strict)
        assert torch.equal(o["dW"], o["dW_without_db"])
    return run, gate


HOSTILE = [HostileCase(f"vit_linear_backward_small-{M}x{K}x{N}-{ar_}", functools.partial(make_linear_backward_small, M, K, N, ar_), True)
           for (M, K, N) in ((1, 32, 4), (333, 160, 196), (704, 512, 512)) for ar_ in ("f32", "bf16")]


@pytest.mark.parametrize("case", HOSTILE, ids=lambda c: c.id)
def test_flagged_linear_backward_under_poisoned_guard_banded_buffers(case, dev):
    run_under_both_fills(case, dev)


@pytest.mark.parametrize("arith", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(70, 96, 100), (333, 160, 196), (704, 512, 512)], ids=lambda s: "x".join(map(str, s)))
def test_a_nan_in_one_token_reaches_what_fp64_says_it_reaches(shape, arith, dev):
    """NaN in a few columns of one token's dY row: exactly those rows of dW (all of their K entries) and those entries of db are
    non-finite in the fp64 result, and nothing else is; the token lies in the last, ragged split where there is more than one."""
    F = hipF()
    M, K, Nout = shape
    g = torch.Generator(device=dev).manual_seed(M * K + Nout)
    dy = torch.randn(M, Nout, generator=g, device=dev)
    a = torch.randn(M, K, generator=g, device=dev)
    cols = torch.tensor([0, Nout // 2 + 1, Nout - 1], device=dev)
    dy[M - 1, cols] = float("nan")
    want_w, want_b = dy.double().T @ a.double(), dy.double().sum(0)
    assert (~torch.isfinite(want_w)).all(1).sum() == 3 and (~torch.isfinite(want_b)).sum() == 3
    _, dW, db = F.vit_linear_backward(dy, a, torch.zeros(Nout, K, device=dev), need_dx=False, math=wgrad_math(arith))
    assert torch.equal(torch.isfinite(dW), torch.isfinite(want_w)), "dW: the non-finite rows are the fp64 result's"
    assert torch.equal(torch.isfinite(db), torch.isfinite(want_b)), "db"
    rel, strict = GATES[arith]
    keep = torch.isfinite(want_b)
    parity_gate(dW[keep], want_w[keep], rel, f"{shape} {arith}: the finite rows", strict)
