"""GPU tests of the split attention kernel (vit_attention_split.hip: a workgroup per (sequence, head, 32 queries), a wave per
tile of 32 keys, the waves' partial soft-maxes merged through LDS) and of what runs it: ``stgcn_vit_attention_split``,
``stgcn_vit_block_forward`` with ``STGCN_VIT_ATTN_SPLIT``, and ``set_low_latency(model, split_attention=True)``.  References are
fp64 (tests/altformer_ref.py), the gate is the resident kernel's: 1e-4, both criteria of ``parity_gate``, with one exception
that test 3 explains."""
import functools

import pytest
import torch

import altformer_ref as ar
from _util import MATH_GATES, hostile_allocations, load_golden, parity_gate, sub_state
from entry_points import peaked_qkv

pytestmark = pytest.mark.gpu
REL = MATH_GATES["f32"][0]
assert REL == 1e-4 and MATH_GATES["f32"][1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def attention_case(B, L, heads, hd, scale):
    """Input and fp64 reference of one attention case: computed once, shared by the tests that use it, never written to."""
    qkv = peaked_qkv(B, L, heads, hd, 100 * L + hd)
    return qkv, ar.attention64(qkv, heads, hd ** -0.5 if scale is None else scale)


# ---- 1. the entry point against fp64 -------------------------------------------------------------------------------------
# 1 / 31 / 32: one tile (the merge is the identity); 33, 65, 161, 225: the last tile has one live key; 64, 96, 224, 256: no
# masked key; 180 is the heads' temporal stage; 255 / 256 are eight tiles.
LENGTHS = (1, 31, 32, 33, 64, 65, 96, 161, 180, 224, 225, 255, 256)


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", LENGTHS)
def test_split_entry_point_vs_fp64(L, hd, dev):
    from stgcn_amd import functional as F
    B, heads = 3, 8
    assert F.vit_attention_split_supported(L, heads, hd)
    for scale in (None, 0.37):
        qkv, want = attention_case(B, L, heads, hd, scale)
        out = F.vit_attention_split(qkv.to(dev), heads, scale)
        assert out.shape == (B, L, heads * hd) and out.dtype == torch.float32
        rel = parity_gate(out, want, REL, f"split attention L={L} hd={hd} scale={scale}")
        print(f"split attention B={B} L={L} heads={heads} hd={hd} scale={scale}: {rel:.3e}")


# ---- 2. split against resident -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [33, 180, 256])
def test_split_agrees_with_resident(L, hd, dev):
    from stgcn_amd import functional as F
    heads = 8
    qkv, want = attention_case(3, L, heads, hd, None)
    qd = qkv.to(dev)
    res, split = F.vit_attention(qd, heads), F.vit_attention_split(qd, heads)
    parity_gate(res, want, REL, f"resident L={L} hd={hd} vs fp64")
    parity_gate(split, want, REL, f"split L={L} hd={hd} vs fp64")
    dist = (split.double() - res.double()).abs().max().item() / want.abs().max().item()
    print(f"L={L} hd={hd}: split vs resident {dist:.3e} of max|ref| (diagnostic)")


# ---- 3. the merge, on planted scores -------------------------------------------------------------------------------------
PLANTED_HD, PLANTED_B, PLANTED_HEADS = 64, 2, 4


def planted_profile(case, L):
    j = torch.arange(L, dtype=torch.float32)
    if case == "rising":       # every tile has a larger maximum than the one before: every f_w but the last underflows or is tiny
        return -60 + 120 * j / (L - 1)
    if case == "falling":      # the first tile holds the maximum, later tiles contribute exp(-large)
        return 60 - 120 * j / (L - 1)
    prof = torch.full((L,), -100.0)
    prof[L - 1 if case == "spike_last" else 0] = 100.0
    return prof


@functools.lru_cache(maxsize=None)
def planted_case(case, L):
    """q = 8 u + noise and k_j = profile[j] / (8 scale) u + noise along one seeded unit vector u per head: the score of key j is
    profile[j] for every query, up to noise of a few tenths.  v is plain noise."""
    B, heads, hd = PLANTED_B, PLANTED_HEADS, PLANTED_HD
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(4242)
    u = torch.randn(heads, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    prof = planted_profile(case, L)
    qkv = torch.empty(B, L, 3, heads, hd)
    qkv[:, :, 0] = 8.0 * u + 0.01 * torch.randn(B, L, heads, hd, generator=g)
    qkv[:, :, 1] = (prof / (8.0 * scale))[None, :, None, None] * u + 0.01 * torch.randn(B, L, heads, hd, generator=g)
    qkv[:, :, 2] = torch.randn(B, L, heads, hd, generator=g)
    s = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0].double(), qkv[:, :, 1].double()) * scale
    qkv = qkv.reshape(B, L, 3 * heads * hd)
    return qkv, s, ar.attention64(qkv, heads, scale)


@pytest.mark.parametrize("case", ["rising", "falling", "spike_last", "spike_first"])
@pytest.mark.parametrize("L", [180, 161])
def test_merge_on_planted_scores(L, case, dev):
    """The ramps are gated by the max-norm criterion alone: with scores of magnitude 60 a plain single-pass fp32 soft-max,
    without any split, reaches 1.2 x the mixed allclose criterion on these inputs (measured on the CPU; the same at +-46), so
    that criterion would test the inputs.  Its max-norm error and that of an fp32 emulation of this merge are the same, at
    most 1.6e-5, six times inside the gate.  The spikes are exact in both forms and keep both criteria."""
    from stgcn_amd import functional as F
    qkv, s, want = planted_case(case, L)
    lo, hi = s.min(dim=-1).values, s.max(dim=-1).values
    ramp = case in ("rising", "falling")
    if ramp:                                     # about -60 .. +60 for every query: exp(range) overflows fp32 without the rescale
        assert (hi - lo).min().item() > 89 and hi.min().item() > 50 and lo.max().item() < -50, (lo.max().item(), hi.min().item())
        tiles = [s[..., t:t + 32].max(dim=-1).values for t in range(0, L, 32)]
        steps = [(b - a) if case == "rising" else (a - b) for a, b in zip(tiles, tiles[1:])]
        assert all(d.min().item() > 0 for d in steps), "every tile has another maximum"
    else:                                        # exp(89) > fp32 max
        assert hi.min().item() > 89 and lo.max().item() < -89, (lo.max().item(), hi.min().item())
        at = s.argmax(dim=-1)
        assert bool((at == (L - 1 if case == "spike_last" else 0)).all())
    assert torch.isfinite(want).all() and want.abs().max().item() > 0.5, "the fp64 reference itself"
    out = F.vit_attention_split(qkv.to(dev), PLANTED_HEADS)
    assert torch.isfinite(out).all()
    print(f"planted {case} L={L}: {parity_gate(out, want, REL, f'planted scores, {case}, L={L}', strict=not ramp):.3e}")


# ---- 4. bit-identical reruns ---------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(dev):
    from stgcn_amd import functional as F
    qkv, _ = attention_case(3, 180, 8, 64, None)
    qd = qkv.to(dev)
    assert torch.equal(F.vit_attention_split(qd, 8), F.vit_attention_split(qd, 8))


# ---- 5. many workgroups --------------------------------------------------------------------------------------------------
def test_many_workgroups(dev):
    """4097 * 8 pairs of 2 query tiles = 65,552 workgroups, past the 65,535 that a grid's y and z dimensions (and 16-bit index
    arithmetic) stop at."""
    from stgcn_amd import functional as F
    B, L, heads, hd = 4097, 33, 8, 32
    g = torch.Generator(device=dev).manual_seed(B + L)
    qkv = torch.randn(B, L, 3, heads, hd, generator=g, device=dev)
    qkv[:, :, :2] *= 2.3
    qkv = qkv.reshape(B, L, 3 * heads * hd)
    out = F.vit_attention_split(qkv, heads)
    idx = ar.sample_idx(B, 64, 77).long()
    idx[0], idx[1] = 0, B - 1                    # the first and the last workgroups are in the sample
    want = ar.attention64(qkv[idx.to(dev)].cpu(), heads, hd ** -0.5)
    print(f"many workgroups: {parity_gate(out[idx.to(dev)], want, REL, 'many workgroups'):.3e}")
    assert torch.isfinite(out).all()


# ---- 6. buffer discipline ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("L", [33, 180])
def test_split_under_poisoned_guard_banded_buffers(L, hd, dev):
    """Input and output between 1 MiB guard bands, everything pre-filled with NaN bytes, then with huge finite values: the guards
    stay intact, every element of ``out`` is written and equals the run on plain buffers bit for bit (a read past the end of
    qkv, or of a key past L, would bring the poison in), and qkv is unchanged."""
    from stgcn_amd import functional as F
    B, heads = 3, 8
    qkv, want = attention_case(B, L, heads, hd, None)
    plain = F.vit_attention_split(qkv.to(dev), heads)
    parity_gate(plain, want, REL, f"plain buffers L={L} hd={hd}")
    for fill in (0xFF, 0x7F):
        with hostile_allocations(fill) as h:
            qd = torch.empty(qkv.shape, device=dev, dtype=torch.float32)
            qd.copy_(qkv)
            out = F.vit_attention_split(qd, heads)
            torch.cuda.synchronize()
            h.check()
            assert [r[2] for r in h.records][:2] == [(B, L, 3 * heads * hd), (B, L, heads * hd)], "qkv and out are guard-banded"
        assert torch.isfinite(out).all(), f"fill 0x{fill:02X}: an element of out was not written, or poison was read"
        assert torch.equal(out, plain), f"fill 0x{fill:02X}: the result depends on what surrounds the buffers"
        assert torch.equal(qd.cpu(), qkv), "qkv was written to"


# ---- 7. the block entry point --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(shape, dev):
    """State, input and the fp64 restatement (on the device)."""
    B, L, D, heads, hidden = shape
    sd = ar.random_block_state(D, hidden, True, seed=B + L + D)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, D, generator=g) * (0.25 + 3.75 * torch.rand(B, L, 1, generator=g)) + torch.randn(B, L, 1, generator=g)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    want = ar.block64(x.to(dev), sdd, heads=heads)[0].cpu()
    pair = lambda n: (sdd[n + ".weight"], sdd[n + ".bias"])       # noqa: E731
    return x.to(dev), want, (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))


@pytest.mark.parametrize("mode", ["f32", "mixed"])
@pytest.mark.parametrize("shape", [(1, 180, 512, 8, 1024), (2, 46, 512, 8, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_block_with_the_flag_vs_fp64_and_the_unflagged_call(shape, mode, dev):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    B, L, D, heads, hidden = shape
    math = HEAD_MATH[mode]
    assert F.vit_block_attention_form(B, L, D, heads, hidden, math | F.VIT_ATTN_SPLIT) == "resident_split"
    assert F.vit_block_attention_form(B, L, D, heads, hidden, math) == "resident"
    xd, want, params = block_case(shape, dev)
    scale = (D // heads) ** -0.5
    plain = F.vit_block_forward(xd, *params, heads, ar.EPS, scale, math)
    split = F.vit_block_forward(xd, *params, heads, ar.EPS, scale, math | F.VIT_ATTN_SPLIT)
    assert not torch.equal(split, plain), "the flag changed nothing: the split kernel did not run"
    print(f"block {shape} {mode}: split vs fp64 {parity_gate(split, want, REL, f'block {shape} {mode}, split, vs fp64'):.3e}, "
          f"vs the unflagged call {parity_gate(split, plain, REL, f'block {shape} {mode}, split vs unflagged'):.3e}")
    assert torch.equal(split, F.vit_block_forward(xd, *params, heads, ar.EPS, scale, math | F.VIT_ATTN_SPLIT)), "two runs differ"


@pytest.mark.parametrize("shape", [(32, 180, 512, 8, 1024), (1, 22, 512, 8, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_block_where_the_flag_changes_nothing(shape, dev):
    """From kAttentionSplitPairs pairs on, and at one key tile, the flagged call runs the resident kernel: bit for bit."""
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import HEAD_MATH
    B, L, D, heads, hidden = shape
    math = HEAD_MATH["mixed"]
    assert F.vit_block_attention_form(B, L, D, heads, hidden, math | F.VIT_ATTN_SPLIT) == "resident"
    g = torch.Generator().manual_seed(L)
    sd = {k: v.to(dev) for k, v in ar.random_block_state(D, hidden, True, seed=B + L + D).items()}
    pair = lambda n: (sd[n + ".weight"], sd[n + ".bias"])       # noqa: E731
    params = (pair("norm1"), pair("attn.qkv"), pair("attn.proj"), pair("norm2"), pair("mlp.fc1"), pair("mlp.fc2"))
    xd = torch.randn(B, L, D, generator=g).to(dev)
    scale = (D // heads) ** -0.5
    plain = F.vit_block_forward(xd, *params, heads, ar.EPS, scale, math)
    assert torch.isfinite(plain).all()
    assert torch.equal(F.vit_block_forward(xd, *params, heads, ar.EPS, scale, math | F.VIT_ATTN_SPLIT), plain)


# ---- 8. the module at one clip -------------------------------------------------------------------------------------------
def _model(style, dev):
    import stgcn_amd
    g = load_golden("model_altformer_shre")
    torch.manual_seed(int(g["model_seed"]))
    model = stgcn_amd.ST_GCN_AltFormer(channel=3, num_class=14, num_frame=180, num_joints=22, style=style, graph="graph.SHRE",
                                       graph_args={"labeling_mode": "spatial"})
    model.gcn0.load_state_dict(sub_state(g, "gcn."), strict=True)
    model.tcn0.load_state_dict(sub_state(g, "tcn."), strict=True)
    model = model.to(dev).eval()
    model.gcn0.A = torch.from_numpy(g["A_fixed"]).clone()
    return model, torch.from_numpy(g["skeleton"]).to(dev)


def _run_recording(model, x):
    from stgcn_amd import functional as F
    from stgcn_amd.altformer import Block
    calls = []

    def record(mod, args):
        x = args[0]
        form = F.vit_block_attention_form(x.shape[0], x.shape[1], x.shape[2], mod.attn.num_heads, mod.mlp.fc1.out_features,
                                          mod._hip_flags(x, train=False))
        calls.append((mod.uses_hip(x), (x.shape[1], form)))
    hooks = [m.register_forward_pre_hook(record) for m in model.modules() if isinstance(m, Block)]
    with torch.no_grad():
        out = model(x)
    for h in hooks:
        h.remove()
    return out, calls


@pytest.mark.parametrize("style", ["ST", "TS"])
def test_one_clip_with_split_attention(style, dev):
    import stgcn_amd
    from stgcn_amd.altformer import Block
    model, clips = _model(style, dev)
    stgcn_amd.set_low_latency(model, min_tokens=0, split_attention=True)
    with torch.no_grad():
        clip = clips[:1].contiguous()
        a, calls = _run_recording(model, clip)
        assert len(calls) == 12 and all(on for on, _ in calls), "every block on the HIP path"
        forms = sorted({f for _, f in calls})
        assert forms == [(22, "resident"), (180, "resident_split")], \
            f"the temporal blocks (180 frames) split, the spatial ones (22 joints, one key tile) do not: {forms}"
        assert sum(f == (180, "resident_split") for _, f in calls) >= 4
        b, _ = _run_recording(model, clip)
        assert torch.equal(a, b), "two runs differ"
        eager = [a] + [model(clips[i:i + 1].contiguous()).clone() for i in (1, 2)]
        static_in = clips[:1].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = model(static_in)
        for i in (1, 2):
            static_in.copy_(clips[i:i + 1])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, eager[i]), f"{style}: replay with clip {i} differs from the eager result"
        assert not torch.equal(eager[1], eager[2])
        for m in model.modules():
            if isinstance(m, Block):
                m.force_torch = True
        t, calls = _run_recording(model, clip)
        assert not any(on for on, _ in calls)
    print(f"{style} one clip, split attention vs torch path: {parity_gate(a, t, REL, f'{style} one clip, split attention'):.3e}")
    assert torch.equal(a.argmax(1), t.argmax(1))
