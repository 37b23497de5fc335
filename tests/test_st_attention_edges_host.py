"""Host-side conditions on st_attention_ref.EDGE_CASES, the inputs of tests/test_st_attention_edges_gpu.py.  No GPU.

The GPU tests hold the kernels to 1e-4 of max|fp64| at shapes chosen to be edges.  That gate means something only if the
inputs are well conditioned - plain fp32 arithmetic, with no kernel involved, stays far inside it - and if each case is the edge
it is named for.  Both are asserted here, so that a failing GPU test points at the kernel, not at its inputs."""
import functools

import pytest
import torch

import st_attention_ref as R

NAMES = [c["name"] for c in R.EDGE_CASES]
FP32_BOUND = 2.5e-5          # a quarter of the project's 1e-4 gate: a condition on the inputs, not a measurement of a kernel
ZERO_GRAD = ("attention_conv.attn_out.bias",)     # analytically 0 behind a batch-statistics BatchNorm


@functools.lru_cache(maxsize=None)
def _fp64(name):
    aux = {}
    return R.edge_grads(R.edge_case(name), aux=aux), aux


def _ratio(a, ref):
    return float((a.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_restatement_is_within_a_quarter_of_the_gate(name):
    """y, dx and every parameter gradient of the restatement run in fp32 lie within 2.5e-5 of max|fp64|."""
    c = R.edge_case(name)
    (y, _, g, dx), _ = _fp64(name)
    y32, _, g32, dx32 = R.edge_grads(c, dtype=torch.float32)
    fig = {"y": _ratio(y32, y), "dx": _ratio(dx32, dx)}
    for k in g:
        if not (k in ZERO_GRAD and c["mode"] == "batch"):
            fig[k] = _ratio(g32[k], g[k])
    worst = max(fig, key=fig.get)
    print(f"{name}: fp32 restatement y {fig['y']:.2e} dx {fig['dx']:.2e} worst {worst} {fig[worst]:.2e}")
    assert torch.isfinite(y32).all() and torch.isfinite(dx32).all()
    for k, v in fig.items():
        assert v <= FP32_BOUND, f"{name}: fp32 restatement of {k} is {v:.2e} of max|fp64| (> {FP32_BOUND:g})"


@pytest.mark.parametrize("name", [c["name"] for c in R.EDGE_CASES if c["V"] <= 3 and c["drop"]])
def test_small_v_cases_have_all_zero_mask_blocks(name):
    """At least 10 % of the (frame, head) blocks of the drop-connect mask are all zero: ss = 0, 1 / (ss + 1e-8) = 1e8."""
    c = R.edge_case(name)
    mask = R.edge_inputs(c)[3].reshape(-1, c["V"])
    assert mask.shape[0] == c["N"] * c["T"] * c["nh"]
    empty = int((mask.sum(1) == 0).sum())
    print(f"{name}: {empty} of {mask.shape[0]} mask blocks are all zero")
    assert empty >= 0.1 * mask.shape[0]
    assert empty < mask.shape[0]                     # and some are not: both branches of the normalisation


@pytest.mark.parametrize("name", ["sharp", "sharp_mask"])
def test_sharp_cases_overflow_exp_without_the_row_maximum(name):
    """At least 100 query rows have a maximal logit above 88.8: exp of it is inf in fp32 unless the maximum is subtracted."""
    _, aux = _fp64(name)
    top = aux["logits"].amax(-1).reshape(-1)
    spread = (aux["logits"].amax(-1) - aux["logits"].amin(-1)).max()
    rows = int((top > R.EXP_OVERFLOW_F32).sum())
    print(f"{name}: {rows} of {top.numel()} rows above {R.EXP_OVERFLOW_F32}, logits {float(aux['logits'].min()):.0f} .. "
          f"{float(aux['logits'].max()):.0f}, largest row spread {float(spread):.0f}")
    assert rows >= 100
    assert not torch.isfinite(torch.exp(aux["logits"].float())).all()


def test_chunks_case_takes_more_than_one_batchnorm_chunk():
    """More than 8192 elements per channel (bn_chunks() > 1), clips not a multiple of the chunk count (uneven chunks)."""
    c = R.edge_case("chunks")
    per_channel = c["N"] * c["T"] * c["V"]
    chunks = min(-(-per_channel // 8192), -(-1024 // c["cout"]), c["N"], 64)       # bn_chunks(N, T*V, Cout) for < 64 K elements
    assert per_channel > 8192 and chunks > 1 and c["N"] % chunks != 0


def test_split_cases_cover_exact_uneven_and_empty_splits():
    """cv_splits(N) = min(N, 16) with per = ceil(N / splits) clips each: (used, empty) splits of the three N > 15 cases."""
    got = {}
    for name in ("n16", "n17", "n33"):
        N = R.edge_case(name)["N"]
        splits = min(N, 16)
        per = -(-N // splits)
        used = -(-N // per)
        got[name] = (per, used, splits - used)
    assert got == {"n16": (1, 16, 0), "n17": (2, 9, 7), "n33": (3, 11, 5)}


def test_head_cases_cover_every_width_pair_off_eight_heads():
    pairs = {(c["cout"] // 4 // c["nh"], c["cout"] // c["nh"]) for c in R.EDGE_CASES if c["nh"] != 8}
    assert pairs == {(4, 16), (8, 32), (16, 64)}
    for c in R.EDGE_CASES:
        assert (c["cout"] // 4 // c["nh"], c["cout"] // c["nh"]) in {(4, 16), (8, 32), (16, 64)}, c["name"]
        assert c["V"] <= 64 and not (c["mode"] == "batch" and c["N"] * c["T"] < 4), c["name"]
