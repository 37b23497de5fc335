"""Non-finite inputs stay non-finite through every HIP path: the cases of tests/nonfinite_cases.py (its docstring states the
contract, (a) nothing hidden, (b) nothing leaked, (c) what a planted Inf owes under the split arithmetics) run on the GPU,
``stgcn_step_stats`` on a poisoned stem output and on logits with NaN rows, and the kernels the plans can name are all reached.

Out of scope: non-finite parameters (the prepacked blobs and their restaging are a topic of their own) and the
eval-with-gradients backward."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import stgcn_amd
    stgcn_amd.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", nc.CASES, ids=lambda c: c.id)
def test_one_planted_value_is_neither_hidden_nor_leaked(case, dev):
    prep = case.prepare()
    run = prep.on(dev)
    clean = run(prep.x)
    for name, t in clean.items():
        assert bool(torch.isfinite(t.float()).all()), f"{case.id}: {name} of the clean input is not finite"
    failures = []
    for label, index, value in case.plants():
        what = f"{case.id} {value}@{label}{index}"
        xp = nc.plant(prep.x, index, value)
        try:
            nc.check(case, prep, index, value, run(xp), prep.reference(xp), what)
        except AssertionError as e:              # every plant is reported, not only the first
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(case.plants())} plants fail:\n" + "\n".join(failures)


def test_cases_reach_every_kernel_the_plans_can_name():
    from entry_points import STEM_KERNELS, TCN_KERNELS, hipF
    F = hipF()
    assert {c.kernel for c in nc.CASES if c.id.startswith("tcn-")} == TCN_KERNELS
    assert {c.kernel for c in nc.CASES if c.id.startswith("stem_fused-")} == STEM_KERNELS
    agcn = [tuple(map(int, c.id.split("-")[1].split("x"))) for c in nc.CASES if c.id.startswith("agcn-")]
    attention = {F.agcn_attention_kernel_name(N, cin, T, V, cout // 4, 3).split("<")[0] for N, cin, cout, T, V in agcn}
    expand = {F.agcn_expand_kernel_name(N, cin, cout, T, V, 3, cin != cout).split("<")[0] for N, cin, cout, T, V in agcn}
    assert attention == {"attention_folded_kernel", "attention_generic_mfma_kernel", "attention_generic_kernel"}, attention
    assert expand == {"agcn_expand_small4_kernel", "agcn_expand_small_kernel", "agcn_expand_mfma_kernel", "agcn_expand_generic_kernel"}, expand
    forms = {F.vit_block_attention_form(int(b), int(l), 256, 8, 512) for b, l in
             (c.id.split("-")[1].split("x")[:2] for c in nc.CASES if c.id.startswith("vit_block_train-"))}
    assert "stream" in forms and "resident" in forms, forms


# ---- stgcn_step_stats ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", sorted(nc.VALUES))
@pytest.mark.parametrize("n,c", [(0, 0), (4, 127), (2, 5)])
def test_step_stats_reads_a_poisoned_probe_as_non_finite(n, c, value, dev):
    """The health probe sums out[n, c, 0, 0] and its square: a non-finite probed element makes both non-finite."""
    from stgcn_amd import dist as sd
    out = torch.relu(torch.randn(5, 128, 3, 22, generator=torch.Generator().manual_seed(3)))
    stats = sd.step_stats(out.to(dev), 5).cpu()
    probe = out[:, :, 0, 0].double()
    assert torch.allclose(stats[1:3].double(), torch.tensor([probe.sum().item(), probe.square().sum().item()], dtype=torch.float64),
                          rtol=1e-5, atol=1e-3)
    stats = sd.step_stats(nc.plant(out, (n, c, 0, 0), value).to(dev), 5).cpu()
    print(f"step_stats with {value} at ({n},{c},0,0): {stats.tolist()}")
    assert not torch.isfinite(stats[1]) and not torch.isfinite(stats[2]) and float(stats[0]) == 5


def test_step_stats_predictions_on_nan_rows_are_torch_argmax(dev):
    """Pins what argmax_row does: a row that holds a NaN predicts the first NaN's column, as torch.argmax (and np.argmax)."""
    from stgcn_amd import dist as sd
    n, classes = 40, 14
    gen = torch.Generator().manual_seed(9)
    logits = torch.randn(n, classes, generator=gen)
    logits[1, :] = nc.VALUES["nan"]
    logits[2, classes - 1] = nc.VALUES["nan"]
    logits[3, 0] = nc.VALUES["nan_ones"]
    logits[4, 5], logits[4, 9] = nc.VALUES["nan_ones"], nc.VALUES["nan"]
    logits[5, 3], logits[5, 4] = float("inf"), nc.VALUES["nan"]
    logits[6, :] = float("-inf")
    logits[n - 1, 7] = nc.VALUES["nan"]
    want = torch.argmax(logits, dim=1)
    assert np.array_equal(want.numpy(), np.argmax(logits.numpy(), axis=1))
    assert want[[1, 2, 3, 4, 5, n - 1]].tolist() == [0, classes - 1, 0, 5, 4, 7]
    labels = want.clone()
    labels[::3] = (labels[::3] + 1) % classes
    out = torch.randn(n, 4, 2, 3, generator=gen).to(dev)
    pred = torch.full((n,), -1, dtype=torch.int64, device=dev)
    stats = sd.step_stats(out, n, logits.to(dev), labels.to(dev), pred).cpu()
    assert torch.equal(pred.cpu(), want)
    assert float(stats[3]) == float((want == labels).sum())
