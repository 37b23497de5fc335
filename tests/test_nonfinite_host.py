"""The non-finite contract's case table (tests/nonfinite_cases.py) is meaningful - no GPU.  For every case and every plant: the
reference of the clean input is finite, the reference of the planted input has a non-finite element, and a case that claims
"nothing leaked" (b) has something finite left to leak into: a finite element inside a touched unit, or a wholly finite unit.
A case that fails here is a bug in the table.

Out of scope of the contract (and of both files): non-finite parameters, and the eval-with-gradients backward."""
import pytest
import torch

import nonfinite_cases as nc


def test_planted_values_are_the_exact_bits():
    x = torch.zeros(2, 3)
    assert nc.plant(x, (1, 2), "nan_ones").view(torch.int32)[1, 2].item() == -1
    assert nc.plant(x, (0, 0), "nan").view(torch.int32)[0, 0].item() == 0x7FC00000
    assert nc.plant(x, (0, 1), "+inf")[0, 1].item() == float("inf") and nc.plant(x, (0, 1), "-inf")[0, 1].item() == float("-inf")
    assert not x.any(), "plant writes to a copy"


def test_the_table_covers_what_the_contract_names():
    families = {c.id.split("-")[0] for c in nc.CASES}
    assert families >= {"agcn", "tcn", "stem_fused", "stem_two_stage", "patch_embed", "st_attention", "vit_linear", "vit_attention",
                        "vit_block", "vit_pool", "vit_pool_classify", "head", "model", "agcn_train", "tcn_train", "stem_train",
                        "st_attention_train", "vit_block_train"}
    for c in nc.CASES:
        values = {v for _, _, v in c.plants()}
        assert values == set(nc.VALUES) - c.without and {"nan", "nan_ones"} <= values, c.id
        assert (c.math == "f16mx") == ({"+inf", "-inf"} <= c.without), c.id                              # f16mx: no Inf cases (c)
        assert {label for label, _, v in c.plants() if v != "nan"} == {"first", "last"}, c.id
        assert c.owes("nan") == ("a" if c.training else "full")
        assert c.owes("+inf") == ("a" if c.training else "units" if c.math in nc.SPLIT_MATHS else "full")


@pytest.mark.parametrize("case", nc.CASES, ids=lambda c: c.id)
def test_the_references_make_the_case_meaningful(case):
    prep = case.prepare()
    clean = prep.reference(prep.x)
    for label, index, value in case.plants():
        what = f"{case.id} {value}@{label}{index}"
        assert all(0 <= i < n for i, n in zip(index, prep.x.shape)) and len(index) == prep.x.dim(), what
        nc.reference_makes_sense(case, prep, index, value, clean, prep.reference(nc.plant(prep.x, index, value)), what)


@pytest.mark.parametrize("case", [c for c in nc.CASES if c.id.startswith(("model-", "head-"))], ids=lambda c: c.id)
def test_a_poisoned_clip_has_no_finite_logit_in_the_reference(case):
    """What the whole-model cases then demand of the HIP paths through (a) and (b): every logit of the poisoned clip non-finite,
    every other clip's logits finite."""
    prep = case.prepare()
    for label, index, value in case.plants():
        bad = nc.nonfinite(prep.reference(nc.plant(prep.x, index, value))["logits"])
        assert bool(bad[index[0]].all()) and int(bad.sum()) == bad.shape[1], f"{case.id} {value}@{label}"
