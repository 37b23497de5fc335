"""The result BITS of the graph conv's forward entry points (attention, eval forward, the fused stem's attention, training
forward), held to tests/golden/agcn_digests.json: SHA-256 digests recorded on an MI355X from the commit before the choice of
their kernels moved behind plan_attention / plan_agcn_expand (tests/golden/make_agcn_digests.py has the cases and says why
these shapes).  Both kernel families sum in a fixed order, so a host-side change must not move a bit; the two refused shapes
are held to the status and text of their refusal.  A digest that moves after a toolchain change, with the host code
untouched, is re-recorded from the fixture's commit with the maker."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_agcn_digests", os.path.join(GOLDEN, "make_agcn_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)
CASES = mk.cases()


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "agcn_digests.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(want):
    assert set(want["digests"]) == {c["id"] for c in CASES} and len(CASES) == 39
    assert want["commit"] and want["device"] and want["rocm"]
    refused = {k: v for k, v in want["digests"].items() if v.startswith("STGCN_")}
    assert sorted(refused) == ["attention-N2-3to128-T8-V65", "attention-N65536-1to4-T1-V1"]
    assert all(v.startswith("STGCN_ERR_UNSUPPORTED: attention: ") for v in refused.values())
    assert len(set(want["digests"].values())) >= 30, "shapes and entry points do not share results"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_result_bits(case, want):
    assert case["id"] in want["digests"], "a case without a recorded digest"
    got = mk.digest(mk.run(case, torch.device("cuda:0")))
    assert got == want["digests"][case["id"]], f"{case['id']}: the result moved (recorded from {want['commit'][:7]} on {want['device']})"
