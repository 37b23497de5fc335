"""The result BITS of the heads' block entry points, held to tests/golden/vit_block_digests.json: SHA-256 digests recorded on
an MI355X from the commit before the block's host code was moved behind one plan (tests/golden/make_vit_block_digests.py has
the cases and says why these sizes).  The suite's 1e-4 / 1e-2 gates pass a refactor that hands the qkv linear's arithmetic to
another linear; a digest does not.  A digest that moves after a toolchain change, with the host code untouched, is re-recorded
from the fixture's commit with the maker."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_vit_block_digests", os.path.join(GOLDEN, "make_vit_block_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)
CASES = mk.cases()


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "vit_block_digests.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(want):
    assert set(want["digests"]) == {c["id"] for c in CASES} and len(CASES) == 62
    assert want["commit"] and want["device"] and want["rocm"]
    refused = [k for k, v in want["digests"].items() if v == mk.UNSUPPORTED]
    assert sorted(refused) == sorted(c["id"] for c in CASES if c["kind"] == "forward" and c["flags"] & mk.BF16 and c["L"] > 256)
    assert len(refused) == 2, "VIT_BF16 at L = 300 is refused with STGCN_ERR_UNSUPPORTED, everything else runs"
    assert len(set(want["digests"].values())) >= 40, "tile forms agree bit for bit; arithmetics and shapes do not"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_result_bits(case, want):
    assert case["id"] in want["digests"], "a case without a recorded digest"
    got = mk.digest(mk.run(case, torch.device("cuda:0")))
    assert got == want["digests"][case["id"]], f"{case['id']}: the result bits moved (recorded from {want['commit'][:7]} on {want['device']})"
