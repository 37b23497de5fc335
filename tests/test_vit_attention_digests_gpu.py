"""The result BITS of the heads' attention entry points on their own, held to tests/golden/vit_attention_digests.json: SHA-256
digests recorded on an MI355X from the commit before the attention kernels were rebuilt from the shared pieces of
csrc/vit_attention_common.h (tests/golden/make_vit_attention_digests.py has the cases and says why these sizes).  A digest that
moves after a toolchain change, with the kernels untouched, is re-recorded from the fixture's commit with the maker."""
import importlib.util
import itertools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_vit_attention_digests", os.path.join(GOLDEN, "make_vit_attention_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)
CASES = mk.cases()


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "vit_attention_digests.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(want):
    assert len(CASES) == 2 * (12 * 5 + 7 * 2) == 148
    assert set(want["digests"]) == {c["id"] for c in CASES}
    assert want["commit"] and want["device"] and want["rocm"]


def test_no_two_arithmetics_of_one_shape_share_a_digest(want):
    """The three arithmetics of the resident forward (fp32, bf16 storage, fp32 storage with bf16 operands) differ pairwise at
    every (L, head_dim), and so do the two of the resident backward: a launcher that hands a call to another arithmetic's
    kernel shows here.  The streaming kernels are the fp32 arithmetic in another summation order, which is the resident
    kernels' own order wherever one stage of 64 keys holds the sequence: they are not compared with them."""
    d = want["digests"]
    for group in (mk.FORWARD, mk.BACKWARD):
        for hd in mk.HEAD_DIMS:
            for L in mk.RESIDENT_L:
                ids = [f"{e}-L{L}-hd{hd}" for e in group if e in mk.RESIDENT]
                assert len(ids) >= 2
                for a, b in itertools.combinations(ids, 2):
                    assert d[a] != d[b], f"{a} and {b} share a digest"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_result_bits(case, want):
    assert case["id"] in want["digests"], "a case without a recorded digest"
    got = mk.digest(mk.run(case, torch.device("cuda:0")))
    assert got == want["digests"][case["id"]], f"{case['id']}: the result bits moved (recorded from {want['commit'][:7]} on {want['device']})"
