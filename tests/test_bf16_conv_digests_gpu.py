"""The result BITS of the two older generations of bf16 matrix-core kernels — the 128-pixel pair of csrc/tcn_bf16.hip and the
256-pixel persistent pair of csrc/stem_bf16_v4.hip (K3v4, KF4) — held to tests/golden/bf16_conv_digests.json: SHA-256 digests
recorded on an MI355X from the commit before all four moved to the one MFMA step of csrc/bf16_common.h and the 128-pixel
pair was rebuilt from one set of pieces (tests/golden/make_bf16_conv_digests.py has the cases and says why these shapes).  Every case first asserts, through the host
queries, that the kernel family it is named for is the one that runs.  A digest that moves after a toolchain change, with the
kernels untouched, is re-recorded from the fixture's commit with the maker."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_bf16_conv_digests", os.path.join(GOLDEN, "make_bf16_conv_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)
CASES = mk.cases()


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "bf16_conv_digests.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(want):
    # 9 + 2 conv shapes and 2 + 1 + 9 stem (shape, arithmetic) pairs, times the flag sets of their families
    assert len(CASES) == 9 * 2 * 3 + 2 * 2 * 6 + (2 * 2 + 1 + 9) * 5 == 148
    assert set(want["digests"]) == {c["id"] for c in CASES}
    assert want["commit"] and want["device"] and want["rocm"]
    for family in mk.FAMILIES:
        flags = {(c["math"], c["flags"]) for c in CASES if c["family"] == family}
        assert {m for m, _ in flags} == set(mk.MATHS), family
        assert any(f & mk.OUT_BF16 for _, f in flags), family


def test_flags_and_arithmetics_of_one_shape_do_not_share_a_digest(want):
    """The cases of one shape differ in arithmetic, result type, activation or layout of the input's or the result's memory.
    Only a channels-last input leaves the result as it was (the same values, read from another layout); every other pair
    differs, so a launcher that drops a flag or hands a call to the other arithmetic shows here."""
    by_shape = {}
    for c in CASES:
        by_shape.setdefault((c["family"], c["Cin"], c["Cout"], c["T"], c["V"], c["K"], c["stride"]), []).append(c)
    for group in by_shape.values():
        seen = {}
        for c in group:
            key = want["digests"][c["id"]]
            other = seen.setdefault(key, c)
            assert other is c or (other["math"] == c["math"] and (other["flags"] ^ c["flags"]) == mk.IN_NTVC), \
                f"{other['id']} and {c['id']} share a digest"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_result_bits(case, want):
    from stgcn_amd import _capi
    assert case["id"] in want["digests"], "a case without a recorded digest"
    mk.check_family(case, _capi.lib())
    got = mk.digest(mk.run(case, torch.device("cuda:0")))
    assert got == want["digests"][case["id"]], f"{case['id']}: the result bits moved (recorded from {want['commit'][:7]} on {want['device']})"
