"""What the host code of the heads' transformer block decides (csrc/vit.h ``plan_block``, read by every block entry point and
query; ``Block._hip_flags`` on the Python side), held to tests/golden/vit_plan_parent.json, which was recorded from the commit
before those decisions were moved into one place (tests/golden/make_golden_vit_plan.py describes the three sections).  No GPU:
the status grid runs with NULL pointers or zero-byte buffers, so no call reaches a launch."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def mk():
    spec = importlib.util.spec_from_file_location("make_golden_vit_plan", os.path.join(GOLDEN, "make_golden_vit_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "vit_plan_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(mk):
    from stgcn_amd.build import build
    return mk.record(build())


def test_the_fixture_has_not_degenerated(mk, want):
    """Every entry point answers each of ARG, UNSUPPORTED and WORKSPACE somewhere on the grid and OK nowhere; the flag words are
    the nine inference and four training words the parent produced."""
    assert len(mk.status_grid()) == 960 and set(want["status"]) == set(mk.ENTRIES)
    for entry, records in want["status"].items():
        codes = [int(r.split("|")[0]) for r in records]
        assert len(codes) == 960 and 0 not in codes and {-1, -2, -3} <= set(codes), entry
        assert all(r.split("|")[1] == "1" for r in records), f"{entry}: a message without the entry point's name"
    assert len(mk.flag_grid()) == 2520 == len(want["flags"])
    train = [g[-1] for g in mk.flag_grid()]
    assert len({w for w, t in zip(want["flags"], train) if not t}) == 9
    assert len({w for w, t in zip(want["flags"], train) if t}) == 4
    assert {q: len(v) for q, v in want["queries"].items()} == {
        "stgcn_vit_block_forward_bf16_supported": 150, "stgcn_vit_block_train_bf16_supported": 150,
        "stgcn_vit_linear_bf16_supported": 4800, "stgcn_vit_linear_backward_bf16_supported": 150,
        "stgcn_vit_attention_bf16_supported": 42}
    assert all(0 < sum(v) < len(v) for v in want["queries"].values())


def test_the_queries_answer_what_the_parent_answered(got, want):
    for q in want["queries"]:
        assert got["queries"][q] == want["queries"][q], q
    assert set(got["queries"]) == set(want["queries"])


@pytest.mark.parametrize("entry", ["stgcn_vit_block_forward", "stgcn_vit_block_forward_train", "stgcn_vit_block_backward",
                                   "stgcn_vit_linear_backward"])
def test_status_and_message_tokens_of_every_flag_word(entry, mk, got, want):
    bad = [(case, g, w) for case, g, w in zip(mk.status_grid(), got["status"][entry], want["status"][entry]) if g != w]
    assert not bad, f"{entry}: {len(bad)} of 960 cases differ, first (flags, shape, pointers) = {bad[0][0]}: {bad[0][1]!r} != {bad[0][2]!r}"


def test_the_flag_word_a_block_hands_to_each_hip_path(mk, got, want):
    bad = [(case, hex(g), hex(w)) for case, g, w in zip(mk.flag_grid(), got["flags"], want["flags"]) if g != w]
    assert not bad, f"{len(bad)} of 2520 cases differ, first {bad[0]}"
