"""What makes the stream contract's cases (tests/stream_order.py) mean something, without a GPU.

1. A decoy that cannot pass: for every case and every compared output, reference(decoy) is further than ten times the
   output's gate from reference(clean), on the gate's own scale (rel * max|reference(clean)|).  A result computed from the
   stale input - or, being linear in it or worse, from half of it - then cannot pass the GPU file's comparison.  The figures
   are printed.
2. Coverage: every function of include/stgcn_hip.h with a ``void *stream`` parameter is reached by a named case of the table
   or listed in ``COVERED_THROUGH`` with its covering case and a reason; the GPU file backs the declared symbols by recording
   what each case really calls."""
import pytest
import torch

import stream_order as so

FACTOR = 10


@pytest.mark.parametrize("case", so.CASES, ids=lambda c: c.id)
def test_the_decoy_is_far_from_the_clean_reference(case):
    prep = case.prepare()
    clean = prep.reference(prep.x)          # first: a kink-free cotangent is drawn from the clean reference and kept
    d = so.decoy(prep.x)
    assert d.shape == prep.x.shape and bool(torch.isfinite(d).all()) and not torch.equal(d, prep.x)
    other = prep.reference(d)
    assert set(case.no_dependence) <= set(clean), f"{case.id}: no_dependence names outputs the reference does not have"
    rows = so.distances(case, clean, other, prep)
    assert rows, f"{case.id}: no output is compared"
    for name, dist, gate in rows:
        print(f"{case.id} {name}: |reference(decoy) - reference(clean)| = {dist:.3e}, gate {gate:.3e}, ratio {dist / gate:.1f}")
    for name, reason in case.no_dependence.items():
        print(f"{case.id} {name}: not compared ({reason})")
    near = [f"{name}: {dist:.3e} <= {FACTOR} x {gate:.3e}" for name, dist, gate in rows if not dist > FACTOR * gate]
    assert not near, f"{case.id}: the decoy's reference is within {FACTOR} gates of the clean one: " + "; ".join(near)


def test_every_stream_taking_entry_point_is_accounted_for():
    entry_points = so.stream_entry_points()
    assert len(entry_points) >= 40 and "stgcn_agcn_forward" in entry_points and "stgcn_version" not in entry_points
    ids = {c.id for c in so.CASES}
    reached = {}
    for c in so.CASES:
        for s in c.symbols:
            reached.setdefault(s, []).append(c.id)
    missing = []
    for name in entry_points:
        if name in reached:
            print(f"{name}: reached by {', '.join(reached[name][:3])}" + (" ..." if len(reached[name]) > 3 else ""))
        elif name in so.COVERED_THROUGH:
            through, reason = so.COVERED_THROUGH[name]
            assert through in ids and reason, f"{name}: covered through {through!r}, which is no case"
            print(f"{name}: covered through {through} ({reason})")
        else:
            missing.append(name)
    assert not missing, f"stream-taking entry points with no case and no reason: {missing}"
    unknown = (set(reached) | set(so.COVERED_THROUGH)) - set(entry_points)
    assert not unknown, f"names that are no stream-taking entry point of the header: {sorted(unknown)}"
    assert not set(reached) & set(so.COVERED_THROUGH), "an entry point is either reached or listed"


def test_the_small_block_row_reaches_the_64_form_and_more_than_one_split():
    """230 tokens at D = 256 under VIT_WGRAD_SMALL: stgcn_vit_wgrad_tile picks the 64 x 64 form, the qkv product has two splits."""
    import entry_points as ep
    (tile, _, _), (tile_qkv, splits_qkv, _) = ep.vit_block_train_small(5, 46, 256, "f32").plans(ep.hipF())
    print(f"vit_block_train_small-5x46x256: D x D tile {tile}; qkv tile {tile_qkv}, {splits_qkv} splits")
    assert tile == 64 and tile_qkv == 64 and splits_qkv > 1


def test_the_exempt_list_is_short_and_reasoned():
    assert len(so.EXEMPT) <= 3 and all(so.EXEMPT.values())
    families = {c.id.split("-")[0] for c in so.CASES}
    assert not {i.split("-")[0] for i in so.EXEMPT} - families, "an exemption removed a whole family"


def test_the_hold_is_four_times_the_slowest_enqueue():
    assert so.HOLD_MS >= 4 * so.SLOWEST_ENQUEUE_MS
