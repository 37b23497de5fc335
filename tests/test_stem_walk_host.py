"""Host side of the fused stem's short last tiles (csrc/kf6.h, narrow three-term form): the run partition of the balanced walk and
the plan's rule for the short form.  No GPU: both are reached through host queries of the library.

Walk: a full tile costs 2 units and a short one (a clip's last tile, where the shape has short tiles) 1; tile L = k * tpc + r
starts at cumulative cost k * (2 tpc - short) + 2 r, and the G workgroups share the total: each takes a contiguous run of tiles
(``v6_run``, csrc/kf6.h: the run boundaries are placed by bisection on the cost).  The runs must cover every tile exactly once, in
order; with no more tiles than workgroups every workgroup gets one tile; and no two workgroups' costs differ by more than one
full tile.

Plan: ``short_last`` and the short form's producer block count against a brute-force walk of the taps."""
import ctypes

import pytest

NS = range(1, 601)
GS = (1, 8, 255, 256, 304)
TPCS = (1, 2, 16, 43)


def _runs(lib, G, N, tpc, short):
    first, end = ctypes.c_int(-1), ctypes.c_int(-1)
    out = []
    for b in range(G):
        assert lib.stgcn_stem_walk_run(b, G, N, tpc, short, ctypes.byref(first), ctypes.byref(end)) == 0
        out.append((first.value, end.value))
    return out


@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("tpc", TPCS)
@pytest.mark.parametrize("G", GS)
def test_runs_cover_every_tile_once_and_balance_the_cost(G, tpc, short):
    from stgcn_amd import _capi
    lib = _capi.lib()
    worst = (0, None)
    for N in NS:
        ntiles = N * tpc
        runs = _runs(lib, G, N, tpc, short)
        at, costs = 0, []
        for b, (first, end) in enumerate(runs):
            if b >= ntiles:                         # (the launch has min(ntiles, G) workgroups: the others get nothing)
                assert first == end == ntiles, (N, b, first, end)
                continue
            assert first == at and end >= first, f"N={N} G={G} tpc={tpc} short={short}: workgroup {b} runs [{first}, {end}), expected to start at {at}"
            at = end
            if ntiles <= G:
                assert end == first + 1, f"N={N} G={G} tpc={tpc}: {ntiles} tiles, workgroup {b} runs [{first}, {end})"
            costs.append(2 * (end - first) - (end // tpc - first // tpc if short else 0))     # (a clip's last tile costs 1)
        assert at == ntiles, f"N={N} G={G} tpc={tpc} short={short}: the runs end at tile {at} of {ntiles}"
        spread = max(costs) - min(costs)
        if spread > worst[0]:
            worst = (spread, N)
    print(f"G={G} tpc={tpc} short={short}: largest cost spread {worst[0]} units (a full tile = 2) at N={worst[1]}")
    assert worst[0] <= 2, f"G={G} tpc={tpc} short={short}: costs differ by {worst[0]} units at N={worst[1]} (one full tile = 2)"


def _brute_short_blocks(T, V, K=9):
    """Walk the taps of the clip's last tile: the 16-row blocks of its image (which starts at frame t_first - 4) that the stored
    pixels read, counted from the block of the tile's first pixel.  0 unless the tile holds 1 .. 128 pixels."""
    TV = T * V
    q0 = (TV - 1) // 256 * 256
    if TV - q0 > 128:
        return 0
    t_first = q0 // V
    rows = {q - t_first * V + tap * V for q in range(q0, TV) for tap in range(K)}      # row of pixel q's tap: prow + tap * V
    first = (q0 - t_first * V) >> 4
    assert min(rows) >> 4 == first
    return (max(rows) >> 4) - first + 1


def test_short_last_and_its_block_count_follow_the_taps():
    from stgcn_amd import _capi
    lib = _capi.lib()
    seen_short = seen_full = seen_over = 0
    for V in range(1, 33):
        for T in range(1, 201):
            got = lib.stgcn_stem_short_tile_blocks(128, T, V, 9)
            if not lib.stgcn_stem_supported(3, 128, T, V, 9, 3, 1) or lib.stgcn_stem_kernel_name(3, 128, T, V, 9, 3, 1) != b"stem_bf16_v6_kernel":
                continue
            want = _brute_short_blocks(T, V)
            if want > 20:                           # more than five blocks per wave: the shape keeps the full form
                seen_over += 1
                want = 0
            assert got == want, f"T={T} V={V}: the plan says {got} blocks, the taps read {want}"
            seen_short += want > 0
            seen_full += want == 0
    assert lib.stgcn_stem_short_tile_blocks(128, 180, 22, 9) == 20      # the headline: five blocks per wave, exactly
    assert seen_short > 100 and seen_full > 100
    print(f"{seen_short} shapes with a short last tile, {seen_full} without ({seen_over} of them read more than 20 blocks)")
