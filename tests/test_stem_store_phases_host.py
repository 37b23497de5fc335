"""Host side of the fused stem's two store phases (csrc/kf6.h, narrow three-term form on shapes with short last tiles): the ORDER
in which a workgroup walks its run.  No GPU: the order is reached through ``stgcn_stem_walk_order``, which runs the kernel's own
``v6_order`` / ``v6_order_next``; the run it permutes comes from ``stgcn_stem_walk_run``.

Rule (written down here on its own, in numpy): workgroup b is of class ``(b >> 3) & 1``.  A class-1 workgroup whose run holds a
short tile (a clip's last tile, where the shape has short tiles) behind its first tile walks the first such tile first and then
the rest of the run in order; every other workgroup walks its run in order.  So: all workgroups together visit every tile exactly
once, a class-1 walk starts with its run's first short tile when it has one, every other walk is the ``stgcn_stem_walk_run``
range in order, and without ``short_last`` nothing is reordered at all."""
import ctypes

import numpy as np
import pytest

NS = range(1, 601)
GS = (1, 8, 16, 255, 256, 304)
TPCS = (1, 2, 3, 16, 43)


def _launch(lib, G, N, tpc, short, tiles, meta):
    """Runs and ordered walks of all G workgroups: (first, end, count) arrays and the walks concatenated in ``tiles``."""
    ntiles = N * tpc
    pos = 0
    base = ctypes.addressof(meta)
    isz = ctypes.sizeof(ctypes.c_int)
    tbase = ctypes.addressof(tiles)
    for b in range(G):
        o = base + 3 * b * isz
        assert lib.stgcn_stem_walk_run(b, G, N, tpc, short, o, o + isz) == 0
        assert lib.stgcn_stem_walk_order(b, G, N, tpc, short, tbase + pos * isz, ntiles - pos, o + 2 * isz) == 0
        pos += meta[3 * b + 2]
        assert pos <= ntiles, f"N={N} G={G} tpc={tpc} short={short}: the walks up to workgroup {b} hold {pos} tiles of {ntiles}"
    m = np.frombuffer(meta, dtype=np.int32, count=3 * G).reshape(G, 3)
    return m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy(), np.frombuffer(tiles, dtype=np.int32, count=pos).copy()


@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("tpc", TPCS)
@pytest.mark.parametrize("G", GS)
def test_ordered_walks_visit_every_tile_once_in_the_order_of_the_rule(G, tpc, short):
    from stgcn_amd import _capi
    lib = _capi.lib()
    tiles = (ctypes.c_int * (NS[-1] * tpc))()
    meta = (ctypes.c_int * (3 * G))()
    b = np.arange(G)
    reordered = class1_with_short = 0
    for N in NS:
        ntiles = N * tpc
        first, end, count, walk = _launch(lib, G, N, tpc, short, tiles, meta)
        what = f"N={N} G={G} tpc={tpc} short={short}"
        assert np.array_equal(count, end - first), f"{what}: a walk's length is not its run's"
        assert walk.size == ntiles and np.array_equal(np.sort(walk), np.arange(ntiles)), f"{what}: the walks do not visit every tile exactly once"
        # the rule: ts = the first tile of the run that ends a clip; walked first by a class-1 workgroup if it lies behind the run's first
        ts = first + (tpc - 1 - first % tpc)
        has_short = (short == 1) & (ts < end)
        moves = has_short & (((b >> 3) & 1) == 1) & (ts > first)
        seg = np.repeat(b, count)                  # the workgroup of each position of the concatenated walks (runs are contiguous,
        i = np.arange(ntiles)                      # so position i of the concatenation is tile i of an in-order walk)
        f, t, mv = first[seg], ts[seg], moves[seg]
        want = np.where(mv & (i == f), t, np.where(mv & (i > f) & (i <= t), i - 1, i))
        assert np.array_equal(walk, want), f"{what}: first difference from the rule at position {int(np.argmax(walk != want))}"
        # a class-1 walk starts with its run's first short tile when it has one (also where that tile is the run's first)
        c1 = has_short & (((b >> 3) & 1) == 1) & (count > 0)
        assert np.array_equal(walk[first[c1]], ts[c1]), f"{what}: a class-1 walk does not start with its first short tile"
        if not short:
            assert not moves.any() and np.array_equal(walk, i), f"{what}: reordered without short tiles"
        reordered += int(moves.sum())
        class1_with_short += int(c1.sum())
    print(f"G={G} tpc={tpc} short={short}: {reordered} reordered walks, {class1_with_short} class-1 walks with a short tile, N = 1 .. {NS[-1]}")
    if short and G >= 16 and tpc > 1:
        assert reordered > 0, "the sweep never reached a reordered walk"
    if G < 16 or not short:
        assert reordered == 0


def test_the_headline_walks():
    """256 clips of 16 tiles on 256 workgroups: one clip each; class 1 walks the clip's last tile first."""
    from stgcn_amd import _capi
    lib = _capi.lib()
    tiles, n = (ctypes.c_int * 16)(), ctypes.c_int()
    for b in (0, 7, 8, 15, 16, 24, 255):
        assert lib.stgcn_stem_walk_order(b, 256, 256, 16, 1, tiles, 16, ctypes.byref(n)) == 0 and n.value == 16
        got = list(tiles)
        want = list(range(16 * b, 16 * b + 16))
        if (b >> 3) & 1:
            want = [want[-1]] + want[:-1]
        assert got == want, (b, got)
    # count only: no buffer
    assert lib.stgcn_stem_walk_order(8, 256, 256, 16, 1, None, 0, ctypes.byref(n)) == 0 and n.value == 16
    assert lib.stgcn_stem_walk_order(300, 256, 256, 16, 1, None, 0, ctypes.byref(n)) == 0 and n.value == 0
