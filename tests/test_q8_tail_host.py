"""The dynamic tail of the int8-prefilter scan on the host (csrc/scan_q8.hip): the launcher's plan for a launch (q8_tail_plan:
where the static share ends, how large the first chunks are) and the map ticket -> tiles that the kernel applies to every
ticket it draws (q8_tail_chunk), through rarc_debug_q8_tail_plan / rarc_debug_q8_tail_chunks.  No GPU.

Swept together over grid, row width (unit 2 and 4), row format, dynamic share, size limit, t_begin and n_tiles, and the map
alone over r0 (below Q8_TAIL_RMIN included) and t_dyn that no plan would produce.  For every case:
  * the static share [t_begin, t_dyn) is whole units of rounds, at least one, and every workgroup's first tile exists;
  * the chunks of the tickets 0, 1, 2, ... cover every tile of [t_dyn, n_tiles) exactly once and nothing else;
  * a chunk stays inside [t_dyn, n_tiles), starts at its workgroup slot of a round and ends at a round's end or at n_tiles;
  * a chunk is whole units of rounds unless n_tiles clips it;
  * first tiles grow with the ticket, so the first ticket past the end (t0 >= n_tiles, returned as n_tiles) is followed only
    by tickets past the end — a workgroup may stop at the first one it draws."""
import ctypes

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B

U32 = ctypes.c_uint32
RMIN = 8   # Q8_TAIL_RMIN


def _plan(t_begin, n_tiles, grid, d_pad, fmt, pct, min_mib):
    t_dyn, r0, unit = U32(), U32(), U32()
    B.check(B.load_library().rarc_debug_q8_tail_plan(t_begin, n_tiles, grid, d_pad, fmt, pct, min_mib, ctypes.byref(t_dyn),
                                                     ctypes.byref(r0), ctypes.byref(unit)))
    return t_dyn.value, r0.value, unit.value


def _chunks(k_first, n, stride, unit, t_dyn, r0, n_tiles):
    t0, t_end = np.empty(n, np.uint32), np.empty(n, np.uint32)
    B.check(B.load_library().rarc_debug_q8_tail_chunks(k_first, n, stride, unit, t_dyn, r0, n_tiles, t0.ctypes.data, t_end.ctypes.data))
    return t0.astype(np.int64), t_end.astype(np.int64)


def _check_map(stride, unit, t_dyn, r0, n_tiles, what):
    """Every property of the docstring for one tail."""
    tail = n_tiles - t_dyn
    rounds = -(-tail // stride)
    # enough tickets: the levels r0, r0/2, ... then RMIN each, `stride` tickets per level; then a stretch past the end
    levels = 2 + int(np.log2(max(r0, RMIN))) + rounds // RMIN
    n = (levels + 2) * stride
    t0, t_end = _chunks(0, n, stride, unit, t_dyn, r0, n_tiles)
    live = t0 < n_tiles
    n_live = int(live.sum())
    assert n_live >= 1, f"{what}: no chunk at all"
    assert live[:n_live].all() and not live[n_live:].any(), f"{what}: a live ticket after one past the end"
    assert (t0[n_live:] == n_tiles).all(), f"{what}: a ticket past the end does not return n_tiles"
    assert n - n_live >= stride, f"{what}: the sweep did not reach past the end"
    a, b = t0[:n_live], t_end[:n_live]
    assert (np.diff(a) > 0).all(), f"{what}: first tiles do not grow with the ticket"
    assert (a >= t_dyn).all() and (b <= n_tiles).all() and (a < b).all(), f"{what}: a chunk leaves [t_dyn, n_tiles)"
    k = np.arange(n_live)
    assert ((a - t_dyn) % stride == k % stride).all(), f"{what}: a chunk does not start at its slot"
    clipped = b == n_tiles
    assert (((b - t_dyn) % stride == 0) | clipped).all(), f"{what}: a chunk ends inside a round"
    r_first, r_end = (a - t_dyn) // stride, -(-(b - t_dyn) // stride)
    assert (((r_end - r_first) % unit == 0) | clipped).all(), f"{what}: a chunk is not whole units of rounds"
    assert ((r_first % unit) == 0).all(), f"{what}: a chunk does not start on a unit of rounds"
    # coverage, by slot: the chunks of slot s are consecutive runs of rounds [r_first, r_end) — each round once, none missing
    seen = np.zeros(tail, np.uint8)
    for x, y in zip(a, b):
        seen[x - t_dyn:y - t_dyn:stride] += 1
    assert (seen == 1).all(), f"{what}: {int((seen == 0).sum())} tail tiles not covered, {int((seen > 1).sum())} more than once"


GRIDS = (1, 3, 8, 37, 256)
SHAPES = ((768, 0), (128, 0), (384, 0), (512, 0), (1024, 1), (256, 1), (768, 2))   # (d_pad, row format): units 2 and 4


@pytest.mark.parametrize("grid", GRIDS)
def test_plan_and_map_together(grid):
    rng = np.random.default_rng(100 + grid)
    cases = 0
    for d_pad, fmt in SHAPES:
        for pct in ((1, 10, 16, 35, 50, 99, 100) if grid < 256 else (16, 35, 100)):   # (the full grid: the shares that differ in kind)
            for t_begin_rounds in (0, 2, 16, 6144 // 8):
                sizes = [1, grid - 1, grid, grid + 1, 2 * grid, 4 * grid, 4 * grid + 1, 8 * grid + grid // 2, 117, 263, 1000 * grid - 1]
                sizes += list(rng.integers(1, 3000 * grid, 6))
                for size in sizes:
                    if size < 1:
                        continue
                    pair = 2 * grid                       # cuts are multiples of 2 x grid
                    t_begin = t_begin_rounds * pair
                    n_tiles = t_begin + int(size)
                    t_dyn, r0, unit = _plan(t_begin, n_tiles, grid, d_pad, fmt, pct, 0)
                    what = f"grid {grid} d_pad {d_pad} fmt {fmt} share {pct}% tiles [{t_begin}, {n_tiles})"
                    assert unit == (4 if d_pad <= 384 else 2), what
                    rounds = -(-size // grid)
                    if t_dyn == n_tiles:                  # no tail: the share is under one unit, or nothing is left behind one unit
                        assert rounds * pct // 100 < unit or size <= unit * grid, f"{what}: no tail"
                        continue
                    assert rounds * pct // 100 >= unit, f"{what}: a tail from a share under one unit"
                    stat = t_dyn - t_begin
                    assert stat % (unit * grid) == 0 and stat >= unit * grid and t_dyn < n_tiles, f"{what}: static share {stat} tiles"
                    assert r0 % unit == 0 and r0 <= rounds, f"{what}: r0 {r0}"
                    # the share asked for is what is handed out, to one unit of rounds (and the static minimum)
                    tail_rounds = -(-(n_tiles - t_dyn) // grid)
                    share = rounds * pct // 100
                    assert stat == unit * grid or share <= tail_rounds < share + unit, f"{what}: tail of {tail_rounds} rounds"
                    _check_map(grid, unit, t_dyn, r0, n_tiles, what)
                    cases += 1
    assert cases > 500, cases


def test_size_limit_of_the_plan():
    """Rows per workgroup under the limit: no tail.  768-dim fp16 tiles are 48 KiB: 32 MiB = 683 rounds (rounded up)."""
    for grid in (8, 256):
        for rounds, want in ((682, False), (683, True), (4096, True)):
            t_dyn, _, _ = _plan(0, rounds * grid, grid, 768, 0, 16, 32)
            assert (t_dyn < rounds * grid) == want, (grid, rounds, t_dyn)
        # fp8 / shadow rows are one byte per value: twice the rounds
        assert _plan(0, 1365 * grid, grid, 768, 2, 16, 32)[0] == 1365 * grid
        assert _plan(0, 1366 * grid, grid, 768, 2, 16, 32)[0] < 1366 * grid
        assert _plan(0, 682 * grid, grid, 768, 0, 16, 0)[0] < 682 * grid     # limit lifted
        assert _plan(0, 4096 * grid, grid, 768, 0, 0, 0)[0] == 4096 * grid   # share 0: the switch is off


@pytest.mark.parametrize("unit", (2, 4))
def test_map_alone(unit):
    """The map for tails no plan would ask for: r0 = 0 and below Q8_TAIL_RMIN, r0 larger than the tail, r0 no multiple of the
    unit's halves, a tail of one tile, a tail that ends in the middle of a round."""
    for stride in (1, 2, 5, 8, 64, 256):
        for r0 in (0, unit, RMIN - unit, RMIN, RMIN + unit, 20, 64, 100, 1024):
            for t_dyn in (0, unit * stride, 6144):
                for extra in (1, 2, stride - 1, stride, stride + 1, RMIN * stride, RMIN * stride + 1, 37 * stride + stride // 2,
                              300 * stride + 1):
                    if extra < 1:
                        continue
                    _check_map(stride, unit, t_dyn, r0, t_dyn + extra, f"stride {stride} unit {unit} r0 {r0} tiles [{t_dyn}, {t_dyn + extra})")


def test_headline_and_the_largest_shard():
    """The four launches of the 100M-row headline on 256 workgroups, and one launch over 2^27 - 1 tiles (the most a uint32 row count
    gives): no 32-bit overflow in the map or the plan."""
    grid = 256
    cuts = (0, 5632, 48640, 390144, 3125000)
    for i in range(4):
        t_dyn, r0, unit = _plan(cuts[i], cuts[i + 1], grid, 768, 0, 16, 32)
        if i < 2:
            assert t_dyn == cuts[i + 1], f"launch {i + 1} is under the size limit"
        else:
            assert cuts[i] < t_dyn < cuts[i + 1]
            _check_map(grid, unit, t_dyn, r0, cuts[i + 1], f"headline launch {i + 1}")
    n_tiles = 2 ** 27 - 1
    for d_pad in (768, 128):
        t_dyn, r0, unit = _plan(0, n_tiles, grid, d_pad, 0, 16, 32)
        assert 0 < t_dyn < n_tiles
        _check_map(grid, unit, t_dyn, r0, n_tiles, f"2^27 - 1 tiles, d_pad {d_pad}")
    # and a tail that reaches the end of the 32-bit tile range itself
    _check_map(grid, 2, 2 ** 32 - 1 - 40 * grid - 3, 16, 2 ** 32 - 1, "tiles up to 2^32 - 1")


def test_counter_offsets():
    lib = B.load_library()
    offs = [lib.rarc_debug_q8_tail_counter_offset(i) for i in range(4)]
    assert offs[0] > B.WS_ANYFLAG_OFFSET and offs[0] % 4 == 0 and [o - offs[0] for o in offs] == [0, 4, 8, 12], offs
    assert offs[3] + 4 <= B.WS_ANYFLAG_OFFSET - 4 + 64 * 4, "past the 64 flag words the seed pass zeroes"
    assert lib.rarc_debug_q8_tail_counter_offset(-1) == -1 and lib.rarc_debug_q8_tail_counter_offset(4) == -1
