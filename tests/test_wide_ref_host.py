"""tests/wide_ref.py held to the rules of the chunk ladder it restates (csrc/wide.hip, wide_search_impl) and to hand-made
examples, on a sweep of n around every boundary of the ladder.  No GPU."""
import numpy as np
import pytest

from tests import wide_ref as WR

K_VALUES = (1, 10, 1024, 1025, 4000, 8192)
D_PADS = (128, 256, 1152, 4096)


def _sweep(k):
    """Row counts around every boundary: the first chunk, the 128- and 256-row blocks behind it, every rung of the ladder, the
    65536-row switch between the two fused kernels, the 131072-row score buffer."""
    growth = 4 if k <= 1024 else 2
    edges, rung, seen = {0, 128, 256, 16384}, 16384, 16384
    while seen < 3_000_000:
        rung = min(rung * growth, WR.WIDE_FUSED_CHUNK)
        seen += rung
        edges.add(seen)
    edges |= {16384 + 65536, 16384 + 65536 + 256, 16384 + WR.WIDE_CHUNK, 16384 + 2 * WR.WIDE_CHUNK}
    ns = set()
    for e in edges:
        for off in (-257, -256, -255, -129, -128, -127, -1, 0, 1, 77, 127, 128, 129, 255, 256, 257, 512 + 129):
            if e + off >= 0:
                ns.add(e + off)
    return sorted(ns)


@pytest.mark.parametrize("d_pad", D_PADS)
@pytest.mark.parametrize("k", K_VALUES)
def test_plan_obeys_the_ladders_rules(k, d_pad):
    for n in _sweep(k):
        pieces = WR.plan(n, k, d_pad)
        at = 0
        for i, p in enumerate(pieces):                        # the pieces tile [0, n) exactly once
            assert p.start == at and p.rows > 0, (n, pieces)
            at += p.rows
            assert (p.form == "first") == (i == 0)
            assert p.tail == (p.rows % 128 != 0)
            if p.form.startswith("fused"):                    # whole 256-row blocks of rows at least 256 wide
                assert p.rows % 256 == 0 and d_pad >= 256
                assert (p.form == "fused256") == (p.rows > 65536)
                assert p.rows <= WR.WIDE_FUSED_CHUNK
            else:
                assert p.rows <= WR.WIDE_CHUNK
            if i > 0:                                         # the first chunk took the ragged end
                assert p.rows % 256 == 0 and not p.tail
                assert (p.form == "stored") == (d_pad < 256)
        assert at == n
        if n:
            assert pieces[0].rows == (n if n <= 16384 else 16384 + (n - 16384) % 256)


def test_hand_made_plans():
    P = WR.Piece
    assert WR.plan(0, 10, 256) == []
    assert WR.plan(1, 1, 128) == [P(0, 1, "first", True)]
    assert WR.plan(16384, 8192, 256) == [P(0, 16384, "first", False)]
    assert WR.plan(16385, 1025, 128) == [P(0, 16385, "first", True)]
    assert WR.plan(16384 + 255, 1025, 256) == [P(0, 16639, "first", True)]
    assert WR.plan(16384 + 256, 1025, 128) == [P(0, 16384, "first", False), P(16384, 256, "stored", False)]
    assert WR.plan(16384 + 256, 1025, 256) == [P(0, 16384, "first", False), P(16384, 256, "fused128", False)]
    assert WR.plan(16384 + 257, 10, 256) == [P(0, 16385, "first", True), P(16385, 256, "fused128", False)]
    # k in the thousands doubles its chunks, smaller k quadruples them
    assert WR.plan(16384 + 65536 + 256 + 77, 1025, 128) == [P(0, 16461, "first", True), P(16461, 32768, "stored", False),
                                                             P(49229, 33024, "stored", False)]
    assert WR.plan(16384 + 65536 + 256 + 77, 1000, 128) == [P(0, 16461, "first", True), P(16461, 65536, "stored", False),
                                                             P(81997, 256, "stored", False)]
    # the score buffer holds 131072 rows: a stored chunk is never larger
    assert [p.rows for p in WR.plan(16384 + 65536 + 3 * 131072, 10, 128)] == [16384, 65536, 131072, 131072, 131072]
    # the 256 x 256 kernel takes over beyond 256 tiles
    assert WR.forms(16384 + 65536 + 65536 + 256, 10, 256) == ["first", "fused128", "fused256"]
    assert WR.smallest_n_with(("fused128", "fused256"), 10, 256) == 16384 + 65536 + 65536 + 256
    assert WR.smallest_n_with(("fused128", "fused256"), 1025, 256) == 16384 + 32768 + 65536 + 65536 + 256
    assert WR.plan(16384 + 65536 + 262144 + (1 << 20) + 512, 10, 1152)[-2:] == [P(344064, 1 << 20, "fused256", False),
                                                                                 P(344064 + (1 << 20), 512, "fused128", False)]


def test_float64_helpers():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((3, 64)).astype(np.float16)
    x = rng.standard_normal((100, 64)).astype(np.float16)
    ref = np.array([[sum(float(a) * float(b) for a, b in zip(qq, xx)) for xx in x] for qq in q])
    assert np.allclose(WR.dot64(q, x, block=7), ref, rtol=0, atol=1e-12)
    assert np.array_equal(WR.image16(x.view(np.uint16)), x)
    f = np.array([[1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.0]], np.float32)       # midpoints go to the even neighbour
    assert WR.image16(f).tolist() == [[1.0, 1.0 + 2.0 ** -9, 65504.0]]
    a = np.array([[5.0, 1.0, 3.0, 3.0, -2.0]])
    assert [float(WR.kth_largest(a, k)[0]) for k in (1, 2, 3, 5)] == [5.0, 3.0, 3.0, -2.0]
    ip = np.array([[1.0, 2.0]], np.float32)
    xn = np.array([4.0, 2.0], np.float32)
    kap = WR.l2_kappa(ip, xn)
    assert kap.tolist() == [[-1.0, 1.0]]
    # qn = 1: real distances 3 and max(0, -1) = 0
    assert WR.l2_dist_error(np.array([[3.5, 0.0]], np.float32), np.array([1.0], np.float32), kap).tolist() == [0.5]
