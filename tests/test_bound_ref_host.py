"""tests/bound_ref.py against the layouts it restates (csrc/rarc_common.h) and against hand-made examples: the GPU tests of
the prefilter's bound read every figure through it."""
import os
import re

import numpy as np
import pytest

from tests import bound_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _common_h():
    with open(os.path.join(ROOT, "rag-arc_amd", "csrc", "rarc_common.h")) as f:
        return f.read()


def test_constants_match_the_header():
    src = _common_h()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))   # noqa: E731
    assert const("RARC_QMETA_HDR") == BR.QMETA_HDR
    assert const("RARC_QMETA_STRIDE") == BR.QMETA_STRIDE["f16"] == BR.QMETA_STRIDE["f32"]
    assert const("RARC_QMETA_F8_STRIDE") == BR.QMETA_STRIDE["f8"] == 2 + BR.TILE_ROWS
    assert "(size_t)RARC_MAX_QUERIES * (size_t)d_pad * 7 + 5 * 1024" in src
    for name, expr in [("q16", "n * 4"), ("q8", "n * 6"), ("eps16", "n * 7"), ("eps8", "n * 7 + 1024"),
                       ("qinv", "n * 7 + 2048"), ("hq", "n * 7 + 3072"), ("floor", "n * 7 + 4096")]:
        assert re.search(rf"q\.{name} = \([a-z0-9_]+\*\)\(b \+ {re.escape(expr)}\);", src), name


@pytest.mark.parametrize("d_pad", [128, 256, 1024])
def test_query_block_parts_tile_the_block(d_pad):
    off = BR.qblock_offsets(d_pad)
    assert off["q32"] == 0 and off["floor"] + 1024 == BR.qblock_bytes(d_pad)
    assert all(v % 256 == 0 for v in off.values())
    qb = np.zeros(BR.qblock_bytes(d_pad), np.uint8)
    qb[off["q8"]: off["q8"] + 256 * d_pad] = 7
    qb[off["eps8"]: off["eps8"] + 1024].view(np.float32)[:] = np.arange(256, dtype=np.float32)
    qb[off["hq"]: off["hq"] + 1024].view(np.float32)[:] = 2.0
    assert BR.qblock_part(qb, d_pad, "q8", 3).shape == (3, d_pad) and (BR.qblock_part(qb, d_pad, "q8", 256) == 7).all()
    assert not BR.qblock_part(qb, d_pad, "q16", 256).any() and not BR.qblock_part(qb, d_pad, "q32", 256).any()
    assert np.array_equal(BR.qblock_part(qb, d_pad, "eps8", 5), np.arange(5, dtype=np.float32))
    assert (BR.qblock_part(qb, d_pad, "hq", 256) == 2.0).all() and not BR.qblock_part(qb, d_pad, "qinv", 256).any()


@pytest.mark.parametrize("storage", ["f16", "f8", "f32"])
def test_tile_metadata_round_trip(storage):
    n = 70                                                # three tiles, the last one ragged
    stride = BR.QMETA_STRIDE[storage]
    assert BR.n_tiles(n) == 3 and BR.qmeta_floats(n, storage) == 4 + 3 * stride
    s = np.array([0.5, 127.0, 32768.0], np.float16)
    rt = np.array([2.0 ** -24, 0.25, 1000.0], np.float16)
    qm = np.zeros(BR.qmeta_floats(n, storage), np.float32)
    words = (rt.view(np.uint16).astype(np.uint32) << 16) | s.view(np.uint16).astype(np.uint32)
    qm[4::stride] = words.view(np.float32)
    qm[5::stride] = 1.0 / s.astype(np.float32)
    if storage == "f8":
        for t in range(3):
            qm[4 + stride * t + 2: 4 + stride * (t + 1)] = 100 * t + np.arange(32)
    gs, grt, ginv = BR.tile_meta(qm, n, storage)
    assert np.array_equal(gs, s.astype(np.float64)) and np.array_equal(grt, rt.astype(np.float64))
    assert np.array_equal(ginv, (1.0 / s.astype(np.float32)).astype(np.float64))
    if storage == "f8":
        mul = BR.row_multipliers_f8(qm, n)
        assert mul.shape == (n,) and mul[0] == 0 and mul[33] == 101 and mul[69] == 205


def test_check_bound_accepts_equality_and_refuses_one_ulp_more():
    eps8, hq = np.array([1.0, 2.0]), np.array([0.5, 0.25])
    R, rt = 1.0, np.array([1.0, 0.5])                     # tile 1 earns hq * 0.5
    n = 40
    lim = BR.tile_bounds(eps8, hq, R, rt, n)
    assert lim.shape == (2, n) and (lim[:, :32] == eps8[:, None]).all()
    assert (lim[0, 32:] == 0.75).all() and (lim[1, 32:] == 1.875).all()
    assert BR.check_bound(lim.copy(), eps8, hq, R, rt) == 1.0
    bad = lim.copy()
    bad[1, 35] = np.nextafter(bad[1, 35], np.inf)         # inside eps8, outside the tile's share of it
    with pytest.raises(AssertionError, match="per-tile bound violated"):
        BR.check_bound(bad, eps8, hq, R, rt)
    bad = lim.copy()
    bad[0, 3] = np.nextafter(1.0, np.inf)
    with pytest.raises(AssertionError, match="bound violated"):
        BR.check_bound(bad, eps8, hq, R, rt)
    with pytest.raises(AssertionError, match="exceeds R"):
        BR.check_bound(lim * 0, eps8, hq, R, np.array([1.0, 1.01]))
    with pytest.raises(AssertionError, match="not attained"):
        BR.check_bound(lim * 0, eps8, hq, R, np.array([0.5, 0.5]))
    assert BR.check_bound(lim * 0, eps8, hq, R, np.array([0.5, 0.5]), attained=False) == 0.0
    with pytest.raises(AssertionError, match="non-finite"):
        BR.check_bound(lim * np.nan, eps8, hq, R, rt)


def test_int8_image_rounds_the_exact_product_to_even():
    rows = np.zeros((33, 8), np.float16)
    rows[0, :6] = [0.5, 1.5, 2.5, -0.5, -1.5, 127.0]
    rows[32, :3] = [1.0, 0.2499, 0.25]
    img = BR.int8_image_f16(rows, np.array([1.0, 2.0]))
    assert img.dtype == np.int8 and img[0, :6].tolist() == [0, 2, 2, 0, -2, 127]
    assert img[32, :3].tolist() == [2, 0, 0] and not img[1:32].any()
    # the restatement agrees with an fp16 fma done the long way (float64 sum, one rounding to fp16) on random data
    rng = np.random.default_rng(0)
    x = rng.standard_normal((64, 16)).astype(np.float16)
    s = np.array([np.float16(126.0 / np.abs(x[:32]).max()), np.float16(100.0 / np.abs(x[32:]).max())])
    y = (x.astype(np.float64) * np.repeat(s.astype(np.float64), 32)[:, None] + 1536.0).astype(np.float16)
    assert np.array_equal(BR.int8_image_f16(x, s), (y.view(np.uint16) & 0xff).astype(np.uint8).view(np.int8))
