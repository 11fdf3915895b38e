"""The int8 scale of a prepared query (csrc/rarc_common.h: rarc_query_scale8, called by rarc_prep_queries' kernel) on the host,
through rarc_debug_query_scale8.  The kernel used to take

    sq = (mx > 0 && mx < inf) ? 127 / mx : 1;    while ((double)mx * (double)sq > 127.4) sq *= 0.9999f;

which never leaves the loop once 127 / mx overflows (0 < mx < 127 / FLT_MAX = 3.73e-37: sq = inf stays inf) and for mx = inf
(inf * sq stays inf down to the subnormal where sq * 0.9999f rounds back to sq).  The helper has no loop; that this sweep
returns is its proof of termination, and for every mx the old lines did handle it must return their sq bit for bit."""
import ctypes

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B

F32 = np.float32
FLT_MIN, FLT_MAX = F32(np.finfo(np.float32).tiny), F32(np.finfo(np.float32).max)
EDGE = F32(127.0 / float(FLT_MAX))                # the fp32 next to 127 / FLT_MAX


def _scale8(mx):
    sq, qi = ctypes.c_float(), ctypes.c_float()
    assert B.load_library().rarc_debug_query_scale8(ctypes.c_float(float(mx)), ctypes.byref(sq), ctypes.byref(qi)) == 0
    return F32(sq.value), F32(qi.value)


def _old_lines(mx):
    """The two lines above in numpy float32 (the comparison in float64, as written).  None: the loop does not end — 64 rounds
    of it change nothing that could end it."""
    mx = F32(mx)
    with np.errstate(all="ignore"):
        sq = F32(127.0) / mx if (mx > 0 and mx < np.inf) else F32(1.0)
        for _ in range(64):
            if not float(mx) * float(sq) > 127.4:
                return F32(sq)
            sq = F32(sq * F32(0.9999))
    return None


def _neighbours(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def _sweep():
    vals = [F32(0.0), F32(-0.0), FLT_MIN, FLT_MAX, F32(np.inf), F32(np.nan)]
    for e in range(-149, 128):
        vals += _neighbours(np.ldexp(F32(1.0), e))
    vals += _neighbours(EDGE) + _neighbours(np.nextafter(EDGE, F32(0.0))) + _neighbours(np.nextafter(EDGE, F32(1.0)))
    rng = np.random.default_rng(2024)
    vals += list(rng.integers(1, 0x7f800000, 4000, dtype=np.uint32).view(np.float32))   # uniform over positive finite patterns
    return [F32(v) for v in vals]


def test_every_scale_is_finite_positive_and_within_range():
    for mx in _sweep():
        sq, qi = _scale8(mx)
        assert np.isfinite(sq) and sq > 0 and np.isfinite(qi) and qi > 0, (mx, sq, qi)
        if np.isfinite(mx):
            assert float(mx) * float(sq) <= 127.4, (mx, sq)
        with np.errstate(all="ignore"):
            assert qi.view(np.uint32) == (F32(1.0) / sq).view(np.uint32), (mx, sq, qi)


def test_the_old_lines_answer_is_kept_wherever_they_had_one():
    kept = spun = 0
    for mx in _sweep():
        old = _old_lines(mx)
        with np.errstate(all="ignore"):
            in_domain = mx == 0 or np.isnan(mx) or (np.isfinite(mx) and mx > 0 and np.isfinite(F32(127.0) / mx))
        if in_domain:
            assert old is not None and _scale8(mx)[0].view(np.uint32) == old.view(np.uint32), (mx, old, _scale8(mx))
            kept += 1
        elif mx > 0:                                # 127 / mx overflowed, or mx is infinite: the old loop spins
            assert old is None and _scale8(mx)[0] == F32(1.0), (mx, old)
            spun += 1
    assert kept > 4000 and spun > 60


@pytest.mark.parametrize("mx", [3.8e-37, 3.7e-37, 2e-38, 1e-40, 1.4e-45])
def test_the_values_the_defect_was_found_with(mx):
    sq, qi = _scale8(F32(mx))
    if mx > float(EDGE) * 1.01:
        assert _old_lines(mx) is not None and sq.view(np.uint32) == _old_lines(mx).view(np.uint32)
    else:
        assert _old_lines(mx) is None and sq == F32(1.0) and qi == F32(1.0)


def test_null_pointers_are_refused():
    lib = B.load_library()
    assert lib.rarc_debug_query_scale8(ctypes.c_float(1.0), None, None) == -1 and b"null pointer" in lib.rarc_last_error()
