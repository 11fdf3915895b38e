"""The dynamic tail of the int8-prefilter scan (scan_q8.hip: the end of every launch's tile range is handed out by ticket, in
chunks of whole tile rounds, q8_tail_chunk) at the smallest shards that reach the hand-out's edges.

Every case forces scan="q8" and runs on 8 persistent workgroups (RARC_SCAN_Q8_WGS=8, the smallest grid the override allows),
so the edges do not depend on the CU count and a few hundred tiles are many rounds.  A round is 8 tiles; the loop consumes
`unit` rounds at once (2; 4 up to 384 dimensions).  Each case must return the oracle's ids and score bits with the tail on
(RARC_SCAN_Q8_TAIL = the dynamic share in per cent; 100 leaves one unit static; RARC_SCAN_Q8_TAIL_MIN=0 lifts the rule that
only launches of 32 MiB of rows per workgroup get a tail), again on a second search of the same index
(a ticket counter that was not re-zeroed would hand out nothing the second time and lose the tail's rows), and the same with
the switch off.  Which workgroup runs a chunk depends on timing, and with it the private segment a candidate lands in; the
answer must not.  The ticket counter of the first launch (in the workspace, where rarc_debug_q8_tail_counter_offset says) says whether the tail ran: every
workgroup draws exactly one ticket past the end, so it reads at least grid + 1 with the tail and 0 without.

Tiles: grid (one round: nothing to hand out), grid + 1, one unit per workgroup exactly (the static minimum: no tail) and
plus one tile (a tail of a single tile: the other workgroups' tickets are past the end), two units and two units plus
one tile, 117 and 263 (not multiples of a round: the last chunk's last round is part live, part redirected to tile 0;
263 tiles at 35 % and 100 % gives several levels of chunks).  The last tile is always partial (n = 32 tiles - 13 rows)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID, NQ, K = 8, 256, 10
_refs = {}


def _reference(oracle, storage, n, d, k=K, nq=NQ):
    """(X, Q, oracle ids, oracle scores), computed once per shape and left unchanged."""
    key = (storage, n, d, k)
    if key not in _refs:
        rng = np.random.default_rng(7000 * d + n)
        X = rng.standard_normal((n, d), dtype=np.float32)
        Q = rng.standard_normal((nq, d), dtype=np.float32)
        qn = oracle.normalize_L2(Q)
        if storage == "f8":
            b, s, _ = oracle.ingest_f8(X)
            I, D = oracle.flat_search_f8(b, s, qn, min(k, n))[:2]
        else:
            I, D = oracle.flat_search_f16(oracle.ingest_f16(X)[0], qn, min(k, n))[:2]
        _refs[key] = (X, Q, I, D)
    return _refs[key]


def _counters(idx):
    """Tickets drawn in each of the (up to four) scan_q8 launches of the last search: the library says where in the workspace its
    counters are, and the index must have a workspace after a search."""
    from rag_arc_amd.hip import binding as B

    offs = [int(B.load_library().rarc_debug_q8_tail_counter_offset(i)) for i in range(4)]
    assert min(offs) > 0 and idx._ws is not None and idx._ws.numel() > max(offs) + 4
    return np.array([int(idx._ws[o:o + 4].cpu().numpy().view(np.uint32)[0]) for o in offs], dtype=np.uint32)


def _tickets(idx):
    """... in the first launch."""
    return int(_counters(idx)[0])


def _search_checked(idx, Q, k, ref_I, ref_D, what):
    D, I = idx.search(Q, k)
    assert np.array_equal(I, ref_I), f"{what}: ids differ from the oracle"
    assert np.array_equal(D.view(np.uint32), ref_D.view(np.uint32)), f"{what}: score bits differ from the oracle"


def _run(monkeypatch, oracle, storage, shadow, d, tiles, pct, nq=NQ, grid=GRID, expect_tail=None, repeats=2):
    from rag_arc_amd.hip.engine import FlatIndexF16

    n = 32 * tiles - 13
    X, Q, ref_I, ref_D = _reference(oracle, storage, n, d)
    kk = min(K, n)
    monkeypatch.setenv("RARC_SCAN_Q8_WGS", str(grid))
    monkeypatch.setenv("RARC_SCAN_Q8_TAIL_MIN", "0")
    monkeypatch.setenv("RARC_SCAN_Q8_TAIL", str(pct))
    idx = FlatIndexF16(d, metric="cosine", scan="q8", storage=storage, shadow=shadow)
    idx.add(X)
    what = f"{storage}{' + shadow' if shadow else ''} d={d} tiles={tiles} share={pct}% nq={nq}"
    for r in range(repeats):   # back to back on one index: the counter is zeroed before every scan
        _search_checked(idx, Q[:nq], kk, ref_I[:nq], ref_D[:nq], f"{what}, search {r + 1}")
        if expect_tail is not None:
            t = _tickets(idx)
            assert (t >= grid + 1) if expect_tail else (t == 0), f"{what}, search {r + 1}: {t} tickets drawn"
    monkeypatch.setenv("RARC_SCAN_Q8_TAIL", "0")   # the purely static hand-out, same binary, same index
    _search_checked(idx, Q[:nq], kk, ref_I[:nq], ref_D[:nq], f"{what}, switch off")
    assert _tickets(idx) == 0, f"{what}: tickets drawn with the switch off"


def _edges(unit):
    return (GRID, GRID + 1, unit * GRID, unit * GRID + 1, 2 * unit * GRID, 2 * unit * GRID + 1, 117, 263)


@pytest.mark.parametrize("pct", (100, 35))
@pytest.mark.parametrize("d,unit,i", [(d, u, i) for d, u in ((768, 2), (128, 4)) for i in range(8)])
def test_tail_edges_match_oracle(monkeypatch, oracle, d, unit, i, pct):
    tiles = _edges(unit)[i]
    rounds = -(-tiles // GRID)
    # the launcher's rule: the share in whole rounds must reach one unit, and the static part keeps one unit
    expect = rounds * pct // 100 >= unit and tiles > unit * GRID
    _run(monkeypatch, oracle, "f16", False, d, tiles, pct, expect_tail=expect)


@pytest.mark.parametrize("nq", (1, 37))
def test_tail_with_few_queries(monkeypatch, oracle, nq):
    """Workgroups that own no query draw chunks like the others."""
    _run(monkeypatch, oracle, "f16", False, 768, 263, 100, nq=nq, expect_tail=True)


@pytest.mark.parametrize("storage,shadow,d", (("f8", False, 256), ("f16", True, 256), ("f8", False, 1024)))
def test_tail_other_row_formats(monkeypatch, oracle, storage, shadow, d):
    """fp8 and int8-shadow rows at their smallest padded dimension (four fetch groups), and the form without the ping-pong."""
    _run(monkeypatch, oracle, storage, shadow, d, 263, 100, expect_tail=True)


def test_tail_repeatable(monkeypatch, oracle):
    """Five searches: segment placement depends on who drew which chunk, ids and score bits do not."""
    _run(monkeypatch, oracle, "f16", False, 768, 263, 100, expect_tail=True, repeats=5)


@pytest.mark.parametrize("pct", (10, 100))
def test_tail_cascaded_scan(monkeypatch, oracle, pct):
    """2.1M x 128 fp16 rows on the full grid, k = 100: the smallest shard the cascade cuts, so the later launches start at
    t_begin != 0, resume the candidate segments, and draw from a counter of their own."""
    from rag_arc_amd.hip.engine import FlatIndexF16

    n, d, k = 2_100_000, 128, 100
    X, Q, ref_I, ref_D = _reference(oracle, "f16", n, d, k=k)
    monkeypatch.delenv("RARC_SCAN_Q8_WGS", raising=False)
    monkeypatch.setenv("RARC_SCAN_Q8_TAIL_MIN", "0")
    monkeypatch.setenv("RARC_SCAN_Q8_TAIL", str(pct))
    idx = FlatIndexF16(d, metric="cosine", scan="q8")
    idx.add(X)
    for r in range(2):
        _search_checked(idx, Q, k, ref_I, ref_D, f"cascaded n={n} d={d} share={pct}%, search {r + 1}")
    flags = _counters(idx)
    # (the first launch is 32 rounds: a tenth of it is less than one unit of four rounds, so at 10 % only the second has a tail)
    want = 2 if pct == 100 else 1
    assert np.count_nonzero(flags) >= want, f"ticket counters {flags.tolist()}: fewer than {want} launch(es) handed out a tail"
    monkeypatch.setenv("RARC_SCAN_Q8_TAIL", "0")
    _search_checked(idx, Q, k, ref_I, ref_D, f"cascaded n={n} d={d}, switch off")
    flags = _counters(idx)
    assert not flags.any(), f"ticket counters {flags.tolist()} with the switch off"
    # under the default size limit a shard this small keeps the static hand-out
    monkeypatch.setenv("RARC_SCAN_Q8_TAIL", str(pct))
    monkeypatch.delenv("RARC_SCAN_Q8_TAIL_MIN")
    _search_checked(idx, Q, k, ref_I, ref_D, f"cascaded n={n} d={d}, default size limit")
    flags = _counters(idx)
    assert not flags.any(), f"ticket counters {flags.tolist()}: a tail on launches under the size limit"
