"""A search_async() batch that is still RUNNING when the index changes answers on the rows as they were at its launch.

The pipelined contexts (FlatIndexF16._pipeline_context, RARC_PIPELINE_Q8=1, a user twin()) enqueue their batches on side
streams; the mutators (add, add_rows_f16, load_rows, load_shard, remove_rows, reset) run on the caller's stream.  These
tests hold each context's side stream behind a device sleep, launch, change the index while the batch is provably still
queued (its sleep event has not completed), and then require ids and score bits equal to the oracle's on the launch-time
rows.  A fresh search afterwards must equal the oracle on the new rows.  Plus: a flagged batch in flight across a
remove_rows() refuses to answer, the sharded store's id map is the launch's, and a released handle never hands out the
answer of the search that took its pinned slot next."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 70_000              # >= FlatIndexF16.PIPELINE_MIN_ROWS: device-answer batches take the pipelined pair
HOLD_MS = 30.0          # how long each side stream is held before the batch under test may start
NQ = 5

# search context -> index configuration
_CTX = {
    "pair16": dict(storage="f16", metric="cosine", scan="auto"),    # the default pair, fp16 MFMA scan
    "pair_q8": dict(storage="f16", metric="cosine", scan="q8"),     # the pair on the int8 path (RARC_PIPELINE_Q8=1)
    "twin16": dict(storage="f16", metric="cosine", scan="q8"),      # a user twin(), int8 path over fp16 rows
    "twin32": dict(storage="f32", metric="ip", scan="q8"),          # a user twin() over fp32 rows (rho lives in _qmeta)
}
_MUTATORS = ("rm_first", "rm_last", "rm_run", "rm_third", "add_1", "add_tile", "add_realloc", "add_slab",
             "add_rows_f16", "load_rows", "load_shard", "reset")


@pytest.fixture(scope="module")
def hold_cycles():
    """torch.cuda._sleep cycles that keep a stream busy for about HOLD_MS on this part (measured once, not assumed)."""
    import torch

    s = torch.cuda.Stream()
    cycles, ms = 1 << 20, 0.0
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)                     # (first launch: code object load)
        for _ in range(8):                          # grow the probe until it is long enough to time
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 2.0:
                break
            cycles *= 4
    assert ms > 0.0
    return max(1, int(cycles * HOLD_MS / ms))


def _hold(streams, cycles):
    """Enqueue a sleep on every stream; the events complete when the sleeps do."""
    import torch

    events = []
    for s in streams:
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            ev = torch.cuda.Event()
            ev.record()
        events.append(ev)
    return events


@functools.lru_cache(maxsize=None)
def _data(d: int, metric: str, seed: int = 17):
    rng = np.random.default_rng(seed + d)
    X = rng.standard_normal((N, d)).astype(np.float32)
    if metric == "ip":
        X *= np.exp(rng.uniform(-1, 1, (N, 1))).astype(np.float32)
    Q = rng.standard_normal((NQ, d)).astype(np.float32)
    return X, Q


def _new_rows(n: int, d: int, metric: str, seed: int):
    """Rows to add: for "ip" scaled by 8e where the stored rows are scaled by at most e, so that max_norm (and for fp32
    storage the residual bound rho in the tile metadata) changes."""
    rng = np.random.default_rng(seed)
    Xn = rng.standard_normal((n, d)).astype(np.float32)
    if metric == "ip":
        Xn *= np.float32(8.0 * np.exp(1.0))
    return Xn


def _ingest(oracle, storage, X, metric):
    norm = metric == "cosine"
    if storage == "f16":
        rows, n2 = oracle.ingest_f16(X, normalize=norm)
        return rows, n2
    rows, n2 = oracle.ingest_f32(X, normalize=norm)
    return rows, n2


def _oracle_search(oracle, storage, X, Q, k, metric):
    qn = oracle.normalize_L2(Q) if metric == "cosine" else Q
    rows, _ = _ingest(oracle, storage, X, metric)
    if storage == "f16":
        return oracle.flat_search_f16(rows, qn, k)[:2]
    return oracle.flat_search_f32(rows, qn, k)[:2]


def _same(ids, scores, want, what):
    wi, ws = want
    assert np.array_equal(ids, wi), what
    assert np.array_equal(np.ascontiguousarray(scores).view(np.uint32), np.ascontiguousarray(ws).view(np.uint32)), what


def _prepare(mutator, idx, X, oracle, cfg, tmp_path, seed):
    """(apply() that changes idx, the fp32 source of the rows it holds afterwards).  Everything slow — building the rows,
    writing a shard file — happens here, before the streams are held."""
    import torch

    from rag_arc_amd.hip.engine import FlatIndexF16

    storage, metric, d = cfg["storage"], cfg["metric"], X.shape[1]
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    holes = {"rm_first": [0], "rm_last": [n - 1], "rm_run": list(range(n // 2 - 50, n // 2 + 50)),
             "rm_third": np.sort(rng.choice(n, n // 3, replace=False))}.get(mutator)
    if holes is not None:
        holes = np.asarray(holes, dtype=np.int64)
        return (lambda: idx.remove_rows(holes)), np.delete(X, holes, axis=0)
    if mutator == "reset":
        return idx.reset, X[:0]
    count = {"add_1": 1, "add_tile": 45, "add_realloc": 40, "add_rows_f16": 40, "load_rows": 37, "load_shard": 70}.get(mutator)
    if mutator == "add_slab":       # one row past what the arena has mapped: the next slab gets mapped
        count = int(idx._rows.shape[0]) - idx.ntotal + 64
    Xn = _new_rows(count, d, metric, seed + 1)
    kept = np.concatenate([X, Xn])
    if mutator in ("add_1", "add_tile", "add_realloc", "add_slab"):
        if mutator == "add_realloc":
            assert not idx.growable and idx.ntotal + count > idx._rows.shape[0]
        if mutator == "add_slab":
            assert idx.growable

            def apply():
                backed = idx.memory_bytes()["backed"]
                idx.add(Xn)
                assert idx.memory_bytes()["backed"] > backed
            return apply, kept
        return (lambda: idx.add(Xn)), kept
    rows, n2 = _ingest(oracle, storage, Xn, metric)
    max_norm = float(np.sqrt(n2.max()))
    if mutator == "add_rows_f16":
        dev = torch.from_numpy(rows.view(np.float16)).to(idx.device)
        return (lambda: idx.add_rows_f16(dev, max_norm)), kept
    if mutator == "load_rows":
        host = rows.view(np.float16) if storage == "f16" else rows
        return (lambda: idx.load_rows(host, max_norm)), kept
    assert mutator == "load_shard"
    src = FlatIndexF16(d, metric=metric, storage=storage)
    src.add(Xn)
    path = str(tmp_path / "extra.rarc")
    src.save_shard(path)
    del src
    return (lambda: idx.load_shard(path)), kept


def _run_case(oracle, hold_cycles, monkeypatch, tmp_path, ctx, mutator, k, d=384):
    import torch

    from rag_arc_amd.hip.engine import FlatIndexF16

    cfg = _CTX[ctx]
    monkeypatch.delenv("RARC_PIPELINE", raising=False)
    if ctx == "pair_q8":
        monkeypatch.setenv("RARC_PIPELINE_Q8", "1")
    X, Q = _data(d, cfg["metric"])
    idx = FlatIndexF16(d, metric=cfg["metric"], storage=cfg["storage"], scan=cfg["scan"],
                       growable=False if mutator == "add_realloc" else None)
    idx.add(X)
    Qd = torch.from_numpy(Q).to(idx.device)
    if ctx.startswith("pair"):
        idx.search_async(Qd, k).result()                        # warm-up: makes the pipelined pair
        assert idx._pair is not None
        searcher, streams = idx, [c._own_stream for c in idx._pair[:2]]
    else:
        searcher = idx.twin()
        searcher.search_async(Qd, k).result()
        streams = [searcher._own_stream]
    apply, kept = _prepare(mutator, idx, X, oracle, cfg, tmp_path, seed=100 * d + k)
    want = _oracle_search(oracle, cfg["storage"], X, Q, k, cfg["metric"])
    cut = 2
    if cfg["metric"] == "ip":
        # the "ip" score range reads the queries' norm back on the context's stream (FlatIndexF16._bins): a host wait behind
        # the hold, so the launch could not return before the hold ends.  The context is handed the range the engine
        # computes for these very queries beforehand instead (same kernel, same values).
        pre = {cut: idx._bins(Qd[:cut]), NQ - cut: idx._bins(Qd[cut:])}
        searcher._bins = lambda q: pre[q.shape[0]]

    events = _hold(streams, hold_cycles)
    handles = [searcher.search_async(Qd[:cut], k), searcher.search_async(Qd[cut:], k)]
    for h in handles:
        assert h.index._parent is not None and any(h.stream == s for s in streams), "the batch is not on a held side stream"
    assert not any(ev.query() for ev in events), "the window never opened: a held stream ran dry before the mutation"
    apply()

    what = (ctx, mutator, k, d)
    for h, sl in zip(handles, (slice(0, cut), slice(cut, NQ))):
        ids, scores = h.result()
        _same(ids.cpu().numpy(), scores.cpu().numpy(), (want[0][sl], want[1][sl]), what + ("in flight",))

    assert idx.ntotal == len(kept)
    if len(kept) == 0:
        D, I = idx.search(Q, k)
        assert (I == -1).all() and np.isneginf(D).all()
        return
    now = _oracle_search(oracle, cfg["storage"], kept, Q, k, cfg["metric"])
    D, I = idx.search(Q, k)
    _same(I, D, now, what + ("after",))
    ids, scores = idx.search_async(Qd, k).result()              # (a new pair, where the index is still large enough)
    _same(ids.cpu().numpy(), scores.cpu().numpy(), now, what + ("after, async",))


_MATRIX = [(c, m, k) for c in _CTX for m in _MUTATORS for k in (10, 100)
           if not (m == "add_rows_f16" and _CTX[c]["storage"] != "f16")]


@pytest.mark.parametrize("ctx,mutator,k", _MATRIX, ids=[f"{c}-{m}-k{k}" for c, m, k in _MATRIX])
def test_inflight_batch_answers_on_launch_rows(oracle, hold_cycles, monkeypatch, tmp_path, ctx, mutator, k):
    _run_case(oracle, hold_cycles, monkeypatch, tmp_path, ctx, mutator, k)


@pytest.mark.parametrize("ctx,mutator", [("pair16", "rm_third"), ("pair_q8", "add_tile")])
def test_inflight_batch_answers_on_launch_rows_d768(oracle, hold_cycles, monkeypatch, tmp_path, ctx, mutator):
    _run_case(oracle, hold_cycles, monkeypatch, tmp_path, ctx, mutator, 100, d=768)


def test_inflight_flagged_batch_refuses_after_remove(oracle, hold_cycles, monkeypatch):
    """k' == k leaves the fp16 scan's certificate no margin: every query is flagged.  A flagged batch whose rows changed
    under it cannot be repaired against the rows it scanned, so result() raises — it never returns an answer."""
    import torch

    from rag_arc_amd.hip import binding as B
    from rag_arc_amd.hip.engine import FlatIndexF16

    monkeypatch.delenv("RARC_PIPELINE", raising=False)
    X, Q = _data(384, "cosine")
    idx = FlatIndexF16(384, scan="mfma16")
    idx.add(X)
    idx.kprime_for = lambda k: k            # (the pipelined contexts are copies: they take it along)
    Qd = torch.from_numpy(Q).to(idx.device)
    h = idx.search_async(Qd, 50)
    h.result()
    assert h.repaired                       # (the batch under test needs one flagged query to refuse)
    events = _hold([c._own_stream for c in idx._pair[:2]], hold_cycles)
    h = idx.search_async(Qd, 50)
    assert h.index._parent is not None
    assert not any(ev.query() for ev in events), "the window never opened"
    idx.remove_rows(np.arange(1000, 1200))
    with pytest.raises(B.RarcError):
        h.result()
    rI, rD = _oracle_search(oracle, "f16", np.delete(X, np.arange(1000, 1200), axis=0), Q, 50, "cosine")
    D, I = idx.search(Q, 50)
    _same(I, D, (rI, rD), "after")


def test_sharded_inflight_remove_maps_with_launch_blocks(oracle, hold_cycles, monkeypatch):
    """_ShardedIndex (world 1, no process group) holding every other block of a two-rank layout: search_async, then
    remove_rows by GLOBAL id (own rows and the other rank's), then host(): the ids are the launch-time global ids."""
    import torch

    from rag_arc_amd.encapsulation.database.vector_db.hip_sharded import _ShardedIndex
    from rag_arc_amd.hip.engine import FlatIndexF16

    monkeypatch.delenv("RARC_PIPELINE", raising=False)
    X, Q = _data(384, "cosine")
    half, k = N // 2, 100
    sh = _ShardedIndex(FlatIndexF16(384))
    sh.add_block(X[:half], 0, N)                 # global ids [0, half) here, [half, N) on the other rank
    sh.add_block(X[half:], N, N)                 # [N, N + half) here
    assert sh.local.ntotal == N and sh.ntotal == 2 * N
    map_then = np.concatenate([np.arange(0, half), np.arange(N, N + half)])
    want_i, want_s = _oracle_search(oracle, "f16", X, Q, k, "cosine")
    Qd = torch.from_numpy(Q).to(sh.local.device)
    sh.search_async(Qd, k).host()                # warm-up: makes the pipelined pair
    events = _hold([c._own_stream for c in sh.local._pair[:2]], hold_cycles)
    p = sh.search_async(Qd, k)
    assert p.handle.index._parent is not None
    assert not any(ev.query() for ev in events), "the window never opened"
    holes = np.concatenate([[0], np.arange(half + 10, half + 110), np.arange(N + 500, N + 600), [N + half - 1]])
    sh.remove_rows(holes)
    scores, ids = p.host()
    _same(ids, scores, (map_then[want_i], want_s), "in flight")
    local_holes = np.concatenate([[0], np.arange(half + 500, half + 600), [N - 1]])
    kept = np.delete(X, local_holes, axis=0)
    ri, rs = _oracle_search(oracle, "f16", kept, Q, k, "cosine")
    map_now = np.concatenate([np.arange(0, half - 1), np.arange(N - 101, N - 101 + half - 101)])
    assert map_now.size == sh.local.ntotal
    scores, ids = sh.search_async(Qd, k).host()
    _same(ids, scores, (map_now[ri], rs), "after")


@pytest.mark.parametrize("nq", [7, 300], ids=["one_launch", "batches"])
def test_released_handle_never_returns_the_next_answer(oracle, nq):
    """host() releases the pinned slot, and the next to_host search of the same shape is handed that slot.  The first
    handle must then refuse (RarcError) — or, at worst, still give its own answer — never the second batch's."""
    from rag_arc_amd.hip import binding as B
    from rag_arc_amd.hip.engine import FlatIndexF16

    rng = np.random.default_rng(41)
    X = rng.standard_normal((5000, 384)).astype(np.float32)
    Q1, Q2 = (rng.standard_normal((nq, 384)).astype(np.float32) for _ in range(2))
    idx = FlatIndexF16(384)
    idx.add(X)
    h1 = idx.search_async(Q1, 10, to_host=True)
    a = h1.host()
    h2 = idx.search_async(Q2, 10, to_host=True)
    b = h2.host()
    _same(a[1], a[0], _oracle_search(oracle, "f16", X, Q1, 10, "cosine"), "first")
    _same(b[1], b[0], _oracle_search(oracle, "f16", X, Q2, 10, "cosine"), "second")
    assert not np.array_equal(a[1], b[1])
    for call in ("result", "host_view", "host"):
        try:
            got = getattr(h1, call)()
        except B.RarcError:
            continue
        if call == "result":
            got = (np.asarray(got[1].cpu()), np.asarray(got[0].cpu()))
        assert np.array_equal(got[1], a[1]) and np.array_equal(got[0].view(np.uint32), a[0].view(np.uint32)), call
