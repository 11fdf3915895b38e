"""The small end of the fp32 range — the mirror of tests/test_gpu_range_edge.py: queries and rows whose elements are near
FLT_MIN or subnormal, whose squares are subnormal or vanish in the fp32 sum of squares, whose largest element is below
127 / FLT_MAX (where the query block's int8 scale 127 / max|q| overflows), and all-zero queries.

The contract, for every case here: the answer is the oracle's, ids and score bits — or RarcUnsupported is raised before
anything reaches a kernel, its message says what does answer, and the index is as usable as before.  Never a bare RarcError,
a non-finite score or another id set.  The reference answers zero and tiny queries (every score is +-0 or next to it, ties by
id), so the outcome expected of every rung is "exact"; DESIGN.md 4.1 names no refusal at this end.

The ladder of scales is applied to ordinary Gaussian data in float64 and then cast; what the cast produced is printed per rung.
The oracle is the definition: (score desc, id asc) on the order-preserving bit pattern of the score, so +0 ranks above -0."""
import numpy as np
import pytest

from tests import l2_ref, subset_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
EDGE = 127.0 / FLT_MAX                 # below it 127 / max|q| is no finite fp32
N, NQ, K = 2000, 4, 10

# (name, kind, value): "scale" multiplies the batch; "max" scales every query so that its largest magnitude is the value
LADDER = [
    ("1e-10", "scale", 1e-10),
    ("2^-63", "scale", 2.0 ** -63),            # squares near FLT_MIN
    ("2^-70", "scale", 2.0 ** -70),            # squares are fp32 subnormals: a device that flushed them would part from the oracle
    ("2^-74", "scale", 2.0 ** -74),            # squares round to the smallest subnormals ...
    ("2^-76", "scale", 2.0 ** -76),            # ... and to zero: the sum of squares of a non-zero vector is 0
    ("above 127/FLT_MAX", "max", EDGE * 1.01),
    ("below 127/FLT_MAX", "max", EDGE * 0.99),
    ("FLT_MIN", "max", FLT_MIN),
    ("1e-42", "scale", 1e-42),                 # the elements themselves are subnormal
    ("0", "scale", 0.0),
]
NARROW = [("f16", "q8"), ("f16", "mfma16"), ("f16", "auto"), ("f8", "auto"), ("f32", "auto")]
COMBOS = [(s, c, 256) for s, c in NARROW] + [("f16", "auto", 1536), ("f32", "auto", 1536)]


def _rung(A, kind, value):
    a = np.asarray(A, np.float64)
    if kind == "max":
        a = a * (value / np.abs(a).max(axis=1, keepdims=True))
    else:
        a = a * value
    return a.astype(F32)


def _describe(name, A):
    a = np.abs(A.astype(np.float64))
    sq = (A * A).astype(F32)                    # the fp32 squares, as the first step of every chain forms them
    with np.errstate(all="ignore"):
        return (f"{name}: max|x| {a.max():.3e}, subnormal elements {int(((a > 0) & (a < FLT_MIN)).sum())}, zeros {int((a == 0).sum())}, "
                f"subnormal squares {int(((sq > 0) & (sq < F32(FLT_MIN))).sum())}, vanished squares {int(((sq == 0) & (a > 0)).sum())}")


def _metrics(storage, scan):
    return ("ip", "cosine", "l2") if (storage in ("f16", "f32") and scan == "auto") else ("ip", "cosine")


def _index(metric, storage, d, scan="auto"):
    from rag_arc_amd.hip.engine import FlatIndexF16

    return FlatIndexF16(d, metric=metric, storage=storage, scan=scan)


class _Ref:
    """The oracle's answer for one (metric, storage, X): the rows are ingested once."""

    def __init__(self, oracle, metric, storage, X):
        self.o, self.metric, self.storage = oracle, metric, storage
        normalize = metric == "cosine"
        if storage == "f8":
            self.rows, self.scales, _ = oracle.ingest_f8(X, normalize=normalize)
        elif storage == "f32":
            self.rows = oracle.ingest_f32(X, normalize=normalize)[0]
        else:
            self.rows = oracle.ingest_f16(X, normalize=normalize)[0]

    def search(self, Q, k):
        """-> (I, D)"""
        o = self.o
        Q = np.ascontiguousarray(Q, F32)
        if self.metric == "l2":
            D, I = l2_ref.search(o, None, Q, k, self.storage, rows=self.rows)
            return I, D
        if self.metric == "cosine":
            Q = o.normalize_L2(Q)
        if self.storage == "f8":
            return o.flat_search_f8(self.rows, self.scales, Q, k)[:2]
        if self.storage == "f32":
            return o.flat_search_f32(self.rows, Q, k)[:2]
        return o.flat_search_f16(self.rows, Q, k)[:2]


def _same(D, I, ref, what=""):
    assert np.isfinite(D).all(), f"{what}: non-finite scores"
    assert np.array_equal(I, ref[0]), f"{what}: ids differ from the oracle's"
    assert np.array_equal(np.ascontiguousarray(D, F32).view(np.uint32), ref[1].view(np.uint32)), f"{what}: score bits differ from the oracle's"


def _outcome(search, ref, what):
    """The contract: the oracle's answer, or RarcUnsupported with a way out in its message.  Anything else fails."""
    from rag_arc_amd.hip import binding as B

    try:
        D, I = search()
    except B.RarcUnsupported as exc:
        msg = str(exc)
        assert "scale" in msg and ("cosine" in msg or "f16" in msg or "f32" in msg), f"{what}: the refusal names no way out: {msg}"
        return "refused"
    _same(D, I, ref, what)
    return "exact"


def _data(d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, d)).astype(F32), rng.standard_normal((NQ, d)).astype(F32), rng


@pytest.mark.parametrize("storage, scan, d", COMBOS)
def test_tiny_queries_on_ordinary_rows(oracle, storage, scan, d):
    """Every rung of the ladder under every metric the storage has; after each rung the unscaled queries are answered as
    before."""
    X, Q0, _ = _data(d, 21)
    for metric in _metrics(storage, scan):
        ref = _Ref(oracle, metric, storage, X)
        plain = ref.search(Q0, K)
        idx = _index(metric, storage, d, scan)
        idx.add(X)
        outcomes = {}
        for name, kind, value in LADDER:
            Q = _rung(Q0, kind, value)
            if metric == "ip" and d == 256 and (storage, scan) == NARROW[0]:
                print(_describe(name, Q))
            what = f"{metric} {storage} {scan} d={d} rung {name}"
            outcomes[name] = _outcome(lambda: idx.search(Q, K), ref.search(Q, K), what)
            D, I = idx.search(Q0, K)
            _same(D, I, plain, what + ", then the unscaled queries")
        print(f"tiny queries {metric} {storage} {scan} d={d}: {outcomes}")
        assert set(outcomes.values()) == {"exact"}, outcomes


@pytest.mark.parametrize("storage, scan, d", COMBOS)
def test_a_mixed_batch(oracle, storage, scan, d):
    """One ordinary query, one whose squares vanish, one all-zero, one below 127 / FLT_MAX, in the same call: the score window
    comes from the largest."""
    X, Q0, _ = _data(d, 22)
    Q = np.stack([Q0[0], _rung(Q0[1:2], "scale", 2.0 ** -76)[0], np.zeros(d, F32), _rung(Q0[3:4], "max", EDGE * 0.99)[0]])
    for metric in _metrics(storage, scan):
        idx = _index(metric, storage, d, scan)
        idx.add(X)
        what = f"mixed batch {metric} {storage} {scan} d={d}"
        assert _outcome(lambda: idx.search(Q, K), _Ref(oracle, metric, storage, X).search(Q, K), what) == "exact"


@pytest.mark.parametrize("storage, scan, d", COMBOS)
def test_a_batch_of_zero_queries(oracle, storage, scan, d):
    """Metric "ip" used to answer this with RARC_E_INVALID "empty histogram range".  The reference answers it: every score is
    +0, so the ids are 0 .. k-1 (metric "l2": the rows of smallest norm)."""
    X, _, _ = _data(d, 23)
    Q = np.zeros((NQ, d), F32)
    for metric in _metrics(storage, scan):
        idx = _index(metric, storage, d, scan)
        idx.add(X)
        ref = _Ref(oracle, metric, storage, X).search(Q, K)
        if metric != "l2":
            assert np.array_equal(ref[0], np.tile(np.arange(K), (NQ, 1))) and not ref[1].view(np.uint32).any()
        what = f"zero queries {metric} {storage} {scan} d={d}"
        assert _outcome(lambda: idx.search(Q, K), ref, what) == "exact"
        assert _outcome(lambda: idx.search(Q[:1], 1), _Ref(oracle, metric, storage, X).search(Q[:1], 1), what + " nq=1 k=1") == "exact"


# ---- tiny rows
TINY_BLOCKS = [(0, 64, 2.0 ** -63), (64, 128, 2.0 ** -70), (128, 192, 2.0 ** -74), (192, 256, 2.0 ** -80), (256, 320, 1e-42),
               (320, 352, 0.0), (352, 384, 1e-10)]
TINY_END = 384
LONE_TILE = (1024, 1056, 2.0 ** -70)            # one tiny tile among ordinary ones


def _tiny_rows(d, seed):
    """Rows 0 .. 383: blocks of whole 32-row tiles on the ladder — sums of squares near FLT_MIN, subnormal (2^-70, 2^-74),
    zero from non-zero elements (2^-80, and 1e-42), subnormal elements, zero rows, 1e-10 — then ordinary rows with one
    tiny tile among them."""
    X, Q, rng = _data(d, seed)
    X64 = X.astype(np.float64)
    for a, b, s in TINY_BLOCKS + [LONE_TILE]:
        X64[a:b] *= s
    X = X64.astype(F32)
    Xp = np.zeros((N, (d + 7) // 8 * 8), F32)
    Xp[:, :d] = X
    nr = l2_ref.canon_dot(Xp, Xp)                # the canonical fp32 sum of squares (FMA chains: the squares are not rounded alone)
    assert ((nr[64:192] > 0) & (nr[64:192] < F32(FLT_MIN))).all() and not nr[192:256].any() and X[192:256].any(axis=1).all()
    return X, Q, rng


def _stored_rows_match(oracle, idx, storage, X, normalize):
    if storage == "f16":
        want = oracle.ingest_f16(X, normalize=normalize)[0]
        assert np.array_equal(idx.rows.cpu().numpy().view(np.uint16), want), "fp16 rows differ from the oracle's"
        return {"subnormal or zero halves of non-zero elements": int((((want & 0x7c00) == 0) & (oracle.pad_queries(X, want.shape[1]) != 0)).sum())}
    if storage == "f8":
        want, scales, _ = oracle.ingest_f8(X, normalize=normalize)
        assert np.array_equal(idx.row_scales.cpu().numpy().view(np.uint32), scales.view(np.uint32)), "fp8 row scales differ from the oracle's"
        assert np.array_equal(idx.rows.cpu().numpy().view(np.uint8), want), "fp8 bytes differ from the oracle's"
        return {"subnormal row scales": int(((scales > 0) & (scales < F32(FLT_MIN))).sum())}
    want = oracle.ingest_f32(X, normalize=normalize)[0]
    assert np.array_equal(idx.rows.cpu().numpy().view(np.uint32), want.view(np.uint32)), "fp32 rows differ from the oracle's"
    image = idx._image16[: idx.ntotal].cpu().numpy().view(np.uint16)
    assert np.array_equal(image, want.astype(np.float16).view(np.uint16)), "the fp16 image is not the rows rounded to nearest even"
    return {"subnormal stored elements": int(((np.abs(want) > 0) & (np.abs(want) < F32(FLT_MIN))).sum())}


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("storage, d", [(s, d) for s in ("f16", "f8", "f32") for d in (100, 256)] + [("f16", 1536), ("f32", 1536)])
def test_tiny_rows_with_ordinary_queries(oracle, storage, d, normalize):
    """First the stored rows, bit for bit (fp8: the row scales too; fp32: the fp16 image too), then the search: over all rows,
    and over the tiny blocks alone with every one of them ranked (k = 384: the order of +-0 and subnormal scores)."""
    metric = "cosine" if normalize else "ip"
    X, Q, _ = _tiny_rows(d, 24)
    for rows, k in ((X, K), (X[:TINY_END], TINY_END)):
        idx = _index(metric, storage, d)
        idx.add(rows[:1000])                    # (two adds: the second starts inside a tile)
        idx.add(rows[1000:])
        seen = _stored_rows_match(oracle, idx, storage, rows, normalize)
        print(f"tiny rows {storage} d={d} normalize={normalize} n={len(rows)}: {seen}")
        what = f"tiny rows {metric} {storage} d={d} n={len(rows)} k={k}"
        assert _outcome(lambda: idx.search(Q, k), _Ref(oracle, metric, storage, rows).search(Q, k), what) == "exact"


@pytest.mark.parametrize("storage, scan, d", COMBOS)
def test_tiny_rows_and_tiny_queries(oracle, storage, scan, d):
    """Products near FLT_MIN (2^-63 both sides), subnormal or vanishing (2^-70): the scores are subnormals and +-0, and ties
    follow (score desc, id asc) with +0 above -0."""
    X0, Q0, _ = _data(d, 25)
    for s in (2.0 ** -63, 2.0 ** -70):
        X, Q = _rung(X0, "scale", s), _rung(Q0, "scale", s)
        ref = _Ref(oracle, "ip", storage, X)
        r = ref.search(Q, K)
        idx = _index("ip", storage, d, scan)
        idx.add(X)
        what = f"tiny rows and queries {storage} {scan} d={d} scale {s:.3e}"
        print(f"{what}: largest |score| {np.abs(r[1]).max():.3e}, zero scores in the answer {int((r[1] == 0).sum())}")
        assert _outcome(lambda: idx.search(Q, K), r, what) == "exact"
        assert _outcome(lambda: idx.search(Q, 300), ref.search(Q, 300), what + " k=300") == "exact"


def test_l2norm_rows_on_the_ladder(oracle):
    """rarc_l2norm_rows_f32 == the oracle's normalize_L2, bit for bit, with a subnormal sum of squares, a sum of squares of 0
    from non-zero elements (the row stays as it is), subnormal elements and zero rows — in place and strided."""
    import torch

    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    rng = np.random.default_rng(26)
    for d in (100, 256):
        base = rng.standard_normal((8, d))
        x = np.concatenate([_rung(base, kind, value) for _, kind, value in LADDER] + [base.astype(F32)])
        want = oracle.normalize_L2(x)
        assert np.isfinite(want).all()
        dx = torch.from_numpy(x).cuda()
        out = torch.empty_like(dx)
        B.check(lib.rarc_l2norm_rows_f32(dx.data_ptr(), d, out.data_ptr(), d, len(x), d, 0))
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
        wide = torch.zeros((len(x), d + 60), dtype=torch.float32, device="cuda")        # strided, in place
        wide[:, :d] = dx
        B.check(lib.rarc_l2norm_rows_f32(wide.data_ptr(), d + 60, wide.data_ptr(), d + 60, len(x), d, 0))
        assert np.array_equal(wide.cpu().numpy()[:, :d].view(np.uint32), want.view(np.uint32)) and not wide[:, d:].any().item()
        B.check(lib.rarc_l2norm_rows_f32(dx.data_ptr(), d, dx.data_ptr(), d, len(x), d, 0))   # in place
        assert np.array_equal(dx.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("strategy", ["subset", "overfetch"])
@pytest.mark.parametrize("storage", ["f16", "f32"])
def test_filtered_search_with_a_tiny_and_a_zero_query(oracle, storage, strategy):
    X, Q0, rng = _data(256, 27)
    allowed = np.sort(rng.choice(N, 700, replace=False))
    Q = np.stack([_rung(Q0[:1], "scale", 2.0 ** -76)[0], np.zeros(256, F32), _rung(Q0[2:3], "max", EDGE * 0.99)[0], Q0[3]])
    idx = _index("ip", storage, 256)
    idx.add(X)
    rows = l2_ref.stored_rows(oracle, X, storage)
    ref_D, ref_I = subset_ref.search(oracle, rows, Q, K, allowed, "ip", False)
    what = f"filtered {storage} {strategy}"
    assert _outcome(lambda: idx.search_filtered(Q, K, idx.rowset(allowed), strategy=strategy), (ref_I, ref_D), what) == "exact"
    for j in (0, 1):                                # and each alone: the batch's score window is the tiny query's own
        one = _outcome(lambda: idx.search_filtered(Q[j: j + 1], K, idx.rowset(allowed), strategy=strategy),
                       (ref_I[j: j + 1], ref_D[j: j + 1]), f"{what} query {j} alone")
        assert one == "exact"


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_store_answers_a_zero_vector(oracle, metric):
    from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
    from tests.helpers import HashEmbeddings

    emb = HashEmbeddings(384)
    texts = [f"small range document {i}" for i in range(600)]
    ids = [f"s{i}" for i in range(600)]
    store = HipFlatVectorStore(emb, metric=metric)
    store.add_texts(texts, ids=ids)
    X = np.asarray(emb.embed_documents(texts), dtype=F32)
    ref = _Ref(oracle, metric, "f16", X).search(np.zeros((1, 384), F32), 5)
    got = store.similarity_search_by_vector([0.0] * 384, k=5)
    assert [doc.id for doc in got] == [ids[i] for i in ref[0][0]] == ids[:5]
    scored = store.similarity_search_by_vector_with_score([0.0] * 384, k=5)
    assert np.array_equal(np.asarray([s for _, s in scored], F32).view(np.uint32), ref[1][0].view(np.uint32))
