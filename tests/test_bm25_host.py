"""BM25 on the host (no GPU): the restatement of rank_bm25 0.2.2's BM25Okapi pinned by hand-computed cases, the CSR index
built from it bit for bit, the refusals, the C-ABI's argument checks, the registry entry, and the shipped code's lack of
fused multiply-adds in the BM25 kernels."""
import ctypes
import math

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B
from rag_arc_amd.hip.bm25 import Bm25Index, OkapiRestatement, check_k, topk_order


def hexes(a):
    return [float(x).hex() for x in np.asarray(a, dtype=np.float64)]


def frac(tf, dl, avgdl, k1=1.5, b=0.75):
    return tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl))


# -- the restatement, by hand ------------------------------------------------------------------------------------------
def test_three_documents_negative_epsilon():
    corpus = [["a", "b"], ["a", "c"], ["a", "b", "d"]]
    ref = OkapiRestatement(corpus)
    avgdl = 7 / 3
    idf = {w: math.log(3 - n + 0.5) - math.log(n + 0.5) for w, n in (("a", 3), ("b", 2), ("c", 1), ("d", 1))}
    idf_sum = 0
    for w in ("a", "b", "c", "d"):          # nd's order: first occurrence
        idf_sum += idf[w]
    average_idf = idf_sum / 4
    assert average_idf < 0
    eps = 0.25 * average_idf
    assert ref.average_idf == average_idf and ref.avgdl == avgdl
    assert ref.idf == {"a": eps, "b": eps, "c": idf["c"], "d": idf["d"]}
    # "b": documents 0 and 2 score below the untouched document 1
    want = [0.0 + eps * frac(1, 2, avgdl), 0.0, 0.0 + eps * frac(1, 3, avgdl)]
    got = ref.get_scores(["b"])
    assert hexes(got) == hexes(want)
    assert got[0] < 0 and got[2] < 0 and got[1] == 0.0
    assert list(topk_order(got, 3)) == [1, 2, 0]       # the shorter document 0 weighs its negative term more


def test_repeated_and_unknown_query_tokens():
    corpus = [["x", "y", "y"], ["y", "z"], ["w"], ["x", "x", "x", "z"]]
    ref = OkapiRestatement(corpus)
    avgdl = 10 / 4
    idf = {w: math.log(4 - n + 0.5) - math.log(n + 0.5) for w, n in (("x", 2), ("y", 2), ("z", 2), ("w", 1))}
    assert all(v >= 0 for v in idf.values())
    t_x = [idf["x"] * frac(1, 3, avgdl), 0.0, 0.0, idf["x"] * frac(3, 4, avgdl)]
    t_y = [idf["y"] * frac(2, 3, avgdl), idf["y"] * frac(1, 2, avgdl), 0.0, 0.0]
    want = [((0.0 + t_x[d]) + t_y[d]) + t_x[d] for d in range(4)]      # query order, the repeat applied twice
    assert hexes(ref.get_scores(["x", "y", "nope", "x"])) == hexes(want)
    assert hexes(ref.get_scores(["nope"])) == hexes([0.0] * 4)


def test_non_ascii_tokens():
    corpus = [["café", "東京", "東京"], ["naïve", "café"], ["東京"]]
    ref = OkapiRestatement(corpus)
    idx = Bm25Index.from_tokens(corpus)
    avgdl = 6 / 3
    idf_t = math.log(3 - 2 + 0.5) - math.log(2 + 0.5)   # 東京 in 2 documents: negative
    idf_c = idf_t                                       # café too
    idf_n = math.log(3 - 1 + 0.5) - math.log(1 + 0.5)
    average_idf = ((0 + idf_c) + idf_t + idf_n) / 3
    eps = 0.25 * average_idf
    want = [0.0 + (eps if average_idf < 0 else idf_t) * frac(2, 3, avgdl), 0.0,
            0.0 + (eps if average_idf < 0 else idf_t) * frac(1, 1, avgdl)]
    assert hexes(ref.get_scores(["東京"])) == hexes(want)
    assert hexes(idx.host_scores(idx.query_ids(["東京"]))) == hexes(want)
    assert list(idx.vocab) == ["café", "東京", "naïve"]


# -- the CSR index against the restatement ------------------------------------------------------------------------------
def _zipf_corpus(seed, n_docs, vocab, max_len=40):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_docs):
        ids = rng.zipf(1.2, size=int(rng.integers(0, max_len)))
        out.append([f"t{int(i)}" for i in ids if i <= vocab])
    return out


@pytest.mark.parametrize("params", [{}, {"k1": 1.2, "b": 0.5, "epsilon": 0.1}, {"b": 1.0}])
def test_csr_matches_the_restatement_bit_for_bit(params):
    corpus = _zipf_corpus(3, 600, 300)
    if params.get("b") == 1.0:
        corpus = [d or ["filler"] for d in corpus]      # b == 1 needs every document non-empty
    ref = OkapiRestatement(corpus, **params)
    idx = Bm25Index.from_tokens(corpus, params)
    assert list(idx.vocab) == list(ref.idf)             # term ids = first-occurrence order = nd's order
    assert idx.average_idf.hex() == ref.average_idf.hex() and idx.avgdl == ref.avgdl
    assert hexes(idx.idf) == hexes([ref.idf[w] for w in idx.vocab])
    # post_w: the reference's per-document fraction for every (term, doc) it has
    k1, b = params.get("k1", 1.5), params.get("b", 0.75)
    dl = np.array(ref.doc_len)
    for w, t in list(idx.vocab.items())[:60]:
        a, e = idx.post_off[t], idx.post_off[t + 1]
        docs = idx.post_doc[a:e]
        assert np.all(np.diff(docs) > 0)
        q_freq = np.array([(d.get(w) or 0) for d in ref.doc_freqs])
        full = q_freq * (k1 + 1) / (q_freq + k1 * (1 - b + b * dl / ref.avgdl))
        assert hexes(idx.post_w[a:e]) == hexes(full[docs])
        assert set(docs.tolist()) == set(np.flatnonzero(q_freq).tolist())
    rng = np.random.default_rng(5)
    words = list(ref.idf)
    for _ in range(20):
        q = [words[int(i)] for i in rng.integers(0, len(words), size=5)] + ["unknown"]
        assert hexes(idx.host_scores(idx.query_ids(q))) == hexes(ref.get_scores(q))


def test_token_ids_and_tokens_build_the_same_index():
    corpus = _zipf_corpus(9, 300, 200)
    by_tok = Bm25Index.from_tokens(corpus)
    ids = [by_tok.vocab[w] for d in corpus for w in d]
    off = np.cumsum([0] + [len(d) for d in corpus])
    by_id = Bm25Index.from_token_ids(off, ids)
    for name in ("post_off", "post_doc", "post_w", "idf"):
        assert np.array_equal(getattr(by_tok, name), getattr(by_id, name)), name
    assert by_tok.average_idf == by_id.average_idf


def test_token_ids_sum_idf_in_first_occurrence_order():
    """Ids that do not ascend in first-occurrence order: average_idf is still summed in nd's order."""
    corpus = [[5, 1, 9], [9, 2], [1, 1, 7], [3]]
    ref = OkapiRestatement(corpus)
    idx = Bm25Index.from_token_ids(np.cumsum([0, 3, 2, 3, 1]), [t for d in corpus for t in d], n_terms=12)
    assert idx.average_idf.hex() == ref.average_idf.hex()
    assert idx.known_ids([5, 4, 11, 9, 99]) == [5, 9]
    assert hexes(idx.host_scores([9, 1])) == hexes(ref.get_scores([9, 1]))


# -- refusals (before anything is uploaded) -----------------------------------------------------------------------------
def test_refusals():
    good = [["a", "b"], ["c"]]
    for k1 in (0.0, -1.0):
        with pytest.raises(ValueError, match="k1"):
            Bm25Index.from_tokens(good, {"k1": k1})
    with pytest.raises(ValueError):
        Bm25Index.from_tokens(good, {"k1": float("nan")})
    with pytest.raises(ValueError):
        Bm25Index.from_tokens(good, {"delta": 1.0})
    with pytest.raises(B.RarcUnsupported, match="NaN"):
        Bm25Index.from_tokens([["a"], [], ["b"]], {"b": 1.0})
    Bm25Index.from_tokens([["a"], ["c"], ["b"]], {"b": 1.0})          # b == 1 without an empty document: fine
    with pytest.raises(B.RarcUnsupported, match="empty"):
        Bm25Index.from_tokens([[], []])
    with pytest.raises(ValueError, match="empty corpus"):
        Bm25Index.from_tokens([])
    for k in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            check_k(k, 10)
    assert check_k(5000, 700) == 700                                  # effective k = min(k, n_docs)
    assert check_k(1024, 5000) == 1024
    with pytest.raises(B.RarcUnsupported, match="1024"):
        check_k(1025, 5000)


def test_retriever_refuses_before_upload():
    from rag_arc_amd.core.retrieval.bm25 import HipBM25Retriever

    with pytest.raises(ValueError):
        HipBM25Retriever.from_texts(["a b", "c"], k=0, warn_default_preprocess=False)
    with pytest.raises(ValueError, match="k1"):
        HipBM25Retriever.from_texts(["a b", "c"], bm25_params={"k1": 0}, warn_default_preprocess=False)
    with pytest.raises(B.RarcUnsupported):
        HipBM25Retriever.from_texts(["a b", ""], bm25_params={"b": 1}, warn_default_preprocess=False)
    r = HipBM25Retriever(k=3, warn_default_preprocess=False)
    assert r.get_name() == "BM25Retriever" and r.get_document_count() == 0
    with pytest.raises(ValueError):
        r.update_k(0)
    with pytest.raises(ValueError):
        r.invoke("a")                                                 # no index


# -- C-ABI --------------------------------------------------------------------------------------------------------------
def test_cabi_rejects_bad_arguments_without_a_gpu():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    p = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
    ws = lib.rarc_bm25_workspace_bytes(4, 32, 100_000, 100)
    assert ws >= 4 * 13 * 100 * 12
    assert lib.rarc_bm25_workspace_bytes(4, 32, 0, 100) == 0
    assert lib.rarc_bm25_workspace_bytes(4, 32, 100, 1025) == 0
    args = lambda **kw: [kw.get(n, v) for n, v in (("off", p), ("doc", p), ("w", p), ("terms", 50), ("n", 100_000),
                                                   ("qoff", p), ("qterm", p), ("qidf", p), ("nq", 4), ("ntok", 32))]
    topk = lambda k=100, ws_bytes=ws, out=p, **kw: lib.rarc_bm25_topk(*args(**kw), k, p, ws_bytes, out, p, None)
    assert topk(off=None) == -1 and b"null pointer" in lib.rarc_last_error()
    assert topk(qterm=None) == -1
    assert topk(out=None) == -1
    assert topk(k=0) == -4 and b"k=0" in lib.rarc_last_error()
    assert topk(k=1025) == -4
    assert topk(k=11, n=10) == -4                                      # k > n_docs
    assert topk(nq=-1) == -1
    assert topk(terms=0) == -1 and b"terms" in lib.rarc_last_error()
    assert topk(n=0) == -4
    assert topk(n=1 << 31) == -4
    assert topk(ws_bytes=ws - 1) == -3 and b"workspace" in lib.rarc_last_error()
    sc = lambda ws_bytes=ws, **kw: lib.rarc_bm25_scores(*args(**kw), p, ws_bytes, p, None)
    assert sc(doc=None) == -1
    assert lib.rarc_bm25_scores(*args(), p, ws, None, None) == -1
    assert sc(ws_bytes=0) == -3
    with pytest.raises(B.RarcError, match="rarc_bm25_scores"):
        B.check(sc(ws_bytes=0), "rarc_bm25_scores")


def test_bm25_kernels_have_no_fused_multiply_add():
    from tests import codeobj

    if not codeobj.os.path.exists(codeobj.LIB):
        pytest.skip("librarc_hip.so not built")
    kernels = codeobj.disassemble("rarc_bm25_")
    assert {n for n in kernels if "tile_kernel" in n} and {n for n in kernels if "merge_kernel" in n}, list(kernels)
    for name, ins in kernels.items():
        fused = [i for i in ins if i.split()[0].startswith(("v_fma_f64", "v_fmac_f64"))]
        assert not fused, f"{name}: {fused[:3]}"
    tile = next(ins for n, ins in kernels.items() if "tile_kernelILb1" in n)
    assert any(i.startswith("v_mul_f64") for i in tile) and any(i.startswith("v_add_f64") for i in tile)


# -- registry -----------------------------------------------------------------------------------------------------------
def test_json_multipath_config_with_a_bm25_arm_parses():
    import json

    from rag_arc_amd.config.modules import HipBM25RetrieverConfig, MultiPathRetrieverConfig, VectorStoreRetrieverConfig

    cfg = json.loads("""{"type": "multipath_retriever", "top_k_per_retriever": 20, "fusion": {"type": "rrf", "k": 60.0},
        "retrievers": [{"type": "vectorstore_retriever", "vectorstore": {"type": "hip_flat_vectorstore",
                          "embedding": {"type": "table_embeddings", "path": "emb.npz"}, "corpus_path": "c.npz"}},
                       {"type": "hip_bm25_retriever", "corpus_path": "c.npz", "k1": 1.2, "b": 0.7, "epsilon": 0.3}]}""")
    m = MultiPathRetrieverConfig(**cfg)
    assert isinstance(m.retrievers[0], VectorStoreRetrieverConfig)
    bm = m.retrievers[1]
    assert isinstance(bm, HipBM25RetrieverConfig)
    assert (bm.k1, bm.b, bm.epsilon, bm.k, bm.index_path) == (1.2, 0.7, 0.3, 5, None)
