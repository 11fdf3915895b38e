"""Okapi BM25 on the MI355X: the host index build, the restatement it is checked against, and the device index.

The reference's BM25Retriever (core/retrieval/bm25.py:215-217, :303-305) scores with rank_bm25 0.2.2's `BM25Okapi`.
rank_bm25 is not a dependency here; `OkapiRestatement` restates that class from its published source (rank_bm25.py,
classes BM25 and BM25Okapi: `_initialize`, `_calc_idf`, `get_scores`) and is the yardstick the device scores are
compared with bit for bit.  `Bm25Index` is the same arithmetic laid out as a term-major CSR:

    post_off [V+1] int64   postings of term t: [post_off[t], post_off[t+1])
    post_doc       int32   ascending within a term
    post_w         fp64    tf*(k1+1) / (tf + k1*((1-b) + b*dl/avgdl))      (the reference's expression, its rounding)
    idf [V]        fp64    log(N - n + 0.5) - log(n + 0.5), or epsilon * average_idf where that is negative

score[d] = sum over the query's tokens, in order, duplicates included, of idf * w[d]; a document a token does not reach
adds an exact zero in the reference, so only postings are visited.  Term ids are first-occurrence order (documents in
order, words in order within a document), the order of rank_bm25's `nd` dict, in which average_idf is summed.

Configurations where the reference itself computes NaN are refused before anything is uploaded: a document whose
length term k1*((1-b) + b*dl/avgdl) is zero (k1 == 0, or b == 1 with an empty document) makes 0/0 for every token it
lacks; an all-empty corpus has avgdl = 0.
"""
from __future__ import annotations

import math
import threading
from typing import Dict, Hashable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .binding import RarcUnsupported

MAX_K = 1024                 # rarc_bm25_topk selects at most this many per query
MAX_DOCS = 0x7fffffff - 8192  # rarc_bm25_*: n_docs limit (one 8192-document tile below 2^31)
DEFAULTS = {"k1": 1.5, "b": 0.75, "epsilon": 0.25}


def okapi_params(bm25_params: Optional[dict] = None) -> Tuple[float, float, float]:
    """(k1, b, epsilon) of BM25Okapi(corpus, **bm25_params), checked.  Only those three keywords are meaningful here
    (rank_bm25's `tokenizer` keyword is what `preprocess_func` does)."""
    p = dict(DEFAULTS)
    for name, v in (bm25_params or {}).items():
        if name not in p:
            raise ValueError(f"bm25_params: unknown parameter {name!r} (k1, b, epsilon)")
        p[name] = v
    k1, b, eps = (float(p[n]) for n in ("k1", "b", "epsilon"))
    if not all(math.isfinite(v) for v in (k1, b, eps)):
        raise ValueError(f"bm25_params must be finite: k1={k1} b={b} epsilon={eps}")
    if k1 <= 0:
        raise ValueError(f"bm25_params: k1={k1} must be > 0 (k1 <= 0 gives 0/0 = NaN for every document a token misses)")
    return k1, b, eps


def check_k(k, n_docs: int) -> int:
    """The effective k of a query (min(k, n_docs), as the reference's _get_relevant_documents): > 0 and <= MAX_K."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k <= 0:
        raise ValueError(f"k must be a positive integer, got {k!r}")
    k = min(int(k), int(n_docs))
    if k > MAX_K:
        raise RarcUnsupported(f"BM25 top-k: k={k} exceeds {MAX_K} (the kernel's selection limit); ask for at most {MAX_K} "
                              f"or use get_scores() for every document's score")
    return k


class OkapiRestatement:
    """rank_bm25 0.2.2 BM25Okapi, restated: dict-based index, numpy float64 get_scores.  The yardstick, not a fast path."""

    def __init__(self, corpus: Sequence[Sequence[Hashable]], k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25):
        self.k1, self.b, self.epsilon = k1, b, epsilon
        self.corpus_size = 0
        self.avgdl = 0
        self.doc_freqs: List[Dict] = []
        self.idf: Dict = {}
        self.doc_len: List[int] = []
        nd = self._initialize(corpus)
        self._calc_idf(nd)

    def _initialize(self, corpus):
        nd = {}
        num_doc = 0
        for document in corpus:
            self.doc_len.append(len(document))
            num_doc += len(document)
            frequencies = {}
            for word in document:
                if word not in frequencies:
                    frequencies[word] = 0
                frequencies[word] += 1
            self.doc_freqs.append(frequencies)
            for word, freq in frequencies.items():
                try:
                    nd[word] += 1
                except KeyError:
                    nd[word] = 1
            self.corpus_size += 1
        self.avgdl = num_doc / self.corpus_size
        return nd

    def _calc_idf(self, nd):
        idf_sum = 0
        negative_idfs = []
        for word, freq in nd.items():
            idf = math.log(self.corpus_size - freq + 0.5) - math.log(freq + 0.5)
            self.idf[word] = idf
            idf_sum += idf
            if idf < 0:
                negative_idfs.append(word)
        self.average_idf = idf_sum / len(self.idf)
        eps = self.epsilon * self.average_idf
        for word in negative_idfs:
            self.idf[word] = eps

    def get_scores(self, query):
        score = np.zeros(self.corpus_size)
        doc_len = np.array(self.doc_len)
        for q in query:
            q_freq = np.array([(doc.get(q) or 0) for doc in self.doc_freqs])
            score += (self.idf.get(q) or 0) * (q_freq * (self.k1 + 1) /
                                               (q_freq + self.k1 * (1 - self.b + self.b * doc_len / self.avgdl)))
        return score


def topk_order(scores: np.ndarray, k: int) -> np.ndarray:
    """Indices of the k best scores: score descending, index ascending among equal scores (the tie order this backend
    defines where the reference's reversed argsort leaves it open)."""
    scores = np.asarray(scores, dtype=np.float64)
    k = min(int(k), scores.size)
    cand = np.arange(scores.size)
    if k < scores.size:       # everything at or above the k-th largest value, then the exact order among those
        kth = np.partition(scores, scores.size - k)[scores.size - k]
        cand = np.flatnonzero(scores >= kth)
    return cand[np.lexsort((cand, -scores[cand]))[:k]]


def synthetic_zipf(n_docs: int, mean_len: int, n_terms: int, seed: int, s: float = 1.0):
    """(doc_offsets, term_ids) of a seeded corpus: document lengths uniform in [mean_len/2, 3*mean_len/2], terms drawn
    from a Zipf(s) law over n_terms ranks (rank r has weight 1/r^s)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(max(mean_len // 2, 0), mean_len + mean_len // 2 + 1, size=n_docs)
    off = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off, zipf_terms(rng, int(off[-1]), n_terms, s)


def zipf_terms(rng, n: int, n_terms: int, s: float = 1.0) -> np.ndarray:
    """n term ids drawn from Zipf(s) over n_terms ranks (inverse CDF)."""
    cdf = np.cumsum(1.0 / np.arange(1, n_terms + 1, dtype=np.float64) ** s)
    cdf /= cdf[-1]
    out = np.empty(n, dtype=np.int64)
    for c0 in range(0, n, 1 << 24):
        c1 = min(n, c0 + (1 << 24))
        out[c0:c1] = np.minimum(np.searchsorted(cdf, rng.random(c1 - c0), side="right"), n_terms - 1)
    return out


class Bm25Index:
    """The BM25Okapi index as a term-major CSR (host arrays), plus `vocab` (token -> term id) when built from tokens."""

    def __init__(self, post_off, post_doc, post_w, idf, present, doc_len, avgdl, average_idf, k1, b, epsilon, vocab=None):
        self.post_off, self.post_doc, self.post_w = post_off, post_doc, post_w
        self.idf, self.present, self.doc_len = idf, present, doc_len
        self.avgdl, self.average_idf = avgdl, average_idf
        self.k1, self.b, self.epsilon = k1, b, epsilon
        self.vocab: Optional[Dict[Hashable, int]] = vocab

    @property
    def n_docs(self) -> int:
        return int(self.doc_len.size)

    @property
    def n_terms(self) -> int:
        return int(self.idf.size)

    @property
    def vocab_size(self) -> int:
        """Distinct terms of the corpus (len(BM25Okapi.idf))."""
        return int(self.present.sum())

    # -- construction -------------------------------------------------------------------------------------------------
    @classmethod
    def from_tokens(cls, corpus: Sequence[Sequence[Hashable]], bm25_params: Optional[dict] = None) -> "Bm25Index":
        """From tokenised documents (what preprocess_func returns).  Term ids in first-occurrence order."""
        vocab: Dict[Hashable, int] = {}
        lens = np.zeros(len(corpus) + 1, dtype=np.int64)
        ids: List[int] = []
        for d, doc in enumerate(corpus):
            for tok in doc:
                tid = vocab.get(tok)
                if tid is None:
                    tid = vocab[tok] = len(vocab)
                ids.append(tid)
            lens[d + 1] = len(doc)
        idx = cls.from_token_ids(np.cumsum(lens), np.asarray(ids, dtype=np.int64), n_terms=len(vocab),
                                 bm25_params=bm25_params)
        idx.vocab = vocab
        return idx

    @classmethod
    def from_token_ids(cls, doc_offsets, term_ids, n_terms: Optional[int] = None,
                       bm25_params: Optional[dict] = None) -> "Bm25Index":
        """From term ids directly: document d is term_ids[doc_offsets[d]:doc_offsets[d+1]].  Terms that never occur have
        no postings and count as unknown tokens.  average_idf is summed in first-occurrence order of the ids, as
        rank_bm25's `nd` dict would hold them."""
        k1, b, epsilon = okapi_params(bm25_params)
        off = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        tids = np.ascontiguousarray(term_ids, dtype=np.int64)
        if off.ndim != 1 or off.size < 1 or off[0] != 0 or off[-1] != tids.size or np.any(np.diff(off) < 0):
            raise ValueError("doc_offsets must be [n_docs + 1], start at 0, not decrease and end at len(term_ids)")
        n = int(off.size - 1)
        if n == 0:
            raise ValueError("BM25 over an empty corpus (the reference divides by corpus_size = 0)")
        if n > MAX_DOCS:
            raise RarcUnsupported(f"BM25: {n} documents exceed {MAX_DOCS}")
        if tids.size and tids.min() < 0:
            raise ValueError("term ids must be >= 0")
        V = int(n_terms) if n_terms is not None else (int(tids.max()) + 1 if tids.size else 0)
        if tids.size and tids.max() >= V:
            raise ValueError(f"term id {int(tids.max())} >= n_terms={V}")
        if V >= 2 ** 31:
            raise RarcUnsupported(f"BM25: {V} terms exceed 2^31 - 1")
        doc_len = np.diff(off)
        total = int(doc_len.sum())
        if total == 0:
            raise RarcUnsupported("BM25 over a corpus whose documents are all empty: avgdl = 0, the reference's scores "
                                  "are NaN")
        avgdl = total / n                                        # num_doc / corpus_size (python int / int)
        # per-document length term k1 * (1 - b + b * dl / avgdl), with the reference's rounding
        dpart = k1 * ((1 - b) + (b * doc_len.astype(np.float64)) / avgdl)
        bad = np.flatnonzero(~(dpart != 0) | ~np.isfinite(dpart))
        if bad.size:
            raise RarcUnsupported(f"BM25 with k1={k1} b={b}: document {int(bad[0])} (length {int(doc_len[bad[0]])}) has "
                                  f"k1*(1 - b + b*dl/avgdl) = {float(dpart[bad[0]])}, which makes the reference's score of "
                                  f"every token it lacks 0/0 = NaN (b == 1 with an empty document does this)")
        # postings: (term, doc) pairs with their counts, term-major, doc ascending
        doc_of = np.repeat(np.arange(n, dtype=np.int64), doc_len)
        pair, tf = np.unique(tids * n + doc_of, return_counts=True)
        post_term = pair // n
        post_doc = (pair - post_term * n).astype(np.int32)
        df = np.bincount(post_term, minlength=V)
        post_off = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(df, out=post_off[1:])
        present = df > 0
        # idf per distinct document frequency, with math.log (the reference's function)
        idf = np.zeros(V, dtype=np.float64)
        uniq, inv = np.unique(df[present], return_inverse=True)
        vals = np.array([math.log(n - int(f) + 0.5) - math.log(int(f) + 0.5) for f in uniq], dtype=np.float64)
        idf[present] = vals[inv]
        # idf_sum in nd's order (first occurrence), sequentially: np.cumsum adds left to right
        terms_seen, first = np.unique(tids, return_index=True)
        order = terms_seen[np.argsort(first, kind="stable")]
        idf_sum = float(np.cumsum(idf[order])[-1])
        average_idf = idf_sum / int(order.size)
        eps = epsilon * average_idf
        idf[present & (idf < 0)] = eps
        tf_f = tf.astype(np.float64)
        post_w = (tf_f * (k1 + 1)) / (tf_f + dpart[post_doc])
        return cls(post_off, post_doc, post_w, idf, present, doc_len, avgdl, average_idf, k1, b, epsilon)

    # -- queries ------------------------------------------------------------------------------------------------------
    def query_ids(self, tokens: Iterable[Hashable]) -> List[int]:
        """Term ids of a tokenised query, in order, duplicates kept, unknown tokens left out."""
        if self.vocab is None:
            raise ValueError("this index was built from term ids: pass term ids (query_term_ids)")
        out = []
        for t in tokens:
            tid = self.vocab.get(t)
            if tid is not None:
                out.append(tid)
        return out

    def known_ids(self, term_ids: Iterable[int]) -> List[int]:
        """Term ids that have postings, in order (ids of terms the corpus lacks are unknown tokens)."""
        out = []
        for t in term_ids:
            t = int(t)
            if 0 <= t < self.n_terms and self.present[t]:
                out.append(t)
        return out

    def host_scores(self, term_ids: Sequence[int]) -> np.ndarray:
        """The restatement over the CSR (vectorised numpy): every document's score for one query of KNOWN term ids."""
        score = np.zeros(self.n_docs)
        for t in term_ids:
            a, b = self.post_off[t], self.post_off[t + 1]
            d = self.post_doc[a:b]
            score[d] = score[d] + self.idf[t] * self.post_w[a:b]
        return score


def pack_queries(queries: Sequence[Sequence[int]], idf: np.ndarray):
    """(q_off int32 [nq+1], q_term int32, q_idf fp64) of queries given as known term ids."""
    q_off = np.zeros(len(queries) + 1, dtype=np.int64)
    np.cumsum([len(q) for q in queries], out=q_off[1:])
    if q_off[-1] > 0x7fffffff:
        raise RarcUnsupported(f"BM25 batch: {int(q_off[-1])} query tokens exceed 2^31 - 1")
    q_term = np.fromiter((t for q in queries for t in q), dtype=np.int32, count=int(q_off[-1]))
    return q_off.astype(np.int32), q_term, idf[q_term].astype(np.float64)


class Bm25Device:
    """A Bm25Index uploaded once to one GPU; top-k and dense scores through rarc_bm25_topk / rarc_bm25_scores.
    Calls are serialised by a lock (the workspace and the device selection are per call)."""

    def __init__(self, index: Bm25Index, device: int = 0):
        import torch

        from . import binding as B

        self._lib = B.load_library()
        self.index = index
        self.device = int(device)
        self._dev = torch.device("cuda", self.device)
        self._lock = threading.Lock()
        with torch.cuda.device(self._dev):
            self.post_off = torch.from_numpy(index.post_off).to(self._dev)
            self.post_doc = torch.from_numpy(index.post_doc).to(self._dev)
            self.post_w = torch.from_numpy(index.post_w).to(self._dev)
            torch.cuda.current_stream(self._dev).synchronize()

    def _queries(self, queries: Sequence[Sequence[int]]):
        import torch

        q_off, q_term, q_idf = pack_queries(queries, self.index.idf)
        t = [torch.from_numpy(a).to(self._dev) for a in (q_off, q_term, q_idf)]
        return t, int(q_term.size)

    def topk(self, queries: Sequence[Sequence[int]], k: int) -> Tuple[np.ndarray, np.ndarray]:
        """(ids int64 [nq][k], scores fp64 [nq][k]) of queries given as known term ids; k already effective
        (check_k).  One launch sequence for the whole batch, in chunks of 65535 queries."""
        import torch

        from . import binding as B

        k = check_k(k, self.index.n_docs)
        nq = len(queries)
        ids = np.empty((nq, k), dtype=np.int64)
        scores = np.empty((nq, k), dtype=np.float64)
        with self._lock, torch.cuda.device(self._dev):
            for c0 in range(0, nq, 65535):
                part = queries[c0:c0 + 65535]
                (q_off, q_term, q_idf), n_tok = self._queries(part)
                ws_bytes = self._lib.rarc_bm25_workspace_bytes(len(part), n_tok, self.index.n_docs, k)
                ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=self._dev)
                out_i = torch.empty((len(part), k), dtype=torch.int64, device=self._dev)
                out_s = torch.empty((len(part), k), dtype=torch.float64, device=self._dev)
                stream = torch.cuda.current_stream(self._dev)
                B.check(self._lib.rarc_bm25_topk(self.post_off.data_ptr(), self.post_doc.data_ptr(), self.post_w.data_ptr(),
                                                 self.index.n_terms, self.index.n_docs, q_off.data_ptr(),
                                                 q_term.data_ptr(), q_idf.data_ptr(), len(part), n_tok, k, ws.data_ptr(),
                                                 ws.numel(), out_i.data_ptr(), out_s.data_ptr(), stream.cuda_stream),
                        "rarc_bm25_topk")
                ids[c0:c0 + len(part)] = out_i.cpu().numpy()
                scores[c0:c0 + len(part)] = out_s.cpu().numpy()
        return ids, scores

    def scores(self, queries: Sequence[Sequence[int]]) -> np.ndarray:
        """Every document's score, fp64 [nq][n_docs], of queries given as known term ids."""
        import torch

        from . import binding as B

        nq = len(queries)
        out = np.empty((nq, self.index.n_docs), dtype=np.float64)
        if nq == 0:
            return out
        with self._lock, torch.cuda.device(self._dev):
            for c0 in range(0, nq, 65535):
                part = queries[c0:c0 + 65535]
                (q_off, q_term, q_idf), n_tok = self._queries(part)
                ws_bytes = self._lib.rarc_bm25_workspace_bytes(len(part), n_tok, self.index.n_docs, 0)
                ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=self._dev)
                dev_out = torch.empty((len(part), self.index.n_docs), dtype=torch.float64, device=self._dev)
                stream = torch.cuda.current_stream(self._dev)
                B.check(self._lib.rarc_bm25_scores(self.post_off.data_ptr(), self.post_doc.data_ptr(),
                                                   self.post_w.data_ptr(), self.index.n_terms, self.index.n_docs,
                                                   q_off.data_ptr(), q_term.data_ptr(), q_idf.data_ptr(), len(part), n_tok,
                                                   ws.data_ptr(), ws.numel(), dev_out.data_ptr(), stream.cuda_stream),
                        "rarc_bm25_scores")
                out[c0:c0 + len(part)] = dev_out.cpu().numpy()
        return out
