"""Lexical retriever on the MI355X (reference: core/retrieval/bm25.py:30-500, BM25Retriever over rank_bm25's BM25Okapi).

Same surface as the reference: from_texts / from_documents, invoke / ainvoke (k = min(kwargs k or self.k, #docs)),
get_scores, get_top_k_with_scores (k = k or self.k), add_documents / delete_documents and their async twins (each rebuilds
the whole index; ids=None deletes everything), get_document_count, get_bm25_info, update_k, get_name ("BM25Retriever"),
save_to_disk / load_from_disk (dill).  Scores are bit-identical to BM25Okapi's float64 (rag_arc_amd.hip.bm25); where the
reference's reversed argsort leaves the order of equal scores open, this one returns score descending, document index
ascending.  Preprocessing stays a python callable; the scoring and the top-k run in librarc_hip.so (csrc/bm25.hip).
`vectorizer` is the device index (rag_arc_amd.hip.bm25.Bm25Device), not a BM25Okapi object.
"""
import asyncio
import logging
import os
import threading
import uuid
import warnings
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Callable, Dict, Iterable, List, Optional, Tuple

import numpy as np

from ..utils.data_model import Document
from .base import BaseRetriever

logger = logging.getLogger(__name__)


def default_preprocessing_func(text: str) -> List[str]:
    """Whitespace split (the reference's default, bm25.py:16-26)."""
    return text.split()


class HipBM25Retriever(BaseRetriever):
    def __init__(self, vectorizer=None, docs=None, k: int = 5,
                 preprocess_func: Callable[[str], List[str]] = default_preprocessing_func,
                 bm25_params: Optional[Dict[str, Any]] = None, device: int = 0, warn_default_preprocess: bool = True,
                 **kwargs):
        super().__init__(**kwargs)
        self._validate_k(k)
        if not callable(preprocess_func):
            raise ValueError("preprocess_func must be callable")
        self.vectorizer = vectorizer
        self.docs = docs if docs is not None else []
        self.k = k
        self.preprocess_func = preprocess_func
        self.bm25_params = dict(bm25_params or {})
        self.device = device
        self._lock = threading.Lock()
        if warn_default_preprocess and preprocess_func is default_preprocessing_func:
            warnings.warn("the default preprocess_func splits on whitespace; give one of your own for other languages",
                          UserWarning, stacklevel=2)

    @staticmethod
    def _validate_k(k) -> None:
        if isinstance(k, bool) or not isinstance(k, int) or k <= 0:
            raise ValueError(f"k must be > 0, got {k!r}")

    # -- construction -------------------------------------------------------------------------------------------------
    @classmethod
    def _index(cls, texts: Iterable[str], preprocess_func, bm25_params, device: int):
        from ...hip.bm25 import Bm25Device, Bm25Index

        index = Bm25Index.from_tokens([preprocess_func(t) for t in texts], bm25_params)   # refusals happen here
        return Bm25Device(index, device=device)

    @classmethod
    def from_texts(cls, texts: Iterable[str], metadatas: Optional[Iterable[Dict[str, Any]]] = None,
                   ids: Optional[Iterable[str]] = None, bm25_params: Optional[Dict[str, Any]] = None,
                   preprocess_func: Callable[[str], List[str]] = default_preprocessing_func, device: int = 0,
                   **kwargs: Any) -> "HipBM25Retriever":
        texts = list(texts)
        if not texts:
            raise ValueError("texts must not be empty")
        metadatas = list(metadatas) if metadatas is not None else [{} for _ in texts]
        ids = list(ids) if ids is not None else [str(uuid.uuid4()) for _ in texts]
        if len(metadatas) != len(texts) or len(ids) != len(texts):
            raise ValueError(f"{len(texts)} texts, {len(metadatas)} metadatas, {len(ids)} ids")
        warn = kwargs.pop("warn_default_preprocess", preprocess_func is default_preprocessing_func)
        cls._validate_k(kwargs.get("k", 5))
        vectorizer = cls._index(texts, preprocess_func, bm25_params, device)
        docs = [Document(content=t, metadata=m, id=i) for t, m, i in zip(texts, metadatas, ids)]
        return cls(vectorizer=vectorizer, docs=docs, preprocess_func=preprocess_func, bm25_params=bm25_params,
                   device=device, warn_default_preprocess=warn, **kwargs)

    @classmethod
    def from_documents(cls, documents: Iterable[Document], bm25_params: Optional[Dict[str, Any]] = None,
                       preprocess_func: Callable[[str], List[str]] = default_preprocessing_func,
                       **kwargs: Any) -> "HipBM25Retriever":
        docs = list(documents)
        if not docs:
            raise ValueError("documents must not be empty")
        return cls.from_texts([d.content for d in docs], [d.metadata for d in docs], [d.id for d in docs],
                              bm25_params=bm25_params, preprocess_func=preprocess_func, **kwargs)

    def _rebuild(self) -> None:
        self.vectorizer = (self._index([d.content for d in self.docs], self.preprocess_func, self.bm25_params, self.device)
                           if len(self.docs) else None)

    # -- queries ------------------------------------------------------------------------------------------------------
    def _require_index(self) -> None:
        if self.vectorizer is None:
            raise ValueError("the BM25 index is not built")

    def _topk(self, queries: List[str], k: int) -> Tuple[np.ndarray, np.ndarray]:
        from ...hip.bm25 import check_k

        k = check_k(k, len(self.docs))
        with self._lock:
            index = self.vectorizer.index
            terms = [index.query_ids(self.preprocess_func(q)) for q in queries]
            return self.vectorizer.topk(terms, k)

    def _to_docs(self, rows: np.ndarray) -> List[List[Document]]:
        from ...encapsulation.database.vector_db.docstore import ColumnarDocstore
        from ...hip import hostmap

        seq = self.docs.columns() if isinstance(self.docs, ColumnarDocstore) else self.docs
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        return hostmap.load().rows_to_docs(seq, rows, rows.shape[0], rows.shape[1])

    def _get_relevant_documents(self, query: str, **kwargs: Any) -> List[Document]:
        return self.batch_invoke([query], **kwargs)[0]

    def batch_invoke(self, inputs: List[str], **kwargs: Any) -> List[List[Document]]:
        """invoke() for a list of queries in one launch sequence (element i equals invoke(inputs[i], **kwargs))."""
        self._require_index()
        inputs = list(inputs)
        if not len(self.docs):
            logger.warning("no documents: empty answer")
            return [[] for _ in inputs]
        if not inputs:
            return []
        rows, _ = self._topk(inputs, kwargs.get("k", self.k))
        return self._to_docs(rows)

    def get_scores(self, query: str) -> List[float]:
        """Every document's BM25 score (fp64), in document order."""
        self._require_index()
        with self._lock:
            terms = self.vectorizer.index.query_ids(self.preprocess_func(query))
            return self.vectorizer.scores([terms])[0].tolist()

    def get_top_k_with_scores(self, query: str, k: Optional[int] = None) -> List[Tuple[Document, float]]:
        self._require_index()
        if not len(self.docs):
            return []
        rows, scores = self._topk([query], k or self.k)
        return [(self.docs[int(r)], float(s)) for r, s in zip(rows[0], scores[0])]

    # -- updates: every one rebuilds the index (as the reference's do) --------------------------------------------------
    def add_documents(self, documents: List[Document], **kwargs: Any) -> List[str]:
        if not documents:
            return []
        total = len(self.docs) + len(documents)
        if total > kwargs.get("rebuild_threshold", 1000):
            warnings.warn(f"rebuilding the BM25 index over {total} documents", RuntimeWarning, stacklevel=2)
        old_docs, old_vec = self.docs, self.vectorizer
        self.docs = list(self.docs) + list(documents)
        try:
            self._rebuild()
        except Exception:
            self.docs, self.vectorizer = old_docs, old_vec
            raise
        logger.info("added %d documents, rebuilt the BM25 index", len(documents))
        return [d.id for d in documents if d.id is not None]

    async def aadd_documents(self, documents: List[Document], **kwargs: Any) -> List[str]:
        loop = asyncio.get_event_loop()
        with ThreadPoolExecutor() as pool:
            return await loop.run_in_executor(pool, lambda: self.add_documents(documents, **kwargs))

    def delete_documents(self, ids: Optional[List[str]] = None, **kwargs: Any) -> bool:
        """ids = None deletes everything."""
        if ids is None:
            self.docs = []
            self.vectorizer = None
            return True
        gone = set(ids)
        kept = [d for d in self.docs if d.id not in gone]
        deleted = len(self.docs) - len(kept)
        if deleted > 0:
            if len(kept) > kwargs.get("rebuild_threshold", 1000):
                warnings.warn(f"rebuilding the BM25 index over {len(kept)} documents", RuntimeWarning, stacklevel=2)
            old_docs, old_vec = self.docs, self.vectorizer
            self.docs = kept
            try:
                self._rebuild()
            except Exception:
                self.docs, self.vectorizer = old_docs, old_vec
                raise
            logger.info("deleted %d documents, rebuilt the BM25 index", deleted)
        return deleted > 0

    async def adelete_documents(self, ids: Optional[List[str]] = None, **kwargs: Any) -> bool:
        loop = asyncio.get_event_loop()
        with ThreadPoolExecutor() as pool:
            return await loop.run_in_executor(pool, lambda: self.delete_documents(ids, **kwargs))

    # -- information --------------------------------------------------------------------------------------------------
    def get_document_count(self) -> int:
        return len(self.docs)

    def get_bm25_info(self) -> Dict[str, Any]:
        info = {"document_count": len(self.docs), "k": self.k, "bm25_params": self.bm25_params,
                "preprocess_func": getattr(self.preprocess_func, "__name__", repr(self.preprocess_func)),
                "has_vectorizer": self.vectorizer is not None}
        if self.vectorizer is not None:
            info.update({"vocab_size": self.vectorizer.index.vocab_size,
                         "average_doc_length": self.vectorizer.index.avgdl})
        return info

    def update_k(self, new_k: int) -> None:
        self._validate_k(new_k)
        self.k = new_k

    def get_name(self) -> str:
        return "BM25Retriever"

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(docs={len(self.docs)}, k={self.k}, "
                f"preprocess_func={getattr(self.preprocess_func, '__name__', '?')})")

    # -- persistence (dill, as the reference): the host CSR, not the token lists -------------------------------------
    def save_to_disk(self, path: str) -> None:
        import dill

        if not path.endswith(".pkl"):
            path = os.path.join(path, "bm25.pkl")
        state = {"index": None if self.vectorizer is None else self.vectorizer.index, "docs": self.docs, "k": self.k,
                 "preprocess_func": self.preprocess_func, "bm25_params": self.bm25_params}
        try:
            with open(path, "wb") as fh:
                dill.dump(state, fh)
        except Exception as exc:
            raise IOError(f"saving the BM25 retriever failed: {exc}") from exc

    @classmethod
    def load_from_disk(cls, path: str, device: int = 0) -> "HipBM25Retriever":
        import dill

        from ...hip.bm25 import Bm25Device

        if not os.path.exists(path):
            raise IOError(f"no such file: {path}")
        with open(path, "rb") as fh:
            state = dill.load(fh)
        vec = None if state["index"] is None else Bm25Device(state["index"], device=device)
        return cls(vectorizer=vec, docs=state["docs"], k=state["k"], preprocess_func=state["preprocess_func"],
                   bm25_params=state["bm25_params"], device=device, warn_default_preprocess=False)
