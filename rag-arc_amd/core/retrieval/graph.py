"""Graph retriever on the MI355X: the third arm of hybrid retrieval beside the dense and the lexical one.

A query is embedded, linked to the entities nearest to it (a `FlatIndexF16` over the entity embeddings, row i = vertex i),
personalized PageRank spreads from those seeds over the entity graph, and the mass of the entities is pushed through the
(chunk)-[:MENTIONS]->(entity) links onto the chunks — the way HippoRAG's and upstream RAG-ARC's graph retrievers end.  The
search, the PageRank, the projection and the top-k all run in librarc_hip.so without leaving HBM
(`EntityGraph.retrieve_chunks`); what comes back to the host is k (chunk, score) pairs per query.

Each returned Document is a copy of the stored chunk with a `score` attribute (the exact fixed-point score S / 2^28), which is
what `MultiPathRetriever` reads with getattr(d, "score", 1.0).  No CPU fallback: without a device the constructor raises.

`expansion="k_hop"` replaces the PageRank by a traversal: the chunks are ranked by their mentions of the entities within `hops`
edges of the seeds, a mention one hop nearer counting `decay` times as much (`EntityGraph.expand_chunks`) — the
expansion a Neo4j-backed local search writes MATCH (s)-[*..h]-(v).  The default, "ppr", is what it was.  With
`relation_types=` (a graph built with `pair_types=`) the traversal crosses only the relation types a query allows,
MATCH (s)-[:CAUSAL|SEQUENTIAL*..h]-(v), still one launch for a batch of mixed filters."""
import dataclasses
import uuid
from typing import Any, Dict, Iterable, List, Optional

import numpy as np

from ..utils.data_model import Document
from .base import BaseRetriever


class HipGraphRetriever(BaseRetriever):
    def __init__(self, embedding, index, graph, mentions, docs: List[Document], k: int = 5, seeds_per_query: int = 5,
                 damping: float = 0.85, max_iterations: int = 20, tolerance: float = 0.0, expansion: str = "ppr", hops: int = 2,
                 decay=None, relation_types=None, **kwargs):
        super().__init__(**kwargs)
        self._validate_k(k)
        if expansion not in ("ppr", "k_hop"):
            raise ValueError(f"expansion must be 'ppr' or 'k_hop', got {expansion!r}")
        self._check_relation_types(expansion, graph, relation_types)
        docs = list(docs)
        if int(index.ntotal) != graph.n:
            raise ValueError(f"the index holds {int(index.ntotal)} rows and the graph {graph.n} vertices: row i must be vertex i")
        if mentions.n_entities != graph.n:
            raise ValueError(f"the mention map is over {mentions.n_entities} entities and the graph has {graph.n} vertices")
        if mentions.n_chunks != len(docs):
            raise ValueError(f"the mention map is over {mentions.n_chunks} chunks and {len(docs)} documents were given: chunk i must be "
                             f"document i")
        graph._check_run(damping, max_iterations, tolerance, None, graph.n)      # the refusals of retrieve_chunks, up front
        graph._check_index(index, seeds_per_query)
        self.embedding, self.index, self.graph, self.mentions, self.docs = embedding, index, graph, mentions, docs
        self.k = k
        self.seeds_per_query, self.damping = int(seeds_per_query), float(damping)
        self.max_iterations, self.tolerance = int(max_iterations), float(tolerance)
        self.expansion, self.hops, self.decay = expansion, int(hops), None
        self.relation_types = relation_types
        self._cooccurrence = None                                                # from_arrays(pairs=None): the projection's arguments
        if expansion == "k_hop":                                                 # the refusals of expand_chunks, up front
            from ...encapsulation.database.graph_db.neighbourhood import check_decay, check_hops

            self.hops = check_hops(hops)
            self.decay = check_decay(decay, self.hops)

    @staticmethod
    def _check_relation_types(expansion, graph, relation_types, nq=None) -> None:
        """the refusals of a typed expand_chunks, before anything is embedded; nq: the queries the filters must fit"""
        if relation_types is None:
            return
        if expansion != "k_hop":
            raise ValueError("relation_types with expansion='ppr': typed personalized PageRank is not built into the retriever: its 'ppr' expansion "
                             "does not take filters yet; use expansion='k_hop', or call EntityGraph.retrieve_chunks(..., relation_types=) "
                             "on the retriever's graph")
        from ...encapsulation.database.graph_db.neighbourhood import check_typed, spread_filters

        filters = check_typed(graph, relation_types)
        if nq:
            spread_filters(filters, nq)

    @staticmethod
    def _validate_k(k) -> None:
        if isinstance(k, bool) or not isinstance(k, int) or k <= 0:
            raise ValueError(f"k must be > 0, got {k!r}")

    @classmethod
    def from_arrays(cls, embedding, entity_embeddings, pairs=None, mentions=None, texts: Iterable[str] = (), pair_weights=None,
                    mention_weights=None, ids: Optional[Iterable[str]] = None, metadatas: Optional[Iterable[Dict[str, Any]]] = None,
                    metric: str = "cosine", device: int = 0, cooccurrence_weight: str = "count", min_weight: int = 1, max_mentions: int = 64,
                    pair_types=None, **kwargs: Any) -> "HipGraphRetriever":
        """entity_embeddings: float32 [n][d], row i = vertex i; pairs / pair_weights: the entity graph's edges (EntityGraph);
        mentions / mention_weights: (chunk, entity) links (MentionMap); texts (and ids, metadatas): the chunks, chunk i = text i.
        pairs=None: the graph is the co-occurrence projection of the mention map (MentionMap.cooccurrence) —
        cooccurrence_weight "count" or "product", min_weight and max_mentions as it takes them; with pairs the three are ignored.
        pair_types: one relation type per pair, an integer in [0, 32) (EntityGraph(types=)): what relation_types= filters on."""
        from ...encapsulation.database.graph_db import EntityGraph, MentionMap
        from ...hip.engine import FlatIndexF16

        texts = [str(t) for t in texts]
        if not texts:
            raise ValueError("texts must not be empty")
        if mentions is None:
            raise ValueError("mentions must be given: the (chunk, entity) links")
        metadatas = list(metadatas) if metadatas is not None else [{} for _ in texts]
        ids = [str(i) for i in ids] if ids is not None else [str(uuid.uuid4()) for _ in texts]
        if len(metadatas) != len(texts) or len(ids) != len(texts):
            raise ValueError(f"{len(texts)} texts, {len(metadatas)} metadatas, {len(ids)} ids")
        cls._validate_k(kwargs.get("k", 5))
        x = np.ascontiguousarray(entity_embeddings, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] < 2:
            raise ValueError(f"expected [n][d] entity embeddings with n >= 2, got an array of shape {x.shape}")
        n = int(x.shape[0])
        if pairs is None:                                                           # (refusals first: the graph and the map
            from ...encapsulation.database.graph_db.cooccurrence import check_arguments

            if pair_weights is not None:
                raise ValueError("pair_weights without pairs: the weights of a co-occurrence graph come from the mentions")
            if pair_types is not None:
                raise ValueError("pair_types without pairs: a co-occurrence graph has no relation types")
            check_arguments(n, cooccurrence_weight, min_weight, max_mentions)
            mention_map = MentionMap(len(texts), n, mentions, weights=mention_weights, device=device)   # check before anything is stored)
            graph = mention_map.cooccurrence(weight=cooccurrence_weight, min_weight=min_weight, max_mentions=max_mentions)
        else:
            graph = EntityGraph(n, pairs, weights=pair_weights, types=pair_types, device=device)
            mention_map = MentionMap(len(texts), n, mentions, weights=mention_weights, device=device)
        index = FlatIndexF16(int(x.shape[1]), metric=metric, device=device)
        index.add(x)
        docs = [Document(content=t, metadata=m, id=i) for t, m, i in zip(texts, metadatas, ids)]
        self = cls(embedding, index, graph, mention_map, docs, **kwargs)
        if pairs is None:                                                           # add_documents rebuilds the projection with these
            self._cooccurrence = {"weight": cooccurrence_weight, "min_weight": min_weight, "max_mentions": max_mentions}
        return self

    # -- growth -----------------------------------------------------------------------------------------------------------
    def add_documents(self, texts: Iterable[str], mentions, mention_weights=None, entity_embeddings=None, pairs=None, pair_weights=None,
                      pair_types=None, ids: Optional[Iterable[str]] = None, metadatas: Optional[Iterable[Dict[str, Any]]] = None) -> List[str]:
        """One more batch of documents, the way the reference's store_graph(documents) is called per batch.
        texts (and ids, metadatas): the new chunks, numbered from len(self.docs); mentions / mention_weights: (chunk, entity)
        links naming chunks by those ABSOLUTE numbers (a link from an old chunk to a new entity is allowed);
        entity_embeddings: float32 [k][d] rows appended to the index, which become vertices graph.n .. graph.n + k - 1;
        pairs / pair_weights / pair_types: relations that extend the graph (EntityGraph.extended).  A retriever built with
        pairs=None rebuilds its co-occurrence projection from the extended map, with the arguments it was built with, and refuses
        pairs= here.  The graph and the map are extended on the device (graph_db/ingest.py) into NEW objects; every check runs
        before anything is changed, and the index, self.graph, self.mentions and self.docs are replaced together at the end: a
        call that raises leaves the retriever answering as before.  -> the ids of the new documents."""
        texts = [str(t) for t in texts]
        if not texts:
            raise ValueError("texts must not be empty")
        if mentions is None:
            raise ValueError("mentions must be given: the (chunk, entity) links of the new chunks")
        metadatas = list(metadatas) if metadatas is not None else [{} for _ in texts]
        ids = [str(i) for i in ids] if ids is not None else [str(uuid.uuid4()) for _ in texts]
        if len(metadatas) != len(texts) or len(ids) != len(texts):
            raise ValueError(f"{len(texts)} texts, {len(metadatas)} metadatas, {len(ids)} ids")
        x = None
        if entity_embeddings is not None:
            x = np.ascontiguousarray(entity_embeddings, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != self.index.dim:
                raise ValueError(f"expected [k][{self.index.dim}] entity embeddings, got an array of shape {x.shape}")
            if x.shape[0] == 0:
                x = None
        n = self.graph.n + (0 if x is None else int(x.shape[0]))
        if self._cooccurrence is not None and (pairs is not None or pair_weights is not None or pair_types is not None):
            raise ValueError("pairs with a co-occurrence graph: this retriever was built with pairs=None, its graph is the projection of "
                             "the mention map and is rebuilt from the extended map")
        if pairs is None and (pair_weights is not None or pair_types is not None):
            raise ValueError("pair_weights or pair_types without pairs")
        new_mentions = self.mentions.extended(mentions, weights=mention_weights, n_chunks=len(self.docs) + len(texts), n_entities=n)
        if self._cooccurrence is not None:
            from ...encapsulation.database.graph_db.cooccurrence import check_arguments

            check_arguments(n, self._cooccurrence["weight"], self._cooccurrence["min_weight"], self._cooccurrence["max_mentions"])
            new_graph = new_mentions.cooccurrence(**self._cooccurrence)
        elif pairs is not None or n != self.graph.n:
            rows = np.zeros((0, 2), np.int64) if pairs is None else pairs
            types = pair_types if pairs is not None else (np.zeros(0, np.int64) if self.graph.typed else None)
            new_graph = self.graph.extended(rows, weights=pair_weights, types=types, n=n)
        else:
            new_graph = self.graph
        self._check_relation_types(self.expansion, new_graph, self.relation_types)
        if x is not None:
            self.index.add(x)
        docs = self.docs + [Document(content=t, metadata=m, id=i) for t, m, i in zip(texts, metadatas, ids)]
        self.graph, self.mentions, self.docs = new_graph, new_mentions, docs
        return ids

    # -- queries ----------------------------------------------------------------------------------------------------------
    def _embed(self, texts: List[str]):
        """one embedding batch: on the device where the provider can, else one host array"""
        emb = self.embedding
        for name in ("embed_queries_device", "embed_queries"):
            batched = getattr(emb, name, None)
            if batched is not None:
                return batched(texts)
        return np.asarray([emb.embed_query(t) for t in texts], dtype=np.float32)

    def _get_relevant_documents(self, query: str, **kwargs: Any) -> List[Document]:
        return self.batch_invoke([query], **kwargs)[0]

    def batch_invoke(self, inputs: List[str], **kwargs: Any) -> List[List[Document]]:
        """invoke() for a list of queries: one embedding batch, one search and one PageRank run (or one traversal, with
        expansion="k_hop") per 256 queries.  Element i equals invoke(inputs[i], **kwargs) — every query is ranked on its own,
        by integer arithmetic.  relation_types= overrides the constructor's: one filter for all inputs or one per input."""
        inputs = list(inputs)
        k = kwargs.get("k", self.k)
        self._validate_k(k)
        relation_types = kwargs.get("relation_types", self.relation_types)
        self._check_relation_types(self.expansion, self.graph, relation_types, len(inputs))
        if not inputs:
            return []
        if self.expansion == "k_hop":
            ids, scores, counts = self.graph.expand_chunks(self.index, self._embed(inputs), self.mentions, seeds_per_query=self.seeds_per_query,
                                                           hops=self.hops, decay=self.decay, top_k=min(k, len(self.docs)),
                                                           relation_types=relation_types)
        else:
            ids, scores, counts = self.graph.retrieve_chunks(self.index, self._embed(inputs), self.mentions,
                                                             seeds_per_query=self.seeds_per_query, top_k=min(k, len(self.docs)),
                                                             damping=self.damping, max_iterations=self.max_iterations,
                                                             tolerance=self.tolerance)
        out: List[List[Document]] = []
        for q in range(len(inputs)):
            answer = []
            for c, s in zip(ids[q, :counts[q]].tolist(), scores[q, :counts[q]].tolist()):
                doc = dataclasses.replace(self.docs[c])
                doc.score = s
                answer.append(doc)
            out.append(answer)
        return out

    # -- information --------------------------------------------------------------------------------------------------------
    def update_k(self, new_k: int) -> None:
        self._validate_k(new_k)
        self.k = new_k

    def get_document_count(self) -> int:
        return len(self.docs)

    def get_name(self) -> str:
        return "HipGraphRetriever"

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(entities={self.graph.n}, edges={self.graph.m}, chunks={len(self.docs)}, "
                f"mentions={self.mentions.nnz}, k={self.k}, seeds_per_query={self.seeds_per_query})")
