"""The arithmetic steps of the reference's graph store that sit on the dense hot path's kernels: entity de-duplication by
all-pairs cosine (encapsulation/database/graph_db/Base_Neo4j.py:538-583) and the Louvain communities of those pairs (:646-658),
event disambiguation by a k-nearest-neighbour graph (event_graphrag_neo4j.py:600-672), and retrieval from the graph those
build: personalized PageRank from the entities a query links to, pushed through the (chunk)-[:MENTIONS]->(entity) links
(event_graphrag_neo4j.py:508-536) onto the chunks a retriever returns, and the traversal a local search asks the server for,
MATCH (s)-[*..h]-(v): the entities within h hops of a query's entities, and MATCH p = allShortestPaths((a)-[*..L]-(b)): how
two of them are connected (neighbourhood.py); and the last step of the
de-duplication, merging each cluster into one entity (Base_Neo4j.py:714-890), which contracts that graph where it lies
(merge.py); and what gds.wcc answers about that graph, its connected components (components.py).  The graph database itself is
out of scope.  Where nobody extracted relations, the graph itself is the co-occurrence projection of the mention links
(cooccurrence.py).  What the reference's
store_graph does per batch of documents — MERGE new mentions, entities and relations into what is there — is ingest.py: graphs and
mention maps built from raw rows and extended on the device."""
from .communities import entity_clusters, louvain_communities
from .components import Components, connected_components
from .cooccurrence import Cooccurrence, cooccurrence_graph, cooccurrence_pairs
from . import ingest
from .merge import MergedEntities, MergePlan, deduplicate_entities, merge_entities, merge_plan
from .neighbourhood import RelationList, k_hop, k_hop_subgraph
from .neighbourhood import all_shortest_paths as shortest_paths
from .pagerank import EntityGraph, personalized_pagerank
from .passages import MentionMap
from .similarity import knn_graph, similar_pairs

__all__ = ["similar_pairs", "knn_graph", "louvain_communities", "entity_clusters", "EntityGraph", "personalized_pagerank", "MentionMap",
           "k_hop", "k_hop_subgraph", "shortest_paths", "RelationList", "merge_plan", "merge_entities", "deduplicate_entities", "MergePlan",
           "MergedEntities", "connected_components", "Components", "cooccurrence_pairs",
           "cooccurrence_graph", "Cooccurrence", "ingest"]
