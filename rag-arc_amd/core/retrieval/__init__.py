from .base import BaseRetriever  # noqa: F401
from .bm25 import HipBM25Retriever  # noqa: F401
from .dense import VectorStoreRetriever  # noqa: F401
from .graph import HipGraphRetriever  # noqa: F401
from .multipath import MultiPathRetriever  # noqa: F401
