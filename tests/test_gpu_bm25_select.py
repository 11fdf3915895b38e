"""rarc_bm25_topk / rarc_bm25_scores on planted indexes (tests/bm25_plant.py): the three exits of bm_select, merge rounds of
every depth, placeholder slots of a short last tile, the key map at the ends of the double range, the summation order and
long posting runs.  Everything is bit-exact against a sequential float64 sum and a full stable sort.  What each case is, is
proven without a GPU in tests/test_bm25_plant_host.py."""
import functools

import numpy as np
import pytest

from rag_arc_amd.hip.bm25 import Bm25Device
from tests import bm25_plant as P

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def device(name):
    """The case's index on the GPU; only the latest is kept, so earlier corpora are released as the file moves on."""
    return Bm25Device(P.case(name).index())


def check_answer(c, q, k, ids, scores, what):
    want = c.order(q, k)
    assert ids.shape == (k,) and scores.shape == (k,), (what, q, k)
    assert ids.max() < c.n_docs and ids.min() >= 0, (what, q, k, ids.max())
    bad = np.flatnonzero(ids != want)
    assert bad.size == 0, (what, q, k, f"{bad.size} ids differ, first at rank {bad[0]}", ids[bad[:5]], want[bad[:5]])
    bad = np.flatnonzero(P.bits(scores) != P.bits(c.scores(q)[want]))
    assert bad.size == 0, (what, q, k, f"{bad.size} scores differ", scores[bad[:5]], c.scores(q)[want][bad[:5]])


@pytest.mark.parametrize("name,k", P.CASE_KS, ids=[f"{n}-k{k}" for n, k in P.CASE_KS])
def test_topk(name, k):
    """ids in the reference order, scores the reference's 64 bits, no id past the corpus; one batch call over all the
    case's queries (the empty one included) equals the one-at-a-time calls."""
    c, dev = P.case(name), device(name)
    batch_i, batch_s = dev.topk(c.queries, k)
    assert batch_i.shape == batch_s.shape == (len(c.queries), k)
    for q, terms in enumerate(c.queries):
        one_i, one_s = dev.topk([terms], k)
        check_answer(c, q, k, one_i[0], one_s[0], "alone")
        check_answer(c, q, k, batch_i[q], batch_s[q], "batch")


@pytest.mark.parametrize("name", list(P.BUILDERS))
def test_dense_scores(name):
    """Bm25Device.scores: the planted vector (the sequential sum, for queries of several tokens) bit for bit, alone and
    in one batch."""
    c, dev = P.case(name), device(name)
    batch = dev.scores(c.queries)
    assert batch.shape == (len(c.queries), c.n_docs)
    for q, terms in enumerate(c.queries):
        want = c.scores(q)
        if len(terms) == 1 and c.idf[terms[0]] == 1.0:
            want = c.vectors[terms[0]]
        for what, got in (("batch", batch[q]), ("alone", dev.scores([terms])[0])):
            bad = np.flatnonzero(P.bits(got) != P.bits(want))
            assert bad.size == 0, (what, q, f"{bad.size} scores differ, first at document {bad[0]}", got[bad[:5]],
                                   want[bad[:5]])
