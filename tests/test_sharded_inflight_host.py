"""The sharded store's pipelined search maps a batch's local rows to global ids with the id map of its LAUNCH: a
remove_rows() between search_async() and host() renumbers the rows that later searches see, not the answer in flight.
The store's batch path (HipFlatVectorStore._search_chunks) yields between chunks, so a caller can delete documents while
the next chunk is in flight.  No GPU: the local engine is a numpy double that answers at launch, as a correctly ordered
device scan does."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from rag_arc_amd.encapsulation.database.vector_db.hip_sharded import _ShardedIndex
from tests.helpers import OracleIndex


class _Answered:
    def __init__(self, ids, scores):
        self.ids, self.scores = ids, scores

    def result(self):
        return self.ids, self.scores


class _AsyncOracleIndex(OracleIndex):
    """OracleIndex plus the pipelined surface _ShardedIndex uses: search_async() answers on the rows of its launch."""

    def search_async(self, queries, k, to_host=False):
        scores, ids = self.search(queries, k)
        return _Answered(torch.from_numpy(ids.copy()), torch.from_numpy(scores.copy()))

    def remove_rows(self, rows):
        holes = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
        self._rows = np.delete(self._rows, holes, axis=0)
        self.ntotal = self._rows.shape[0]
        return int(holes.size)


def _launch_map(blocks):
    return np.concatenate([np.arange(g0, g0 + n, dtype=np.int64) for g0, n in blocks])


@pytest.mark.parametrize("holes", [[6, 7, 8], [1, 2, 13, 20], [0, 11, 18, 25]],
                         ids=["other_rank_rows", "own_and_other_rows", "block_ends"])
def test_pending_shard_maps_with_the_launch_time_blocks(holes):
    d, k = 16, 10
    rng = np.random.default_rng(3)
    A, Bv = rng.standard_normal((6, d)).astype(np.float32), rng.standard_normal((7, d)).astype(np.float32)
    Q = rng.standard_normal((5, d)).astype(np.float32)
    sh = _ShardedIndex(_AsyncOracleIndex(d))
    # this engine holds the first half of every add, as rank 0 of a two-rank store does: the id map has gaps
    sh.add_block(A, 0, 12)
    sh.add_block(Bv, 12, 14)
    assert sh.ntotal == 26 and sh.local.ntotal == 13
    rows_then, map_then = sh.local.rows.copy(), _launch_map(sh._blocks)
    want_i, want_s, _ = cpu_ref.flat_search_f16(rows_then, cpu_ref.normalize_L2(Q), k)

    h = sh.search_async(Q, k)
    sh.remove_rows(holes)
    assert sh.ntotal == 26 - len(holes)
    scores, ids = h.host()
    assert np.array_equal(ids, map_then[want_i]), (holes, ids, map_then[want_i])
    assert np.array_equal(scores.view(np.uint32), want_s.view(np.uint32))

    # a search launched after the removal maps with the new blocks
    map_now = _launch_map(sh._blocks)
    assert map_now.size == sh.local.ntotal
    now_i, now_s, _ = cpu_ref.flat_search_f16(sh.local.rows, cpu_ref.normalize_L2(Q), k)
    scores, ids = sh.search_async(Q, k).host()
    assert np.array_equal(ids, map_now[now_i]) and np.array_equal(scores.view(np.uint32), now_s.view(np.uint32))
