"""The two self-joins (csrc/pairs.hip, csrc/knn.hip) on columns with LONG nomination lists and a decided answer, against the
float64 oracle of tests/knn_ref.py.  tests/test_knn_ref_host.py proves on the CPU what each input promises: how long the lists
must be, and that no tolerance band excuses anything — so the comparisons here are plain equality of sets and of ids in order.

  similar_pairs  columns with more than 1024 nominees: the second trip of pairs_finalize_kernel's block loop
  knn_graph      one tight cluster of 1100 rows (several rounds of knn_finalize_kernel's 1024-entry buffer) and of 4300 rows
                 (five or six rounds; knn_tighten_kernel's radix select reads its keys from global memory past 4096 entries)

Where a list length has to be shown the C entries are called directly: a cand_cap below the length must raise flag bit 0."""
import ctypes

import numpy as np
import pytest

from tests import knn_ref as R
from tests.test_gpu_similar_pairs import _same

pytestmark = pytest.mark.gpu


def _pad256(n):
    return (n + 255) // 256 * 256


def _direct_pairs(x, threshold, cand_cap, out_cap):
    """rarc_similar_pairs once, no regrow loop: (pairs [min(found, out_cap)][2], cosines, found, flags)."""
    import torch

    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n, d = t.shape
    ws = torch.empty(int(lib.rarc_similar_pairs_workspace_bytes(n, d, cand_cap)), dtype=torch.uint8, device="cuda")
    pairs = torch.full((out_cap + 64, 2), -7, dtype=torch.int64, device="cuda")
    cos = torch.full((out_cap + 64,), -7.0, dtype=torch.float64, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    B.check(lib.rarc_similar_pairs(t.data_ptr(), t.stride(0), n, d, ctypes.c_double(threshold), ws.data_ptr(), ws.numel(), cand_cap,
                                   pairs.data_ptr(), cos.data_ptr(), out_cap, count.data_ptr(), flags.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "rarc_similar_pairs")
    torch.cuda.synchronize()
    found = int(count.item())
    assert torch.all(pairs[out_cap:] == -7) and torch.all(cos[out_cap:] == -7.0)      # nothing past out_cap was written
    return pairs[:min(found, out_cap)].cpu().numpy(), cos[:min(found, out_cap)].cpu().numpy(), found, int(flags.item())


def _direct_knn(x, top_k, cutoff, cand_cap):
    """rarc_knn_graph once, no regrow loop: ((ids, cosines, counts), flags)."""
    import torch

    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n, d = t.shape
    ws = torch.empty(int(lib.rarc_knn_graph_workspace_bytes(n, d, top_k, cand_cap)), dtype=torch.uint8, device="cuda")
    ids = torch.full((n, top_k), -7, dtype=torch.int64, device="cuda")
    cos = torch.full((n, top_k), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    B.check(lib.rarc_knn_graph(t.data_ptr(), t.stride(0), n, d, top_k, ctypes.c_double(cutoff), ws.data_ptr(), ws.numel(), cand_cap,
                               ids.data_ptr(), cos.data_ptr(), cnt.data_ptr(), flags.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "rarc_knn_graph")
    torch.cuda.synchronize()
    return (ids.cpu().numpy(), cos.cpu().numpy(), cnt.cpu().numpy()), int(flags.item())


def _knn(x, top_k, cutoff):
    from rag_arc_amd.encapsulation.database.graph_db import knn_graph

    return knn_graph(x, top_k=top_k, similarity_cutoff=cutoff, as_arrays=True)


# ---- A. similar_pairs: columns with more than 1024 nominees, exact set --------------------------------------------------------

@pytest.fixture(scope="module")
def long_pairs():
    x = R.long_pair_lists()
    pairs, cos = R.pairs_from_sim(R.cosine_matrix_f64(x), R.LONG_PAIRS_THR)
    return x, pairs, cos


def _assert_pair_set(got_pairs, got_cos, want_pairs, want_cos, n, what):
    """Both ordered by (i, j): the same pairs, none twice, per column the same number, scores within 1e-12 — and the existing
    file's _same on the columns past one block (as python objects the whole answer, 1.8 M triples, would take it ten seconds;
    the array comparison above it is the stricter one: no pair may differ, not even at the threshold)."""
    key, want_key = got_pairs[:, 0] * n + got_pairs[:, 1], want_pairs[:, 0] * n + want_pairs[:, 1]
    assert np.all(key[1:] > key[:-1]), (what, "a pair appears twice, or the order is not (i, j)")
    got_cols, want_cols = np.bincount(got_pairs[:, 1], minlength=n), np.bincount(want_pairs[:, 1], minlength=n)
    bad = np.nonzero(got_cols != want_cols)[0]
    assert bad.size == 0, (what, "pairs per column differ", bad[:8], got_cols[bad[:8]], want_cols[bad[:8]])
    assert np.array_equal(key, want_key), (what, "pair sets differ")
    assert np.max(np.abs(got_cos - want_cos)) <= 1e-12, (what, "scores")
    long_cols = np.nonzero(want_cols > R.LONG_PAIRS_OVER)[0]
    assert len(long_cols) == 256
    g, w = np.isin(got_pairs[:, 1], long_cols[::8]), np.isin(want_pairs[:, 1], long_cols[::8])
    _same(list(zip(got_pairs[g, 0].tolist(), got_pairs[g, 1].tolist(), got_cos[g].tolist())),
          list(zip(want_pairs[w, 0].tolist(), want_pairs[w, 1].tolist(), want_cos[w].tolist())), R.LONG_PAIRS_THR, what)


def test_pairs_of_columns_past_one_block_are_the_oracles_set(long_pairs):
    """256 columns hold more than 1024 + 64 true pairs each (and more nominees): pairs_finalize_kernel takes its block loop's
    second trip — s_keep reset, s_base taken again — on every one of them.  A pair dropped or written twice there changes the
    set, the count per column and the total."""
    from rag_arc_amd.encapsulation.database.graph_db import similar_pairs

    x, want_pairs, want_cos = long_pairs
    n = len(x)
    got_pairs, got_cos = similar_pairs(x, R.LONG_PAIRS_THR, as_arrays=True)
    assert len(got_pairs) == len(want_pairs)
    _assert_pair_set(got_pairs, got_cos, want_pairs, want_cos, n, "long lists")


def test_pairs_entry_counts_all_and_flags_a_small_output_and_a_short_list(long_pairs):
    """rarc_similar_pairs itself.  Lists that hold every row, room for every pair: no flag, out_count = the set's size, the set.
    Room for fewer: flag bit 1, out_count still counts every pair, what was written are distinct pairs of the set.  Lists of
    1024: flag bit 0 — some column nominated more than 1024 rows, which is how it is known the long trips ran above."""
    x, want_pairs, want_cos = long_pairs
    n, total = len(x), len(want_pairs)
    want_key = want_pairs[:, 0] * n + want_pairs[:, 1]
    pairs, cos, found, flags = _direct_pairs(x, R.LONG_PAIRS_THR, _pad256(n), total)
    assert flags == 0 and found == total
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    _assert_pair_set(pairs[order], cos[order], want_pairs, want_cos, n, "direct")
    small = total // 3
    pairs, cos, found, flags = _direct_pairs(x, R.LONG_PAIRS_THR, _pad256(n), small)
    assert flags == 2 and found == total and len(pairs) == small
    key = pairs[:, 0] * n + pairs[:, 1]
    at = np.searchsorted(want_key, key)
    assert len(np.unique(key)) == small and np.all(at < total) and np.array_equal(want_key[np.minimum(at, total - 1)], key)
    assert np.max(np.abs(cos - want_cos[at])) <= 1e-12
    _, _, found, flags = _direct_pairs(x, R.LONG_PAIRS_THR, 1024, total)
    assert flags & 1 and found < total                                                # (the hidden nominations are missing pairs)


def test_pairs_of_long_columns_in_the_second_super_block(long_pairs):
    """The same rows behind 4097 zero rows (which pair with nothing): the long columns are columns 1 ... of the super-block at
    col0 = 4096, their nominees rows 4097 and up.  The answer is the first case's, shifted."""
    from rag_arc_amd.encapsulation.database.graph_db import similar_pairs

    x, want_pairs, want_cos = long_pairs
    lead = 4097
    got_pairs, got_cos = similar_pairs(R.long_pair_lists(lead=lead), R.LONG_PAIRS_THR, as_arrays=True)
    assert len(got_pairs) == len(want_pairs) and got_pairs.min() >= lead
    _assert_pair_set(got_pairs - lead, got_cos, want_pairs, want_cos, len(x), "second super-block")


# ---- B. knn_graph: one tight cluster larger than the finalize's buffer and than the tighten's LDS select ---------------------------

def _tight_input(which):
    seed, m = which
    x, at, marks = R.tight_cluster(seed, m, probe=R.TIGHT_PROBE if which == R.TIGHT_LARGE else 0.0)
    sim = R.cosine_matrix_f64(x)
    return x, at, marks, sim, R.tight_cutoffs(sim, at)


@pytest.fixture(scope="module")
def tight_small():
    return _tight_input(R.TIGHT_SMALL)


@pytest.fixture(scope="module")
def tight_large():
    return _tight_input(R.TIGHT_LARGE)


def _bit_equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[2], b[2])


def _assert_symmetric_bits(ids, cos, n):
    """cos[i -> j] and cos[j -> i] are the same bits wherever both edges appear."""
    i, t = np.nonzero(ids >= 0)
    j = ids[i, t]
    key, back = i * n + j, j * n + i
    order = np.argsort(key)
    at = np.minimum(np.searchsorted(key[order], back), len(key) - 1)
    both = key[order][at] == back
    assert both.any()
    bits = cos[i, t].view(np.uint64)
    assert np.array_equal(bits[both], bits[order][at][both])


def _tight_case(inp, short_cap, top_k, which_cutoff):
    x, at, marks, sim, cutoffs = inp
    n, cutoff = len(x), cutoffs[which_cutoff]
    want = R.knn_from_sim(sim, top_k, cutoff)
    got_short, flags = _direct_knn(x, top_k, cutoff, short_cap)
    if which_cutoff < 2:        # (proven on the CPU for these two; under the median cutoff the lists are as long in practice only)
        assert flags & 1, "no list passed %d entries: the long path did not run" % short_cap
    got, flags = _direct_knn(x, top_k, cutoff, _pad256(n))
    assert flags == 0
    R.assert_equal_in_order(got, want, (len(at), top_k, cutoff))
    assert _bit_equal(_knn(x, top_k, cutoff), got), "the wrapper's answer differs from the direct call's"
    ids, cos, cnt = got
    in_cluster = np.zeros(n, bool)
    in_cluster[at] = True
    assert in_cluster[ids[at][ids[at] >= 0]].all()                                   # a cluster row's neighbours lie in the cluster
    _assert_symmetric_bits(ids, cos, n)
    if which_cutoff == 0:
        assert np.all(cnt == top_k)
    elif which_cutoff == 1:
        assert np.all(cnt[at] == top_k)
    return got


@pytest.mark.parametrize("which_cutoff", [0, 1, 2], ids=["none", "0.85", "median"])
@pytest.mark.parametrize("top_k", R.TIGHT_TOP_KS[R.TIGHT_SMALL])
def test_cluster_of_1100_takes_several_finalize_rounds(tight_small, top_k, which_cutoff):
    """Every cluster column's list holds the 1100 cluster rows: with cand_cap 1024 flag bit 0 is raised, with room for all the
    finalize takes two rounds (the second refills what the running answer of top_k leaves of the buffer).  The best neighbours arrive in every round;
    a lost prefix, a skipped round or a wrong refill changes ids that the oracle decides."""
    _tight_case(tight_small, 1024, top_k, which_cutoff)


@pytest.mark.parametrize("which_cutoff", [0, 1, 2], ids=["none", "0.85", "median"])
@pytest.mark.parametrize("top_k", [10, 256])
def test_cluster_of_4300_selects_from_global_memory_and_takes_five_rounds(tight_large, top_k, which_cutoff):
    """Lists of 4300: with cand_cap 4096 flag bit 0 is raised; with room for all, the last tighten of every cluster column selects
    a_K among more than 4096 keys read from global memory and compacts 17 tiles in place, and the finalize takes five rounds (six with a running answer of 256)."""
    _tight_case(tight_large, 4096, top_k, which_cutoff)


def test_probe_column_keeps_its_own_row_out_of_the_global_select(tight_large):
    """top_k = 1: a_K is the best score among the OTHERS.  The probe row's best neighbour has cosine ~0.996 and nearly the whole
    cluster lies within 2 eps under it (a list past 4096 entries at the last tighten), while the row's own score is 1: counted
    into the select it would put the threshold at 1 - 2 eps, above every other row, and the column would come back empty."""
    x, at, marks, sim, cutoffs = tight_large
    got = _tight_case(tight_large, 4096, 1, 0)
    p = marks["probe"]
    assert got[2][p] == 1 and got[0][p, 0] == np.argmax(np.where(np.arange(len(x)) == p, -np.inf, sim[p]))


# ---- C. small companions --------------------------------------------------------------------------------------------------------

def test_identical_copies_past_one_buffer_keep_the_lowest_indices():
    """1300 bit-identical rows among 1500, top_k 64: every copy's list holds the 1299 others at one score — two finalize rounds,
    and only the sort's index tie-break orders entries across them: the 64 lowest other copies, ascending, the same bits."""
    x, at = R.many_identical_copies()
    got = _knn(x, 64, -1.0)
    R.compare(got, R.cosine_matrix_f64(x), 64, -1.0, what="1300 identical copies")
    ids, cos, cnt = got
    for a in at:
        assert np.array_equal(ids[a], at[at != a][:64]), a
    assert np.all(cnt == 64) and len(set(cos[at].view(np.uint64).ravel().tolist())) == 1 and abs(cos[at[0], 0] - 1.0) <= 1e-12
    got_direct, flags = _direct_knn(x, 64, -1.0, _pad256(len(x)))
    assert flags == 0 and _bit_equal(got, got_direct)
    assert _direct_knn(x, 64, -1.0, 1024)[1] & 1                                      # ... and the lists were longer than one buffer


def test_thinned_columns_beside_the_long_ones():
    """The 1100-row cluster at cutoff 0.85 with a zeroed row (an empty list: the finalize's one round takes nothing in), a
    group of five near-duplicates (four survivors each: fewer than top_k) and background rows with no neighbour above the
    cutoff (count 0, padding (-1, -inf)) in the same launches as the columns that take several rounds."""
    seed, m = R.TIGHT_SMALL
    x, at, marks = R.tight_cluster(seed, m, zero_rows=1, group=4)
    sim = R.cosine_matrix_f64(x)
    want = R.knn_from_sim(sim, 10, 0.85)
    got = _knn(x, 10, 0.85)
    R.assert_equal_in_order(got, want, "thinned")
    R.compare(got, sim, 10, 0.85, what="thinned")
    ids, cos, cnt = got
    z, grp = marks["zeroed"], marks["group"]
    assert np.all(cnt[z] == 0) and not np.isin(ids, z).any()
    assert np.all(cnt[grp] == 4) and all(set(ids[g, :4]) == set(grp) - {g} for g in grp)
    assert np.all(ids[grp, 4:] == -1) and np.all(np.isneginf(cos[grp, 4:]))
    empty = cnt == 0
    assert empty.sum() > 600 and np.all(ids[empty] == -1) and np.all(np.isneginf(cos[empty]))
    assert np.all(cnt[at] == 10)
