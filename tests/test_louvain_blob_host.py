"""tests/louvain_blob.py restates the layouts of the GRAPH and the STATE blob; their totals must be the library's own
(rarc_graph_csr_workspace_bytes, rarc_louvain_workspace_bytes: host code, no device needed), or the GPU tests that read the blobs
where they lie would read the wrong bytes."""
import pytest

from rag_arc_amd.hip import binding as B
from tests import louvain_blob as LB

NS = [2, 3, 63, 64, 65, 2048, 2049, 8192, 8193, 8194, 524_289]


def _ms(n):
    """m below, at and above n - 1, on both sides of the DEG_LDS edge of the global tables, and large enough for the pair table
    to outgrow them"""
    out = {1, 2, max(1, n - 2), n - 1, n, 3 * n, LB.DEG_LDS - 1, LB.DEG_LDS, LB.DEG_LDS + 1, 100_000, 3_000_000}
    return sorted(m for m in out if m >= 1)


@pytest.mark.parametrize("n", NS)
def test_totals_equal_the_library_s(n):
    lib = B.load_library()
    for m in _ms(n):
        assert LB.graph_bytes(n, m) == lib.rarc_graph_csr_workspace_bytes(n, m), (n, m)
        assert LB.state_bytes(n, m) == lib.rarc_louvain_workspace_bytes(n, m), (n, m)


def test_the_cases_reach_both_sides_of_the_global_table_edge():
    """the table of the STATE blob is the sweep's global tables only where a vertex may exceed DEG_LDS neighbours"""
    assert LB.global_slots(LB.DEG_LDS + 1, 10 ** 6) == 0 and LB.global_slots(10 ** 6, LB.DEG_LDS) == 0
    assert LB.global_slots(LB.DEG_LDS + 2, LB.DEG_LDS + 1) == 2 * LB.DEG_LDS * 2      # the power of two >= 2 * 8193
    assert LB.global_blocks(LB.DEG_LDS + 2, LB.DEG_LDS + 1) == 32
    assert LB.global_blocks(3_000_000, 3_000_000) == 1                                # 2^23 slots of 8 bytes: one table fits
    # both orders of the two tables occur among the cases above
    sweep = lambda n, m: LB.global_blocks(n, m) * LB.global_slots(n, m) * 8
    assert sweep(8194, 8193) > LB.pair_slots(8193) * 12 and sweep(524_289, 3_000_000) < LB.pair_slots(3_000_000) * 12


def test_parts_are_aligned_and_in_order():
    for off, total in (LB.graph_offsets(65, 100), LB.state_offsets(65, 100)):
        vals = list(off.values())
        assert vals == sorted(vals) and vals[0] == 0 and all(v % LB.ALIGN == 0 for v in vals) and total % LB.ALIGN == 0
    assert LB.scan_blocks(2048) == 1 and LB.scan_blocks(2049) == 2 and LB.scan_blocks(524_289) == 257
