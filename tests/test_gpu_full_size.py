"""BASELINE configs 4 and 5 at their FULL corpus size on one GPU (`bench.py --full` checks the same property after its
timed loop; here it is a test): 100M x 768 fp16 rows and 100M x 1024 fp8 rows resident in HBM, one batch of 256 queries,
top-100 — the size-independent property: an exhaustive canonical re-scan of the whole shard finds NO row beating any
query's k-th entry and every returned (id, score) pair is the canonical one (rarc_verify_batch), the answer is sorted by
(score desc, id asc), and a sample of queries agrees with the other scan kernel / with the oracle on the leading rows.
Skipped when the device does not have the memory free (a 192 GB part cannot hold config 4 on one GPU)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from rag_arc_amd.hip import engine

    return engine


def _need(gb):
    import torch

    free, _ = torch.cuda.mem_get_info()
    if free < gb * (1 << 30):
        pytest.skip(f"needs {gb} GiB of free HBM, {free / (1 << 30):.0f} available")


def _sorted_ok(D, I):
    """rows ordered by (score desc, id asc)"""
    tie = D[:, :-1] == D[:, 1:]
    return bool(np.all(D[:, :-1] >= D[:, 1:]) and np.all(I[:, :-1][tie] < I[:, 1:][tie]))


def test_config4_full_shard_100m_x_768_fp16(hip):
    import torch

    import bench
    from rag_arc_amd.hip import binding as B

    _need(175)
    lib = B.load_library()
    n, d, nq, k = 100_000_000, 768, 256, 100
    idx = bench.build_index(torch, lib, B, hip.FlatIndexF16, 0, d, 0, n)
    q = torch.empty((nq, d), dtype=torch.float32, device="cuda")
    B.check(lib.rarc_synth_rows_f32(q.data_ptr(), d, d, 0, nq, 4321, 0))
    assert idx._use_q8(k)                                   # the int8-prefilter scan, four launches (the cascade)
    I, D = idx.search_device(q, k)
    assert len(idx.last_repaired) == 0
    beating, wrong = idx.verify_batch(q, I, D, detail=True)  # all 256 queries, every one of the 100M rows
    assert beating == 0 and wrong == 0
    Dh, Ih = D.cpu().numpy(), I.cpu().numpy()
    assert Ih.min() >= 0 and Ih.max() < n
    assert _sorted_ok(Dh, Ih)
    idx.scan = "mfma16"                                     # the other scan kernel on 32 of the queries: same bits
    I2, D2 = idx.search_device(q[:32], k)
    assert torch.equal(I2, I[:32]) and torch.equal(D2.view(torch.int32), D[:32].view(torch.int32))
    del idx, D, I, D2, I2
    torch.cuda.empty_cache()


def test_config5_full_corpus_100m_x_1024_fp8(hip):
    import torch

    import bench
    from rag_arc_amd.hip import binding as B

    _need(125)
    lib = B.load_library()
    n, d, nq, k = 100_000_000, 1024, 256, 100
    idx = bench.build_index(torch, lib, B, hip.FlatIndexF16, 0, d, 0, n, storage="f8")
    q = torch.empty((nq, d), dtype=torch.float32, device="cuda")
    B.check(lib.rarc_synth_rows_f32(q.data_ptr(), d, d, 0, nq, 4321, 0))
    I, D = idx.search_device(q, k)
    assert len(idx.last_repaired) == 0
    beating, wrong = idx.verify_batch(q, I, D, which=range(0, nq, 4), detail=True)   # 64 queries x 100M rows
    assert beating == 0 and wrong == 0
    assert _sorted_ok(D.cpu().numpy(), I.cpu().numpy())
    del idx, D, I
    torch.cuda.empty_cache()
