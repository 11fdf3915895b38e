"""The two blobs of csrc/louvain.hip restated on the host (numpy only), for the tests that read what a single step wrote
(tests/test_gpu_louvain_steps.py); held to the library's own size functions in tests/test_louvain_blob_host.py.

Every part starts on a multiple of 256 bytes.  GRAPH blob (csrc/graph_csr.h, lv_graph_carve), in order:
    hdr i64 [32] | row_ptr i64 [n + 1] | k u32 [n] | loop u32 [n] | cnt u32 [n] | adj i32 [2 m] | adj_w u32 [2 m]
    | adj_src i32 [2 m] | list[0..3] i32 [n] each | scan i64 [tiles(n) + 1]
hdr[0] = M2, hdr[1 + b] = the length of list b, hdr[5] = the pairs that were skipped (outside 0 <= i < j < n).
STATE blob (csrc/louvain.hip, lv_state_carve), in order:
    comm[0], comm[1] i32 [n] | tot[0], tot[1] u32 [n] | size[0], size[1] u32 [n] | scal i64 [8] | flag u32 [n]
    | newid i64 [n + 1] | scan i64 [tiles(n) + 1] | table: the larger of the sweep's global tables and the aggregate's pair table
"""
import numpy as np

ALIGN = 256
SCAN_TILE = 2048
DEG_LDS = 8192
H_M2, H_LIST, H_BAD, H_WORDS = 0, 1, 5, 32
S_WORDS = 8
GLOBAL_TABLE_BUDGET = 64 << 20


def align(b: int) -> int:
    return (b + ALIGN - 1) // ALIGN * ALIGN


def scan_blocks(n: int) -> int:
    return (n + SCAN_TILE - 1) // SCAN_TILE


def _carve(parts):
    off, o = {}, 0
    for name, size in parts:
        off[name] = o
        o += align(size)
    return off, o


def graph_offsets(n: int, m: int):
    """(byte offset of every part, the blob's size)"""
    return _carve([("hdr", H_WORDS * 8), ("row_ptr", (n + 1) * 8), ("k", n * 4), ("loop", n * 4), ("cnt", n * 4), ("adj", m * 8),
                   ("adj_w", m * 8), ("adj_src", m * 8)] + [(f"list{b}", n * 4) for b in range(4)]
                  + [("scan", (scan_blocks(n) + 1) * 8)])


def max_degree(n: int, m: int) -> int:
    return min(n - 1, m)


def _pow2_at_least(x: int, start: int) -> int:
    s = start
    while s < x:
        s <<= 1
    return s


def global_slots(n: int, m: int) -> int:
    """slots of one global-memory table of the sweep: none where no vertex can have more than DEG_LDS neighbours"""
    return 0 if max_degree(n, m) <= DEG_LDS else _pow2_at_least(2 * max_degree(n, m), 1024)


def global_blocks(n: int, m: int) -> int:
    s = global_slots(n, m)
    return 0 if not s else max(1, min(32, GLOBAL_TABLE_BUDGET // (s * 8)))


def pair_slots(m: int) -> int:
    return _pow2_at_least(2 * m, 1024)


def state_offsets(n: int, m: int):
    table = max(global_blocks(n, m) * global_slots(n, m) * 8, pair_slots(m) * 12)
    return _carve([("comm0", n * 4), ("comm1", n * 4), ("tot0", n * 4), ("tot1", n * 4), ("size0", n * 4), ("size1", n * 4),
                   ("scal", S_WORDS * 8), ("flag", n * 4), ("newid", (n + 1) * 8), ("scan", (scan_blocks(n) + 1) * 8),
                   ("table", table)])


def graph_bytes(n: int, m: int) -> int:
    return graph_offsets(n, m)[1]


def state_bytes(n: int, m: int) -> int:
    return state_offsets(n, m)[1]


def _view(blob_u8: np.ndarray, off: int, dtype, count: int) -> np.ndarray:
    nbytes = count * np.dtype(dtype).itemsize
    return blob_u8[off: off + nbytes].view(dtype)


def read_graph(blob_u8: np.ndarray, n: int, m: int) -> dict:
    """The parts of a GRAPH blob copied to the host (uint8 [>= graph_bytes(n, m)]): hdr, row_ptr, k, loop, adj, adj_w, adj_src
    (all 2 m slots: the first row_ptr[n] are written) and list[0..3] (all n slots: the first hdr[H_LIST + b] are written)."""
    b = np.ascontiguousarray(blob_u8, dtype=np.uint8)
    off, total = graph_offsets(n, m)
    assert b.size >= total, (b.size, total)
    return {"hdr": _view(b, off["hdr"], np.int64, H_WORDS), "row_ptr": _view(b, off["row_ptr"], np.int64, n + 1),
            "k": _view(b, off["k"], np.uint32, n), "loop": _view(b, off["loop"], np.uint32, n),
            "adj": _view(b, off["adj"], np.int32, 2 * m), "adj_w": _view(b, off["adj_w"], np.uint32, 2 * m),
            "adj_src": _view(b, off["adj_src"], np.int32, 2 * m),
            "list": [_view(b, off[f"list{i}"], np.int32, n) for i in range(4)]}


def read_state(blob_u8: np.ndarray, n: int, m: int) -> dict:
    """comm[s], tot[s], size[s] of both slots of a STATE blob copied to the host: the whole blob, or its start up to `scal`"""
    b = np.ascontiguousarray(blob_u8, dtype=np.uint8)
    off, _ = state_offsets(n, m)
    assert b.size >= off["scal"], (b.size, off["scal"])
    return {"comm": [_view(b, off[f"comm{s}"], np.int32, n) for s in range(2)],
            "tot": [_view(b, off[f"tot{s}"], np.uint32, n) for s in range(2)],
            "size": [_view(b, off[f"size{s}"], np.uint32, n) for s in range(2)]}
