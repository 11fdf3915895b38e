"""The grouped forms of the filtered search through the C ABI (include/rarc.h: rarc_search_rows_grouped,
rarc_strike_rows_grouped): both exports exist and refuse bad arguments with the documented codes before touching a device —
no GPU needed; rarc_version() is unchanged (the exports are additions)."""
import ctypes

from rag_arc_amd.hip import binding as B

E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4


def _lib():
    return B.load_library()


def test_both_exports_exist_and_the_version_is_unchanged():
    lib = _lib()
    raw = ctypes.CDLL(B.library_path())
    for name in ("rarc_search_rows_grouped", "rarc_search_rows_grouped_workspace_bytes", "rarc_strike_rows_grouped",
                 "rarc_search_rows", "rarc_strike_rows"):
        assert hasattr(raw, name) and hasattr(lib, name), name
    assert lib.rarc_version() == 600


def test_search_rows_grouped_validates_its_arguments():
    lib = _lib()
    p = ctypes.c_void_p(256)
    good = dict(rows=p, fmt=0, n=100, d_pad=128, qb=p, nq=4, lists=p, tiles=p, n_tiles=2, m_max=10, k=5, base=0, xn=None, l2=0,
                oi=p, os=p, st=p, ws=p, wsb=1 << 30)

    def call(**kw):
        a = {**good, **kw}
        return lib.rarc_search_rows_grouped(a["rows"], a["fmt"], a["n"], a["d_pad"], a["qb"], a["nq"], a["lists"], a["tiles"],
                                            a["n_tiles"], a["m_max"], a["k"], a["base"], a["xn"], a["l2"], a["oi"], a["os"], a["st"],
                                            a["ws"], a["wsb"], None)

    for null in ("rows", "qb", "lists", "tiles", "oi", "os", "st", "ws"):
        assert call(**{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error(), null
    assert call(nq=0) == E_INVALID and call(nq=257) == E_INVALID and call(k=0) == E_INVALID and call(k=8193) == E_INVALID
    assert b"rarc_search_rows_grouped" in lib.rarc_last_error()
    assert call(d_pad=4224) == E_UNSUPPORTED and call(d_pad=100) == E_UNSUPPORTED and call(d_pad=0) == E_UNSUPPORTED
    assert call(fmt=1) == E_INVALID and b"fmt" in lib.rarc_last_error()
    assert call(l2=1) == E_INVALID and b"d_xn" in lib.rarc_last_error()
    assert call(n_tiles=0) == E_INVALID and call(n_tiles=5) == E_INVALID and b"n_tiles" in lib.rarc_last_error()
    assert call(m_max=-1) == E_INVALID and call(m_max=101) == E_INVALID
    assert call(wsb=1024) == E_WORKSPACE and b"workspace" in lib.rarc_last_error()
    # the workspace is rarc_search_rows's own, whatever the lists hold
    for nq, k in ((1, 10), (40, 10), (256, 1), (256, 8192)):
        assert lib.rarc_search_rows_grouped_workspace_bytes(nq, k) == lib.rarc_search_rows_workspace_bytes(nq, k) > 0
        assert call(nq=nq, n_tiles=1, k=k, wsb=lib.rarc_search_rows_grouped_workspace_bytes(nq, k) - 512) == E_WORKSPACE
    for nq, k in ((0, 5), (257, 5), (1, 0), (1, 8193)):
        assert lib.rarc_search_rows_grouped_workspace_bytes(nq, k) == 0


def test_strike_rows_grouped_validates_its_arguments():
    lib = _lib()
    p = ctypes.c_void_p(256)

    def call(ids=p, sc=p, nq=1, kp=10, bits=p, off=p, n=100, k=5, oi=p, os=p, cnt=p):
        return lib.rarc_strike_rows_grouped(ids, sc, nq, kp, bits, off, n, 0, k, 0, oi, os, cnt, None)

    for null in ("ids", "sc", "bits", "off", "oi", "os", "cnt"):
        assert call(**{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error(), null
    assert call(nq=0) == E_INVALID and call(k=0) == E_INVALID and call(kp=0) == E_INVALID and call(n=-1) == E_INVALID
