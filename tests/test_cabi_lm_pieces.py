"""The decoder's layer pieces (rarc_lm_rope_table, rarc_lm_rmsnorm, rarc_lm_rowscale_parts, rarc_lm_swiglu, rarc_lm_attention,
rarc_lm_last_logits, rarc_lm_last_embed, rarc_lm_gather_last) refuse what their kernels cannot take through the C-ABI, before
anything touches a device: an error code with a rarc_last_error text on a box without a GPU.  Rejected calls only: the
pointers below are never dereferenced and no call here launches a kernel, so no output can have been written."""
import ctypes
import inspect

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, aligned pointer nobody reads
OPT = ctypes.c_void_p(8192)    # the same for an argument that MAY be null (left out of the null-pointer sweep)
E_INVALID, E_UNSUPPORTED = -1, -4


def _rope(lib, n_rows=8, head_dim=64, theta=1e6, table=P):
    return lib.rarc_lm_rope_table(n_rows, head_dim, theta, table, None)


def _rms(lib, x=P, delta=None, w=OPT, n_rows=4, hidden=128, y=OPT):
    return lib.rarc_lm_rmsnorm(x, delta, w, 1e-6, n_rows, hidden, y, None)


def _parts(lib, ssq=P, n_parts=4, n_rows=4, hidden=128, r=P):
    return lib.rarc_lm_rowscale_parts(ssq, n_parts, 1e-6, n_rows, hidden, r, None)


def _swiglu(lib, gu=P, n_rows=4, inter=128, out=P):
    return lib.rarc_lm_swiglu(gu, n_rows, inter, out, None)


def _attn(lib, qkv=P, start=P, n_seq=1, seq_len=8, n_q=4, n_kv=2, head_dim=64, q_norm=P, k_norm=P, rope=P, rope_rows=None, cache=None,
          prefix_of=None, prefix_start=None, n_prefix=0, prefix_len=0, kernel=0, ctx=P):
    rope_rows = (prefix_len if cache is not None else 0) + seq_len if rope_rows is None else rope_rows
    return lib.rarc_lm_attention(qkv, start, n_seq, seq_len, n_q, n_kv, head_dim, q_norm, k_norm, 1e-6, rope, rope_rows, cache, prefix_of,
                                 prefix_start, n_prefix, prefix_len, kernel, ctx, None)


def _logits(lib, x=P, w=P, head=P, n_seq=2, row_stride=4, row_off=3, hidden=128, vocab=100, no_id=1, yes_id=2, out=P):
    return lib.rarc_lm_last_logits(x, w, head, 1e-6, n_seq, row_stride, row_off, hidden, vocab, no_id, yes_id, out, None)


def _embed(lib, x=P, w=P, n_seq=2, row_stride=4, row_off=3, hidden=128, out_dim=128, normalize=1, out=P, ld_out=128):
    return lib.rarc_lm_last_embed(x, w, 1e-6, n_seq, row_stride, row_off, hidden, out_dim, normalize, out, ld_out, None)


def _gather(lib, src=P, seq_len=4, width=128, n_seq=2, n_rows=4, dst=P):
    return lib.rarc_lm_gather_last(src, seq_len, width, n_seq, n_rows, dst, None)


ENTRIES = {"rarc_lm_rope_table": _rope, "rarc_lm_rmsnorm": _rms, "rarc_lm_rowscale_parts": _parts, "rarc_lm_swiglu": _swiglu,
           "rarc_lm_attention": _attn, "rarc_lm_last_logits": _logits, "rarc_lm_last_embed": _embed, "rarc_lm_gather_last": _gather}


def _refused(lib, rc, code, entry):
    return rc == code and lib.rarc_last_error().startswith(entry.encode() + b":")


def test_every_piece_is_bound():
    lib = B.load_library()
    for name in ENTRIES:
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_pointers(entry):
    lib, fn = B.load_library(), ENTRIES[entry]
    for arg in [k for k, v in inspect.signature(fn).parameters.items() if v.default is P]:
        assert _refused(lib, fn(lib, **{arg: None}), E_INVALID, entry), (entry, arg)
    assert _refused(lib, _rms(lib, w=None), E_INVALID, "rarc_lm_rmsnorm")      # the weights may only be null with y
    # a cache without its owner / start arrays
    assert _refused(lib, _attn(lib, cache=P, prefix_of=None, prefix_start=P, n_prefix=1, prefix_len=32), E_INVALID, "rarc_lm_attention")
    assert _refused(lib, _attn(lib, cache=P, prefix_of=P, prefix_start=None, n_prefix=1, prefix_len=32), E_INVALID, "rarc_lm_attention")


def test_counts_of_zero_or_below():
    """0 % n == 0 and -8 % 8 == 0 in C: without their own checks such calls launch nothing (or a grid of size 0) and return
    RARC_OK over an output nobody wrote"""
    lib = B.load_library()
    for v in (0, -1, -128):
        assert _refused(lib, _rope(lib, n_rows=v), E_INVALID, "rarc_lm_rope_table")
        assert _refused(lib, _rms(lib, n_rows=v), E_UNSUPPORTED, "rarc_lm_rmsnorm")
        assert _refused(lib, _rms(lib, hidden=v), E_UNSUPPORTED, "rarc_lm_rmsnorm")
        assert _refused(lib, _parts(lib, n_rows=v), E_UNSUPPORTED, "rarc_lm_rowscale_parts")
        assert _refused(lib, _parts(lib, hidden=v, n_parts=v // 32), E_UNSUPPORTED, "rarc_lm_rowscale_parts")
        assert _refused(lib, _swiglu(lib, n_rows=v), E_UNSUPPORTED, "rarc_lm_swiglu")
        assert _refused(lib, _swiglu(lib, inter=v), E_UNSUPPORTED, "rarc_lm_swiglu")
        assert _refused(lib, _attn(lib, n_seq=v), E_INVALID, "rarc_lm_attention")
        assert _refused(lib, _attn(lib, seq_len=v, rope_rows=8), E_INVALID, "rarc_lm_attention")
        assert _refused(lib, _attn(lib, n_q=v), E_UNSUPPORTED, "rarc_lm_attention")
        assert _refused(lib, _attn(lib, n_kv=v), E_UNSUPPORTED, "rarc_lm_attention")
        assert _refused(lib, _attn(lib, n_q=v, n_kv=v), E_UNSUPPORTED, "rarc_lm_attention")
        assert _refused(lib, _attn(lib, cache=P, prefix_of=P, prefix_start=P, n_prefix=v, prefix_len=32), E_INVALID, "rarc_lm_attention")
        assert _refused(lib, _attn(lib, cache=P, prefix_of=P, prefix_start=P, n_prefix=1, prefix_len=v, rope_rows=64), E_INVALID, "rarc_lm_attention")
        for fn, name in ((_logits, "rarc_lm_last_logits"), (_embed, "rarc_lm_last_embed")):
            for arg in ("n_seq", "hidden", "row_stride"):
                assert _refused(lib, fn(lib, **{arg: v}), E_INVALID, name), (name, arg, v)
        assert _refused(lib, _logits(lib, vocab=v), E_INVALID, "rarc_lm_last_logits")
        assert _refused(lib, _embed(lib, out_dim=v), E_INVALID, "rarc_lm_last_embed")
        for arg in ("seq_len", "width", "n_seq"):
            assert _refused(lib, _gather(lib, **{arg: v}), E_UNSUPPORTED, "rarc_lm_gather_last"), (arg, v)


def test_widths_the_vector_loads_cannot_take():
    lib = B.load_library()
    for hidden in (4, 12, 100, 1021):                          # rmsnorm: 16-byte pieces
        assert _refused(lib, _rms(lib, hidden=hidden), E_UNSUPPORTED, "rarc_lm_rmsnorm"), hidden
    for hidden, n_parts in ((64, 2), (96, 3), (160, 5), (8, 0), (128, 8), (256, 4)):   # float4 loads of the partial sums; n_parts = hidden / 32
        assert _refused(lib, _parts(lib, hidden=hidden, n_parts=n_parts), E_UNSUPPORTED, "rarc_lm_rowscale_parts"), hidden
    for inter in (4, 12, 100):
        assert _refused(lib, _swiglu(lib, inter=inter), E_UNSUPPORTED, "rarc_lm_swiglu"), inter
    for width in (4, 12, 100):
        assert _refused(lib, _gather(lib, width=width), E_UNSUPPORTED, "rarc_lm_gather_last"), width
    assert _refused(lib, _gather(lib, n_seq=5, n_rows=4), E_UNSUPPORTED, "rarc_lm_gather_last")


def test_the_shapes_of_the_attention():
    lib = B.load_library()
    for kw in ({"head_dim": 32}, {"head_dim": 96}, {"head_dim": 256}, {"head_dim": 0}, {"n_q": 3, "n_kv": 2}, {"n_q": 2, "n_kv": 4}):
        assert _refused(lib, _attn(lib, **kw), E_UNSUPPORTED, "rarc_lm_attention"), kw
    for kernel in (-1, 3):
        assert _refused(lib, _attn(lib, kernel=kernel), E_INVALID, "rarc_lm_attention"), kernel
    pre = dict(cache=P, prefix_of=P, prefix_start=P, n_prefix=2)
    assert _refused(lib, _attn(lib, seq_len=8, rope_rows=7), E_INVALID, "rarc_lm_attention")              # a table shorter than the keys
    assert _refused(lib, _attn(lib, seq_len=8, prefix_len=32, rope_rows=39, **pre), E_INVALID, "rarc_lm_attention")
    assert _refused(lib, _attn(lib, prefix_len=4097, **pre), E_INVALID, "rarc_lm_attention")
    # the resident kernel asked for by name: refused when the keys do not fit, never replaced by the other kernel
    for kw in ({"head_dim": 128, "n_q": 2, "n_kv": 1, "seq_len": 289}, {"head_dim": 128, "n_q": 2, "n_kv": 1, "seq_len": 320},
               {"head_dim": 64, "seq_len": 545}, {"head_dim": 64, "seq_len": 4096},
               {"head_dim": 128, "n_q": 2, "n_kv": 1, "seq_len": 200, "prefix_len": 96, **pre}, {"head_dim": 64, "seq_len": 500, "prefix_len": 64, **pre}):
        assert _refused(lib, _attn(lib, kernel=2, **kw), E_UNSUPPORTED, "rarc_lm_attention"), kw


def test_the_row_and_the_columns_of_the_endings():
    lib = B.load_library()
    for fn, name in ((_logits, "rarc_lm_last_logits"), (_embed, "rarc_lm_last_embed")):
        for kw in ({"row_off": -1}, {"row_off": 4}, {"row_stride": 1, "row_off": 1}):
            assert _refused(lib, fn(lib, **kw), E_INVALID, name), (name, kw)
    for kw in ({"no_id": -1}, {"yes_id": -1}, {"no_id": 100}, {"yes_id": 100}):
        assert _refused(lib, _logits(lib, **kw), E_INVALID, "rarc_lm_last_logits"), kw
    for kw in ({"out_dim": 129}, {"out_dim": 64, "ld_out": 63}, {"out_dim": 128, "ld_out": 0}):
        assert _refused(lib, _embed(lib, **kw), E_INVALID, "rarc_lm_last_embed"), kw


def test_the_rope_table():
    lib = B.load_library()
    for kw in ({"head_dim": 32}, {"head_dim": 96}, {"head_dim": 0}, {"n_rows": 2 ** 26, "head_dim": 128}):
        assert _refused(lib, _rope(lib, **kw), E_UNSUPPORTED, "rarc_lm_rope_table"), kw
    for theta in (0.0, -1e4, float("inf"), float("nan")):
        assert _refused(lib, _rope(lib, theta=theta), E_INVALID, "rarc_lm_rope_table"), theta
