"""The encoder's layer pieces (rarc_enc_embed_ln, rarc_enc_add_ln, rarc_enc_attention, rarc_enc_pool, rarc_enc_pool_mean) refuse
what they must through the C-ABI before anything touches a device: an error code with a rarc_last_error text on a box without a
GPU.  Rejected calls only: the pointers below are never dereferenced and no call here launches a kernel (a call that the
library wrongly accepted would; the sequence-length cases therefore keep n_seq = 1, where the offset b * seq_len * hidden of
the only sequence is 0 whatever seq_len is)."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, aligned pointer nobody reads
E_INVALID, E_UNSUPPORTED = -1, -4


def _embed(lib, ids=P, word=P, pos=P, type0=P, gamma=P, beta=P, n_tokens=4, seq_len=2, hidden=128, vocab=10, out=P):
    return lib.rarc_enc_embed_ln(ids, word, pos, type0, gamma, beta, 1e-12, n_tokens, seq_len, hidden, vocab, out, None)


def _add(lib, x=P, resid=P, gamma=P, beta=P, n_rows=4, hidden=128, out=P):
    return lib.rarc_enc_add_ln(x, resid, gamma, beta, 1e-12, n_rows, hidden, out, None)


def _attn(lib, qkv=P, lens=P, n_seq=1, seq_len=8, hidden=128, heads=2, ctx=P):
    return lib.rarc_enc_attention(qkv, lens, n_seq, seq_len, hidden, heads, ctx, None)


def _pool(lib, hid=P, n_seq=1, seq_len=4, hidden=128, normalize=1, out=P):
    return lib.rarc_enc_pool(hid, n_seq, seq_len, hidden, normalize, out, None)


def _pool_mean(lib, hid=P, lens=P, n_seq=1, seq_len=4, hidden=128, normalize=1, out=P):
    return lib.rarc_enc_pool_mean(hid, lens, n_seq, seq_len, hidden, normalize, out, None)


ENTRIES = {"rarc_enc_embed_ln": _embed, "rarc_enc_add_ln": _add, "rarc_enc_attention": _attn, "rarc_enc_pool": _pool,
           "rarc_enc_pool_mean": _pool_mean}
LN_TEXT = "hidden must be a multiple of 64, <= 1024"
ATTN_TEXT = b"rarc_enc_attention: head_dim must be 32 or 64 and seq_len <= 512"


def _pointer_args(fn):
    import inspect

    return [k for k, v in inspect.signature(fn).parameters.items() if v.default is P]


def _refused(lib, rc, code, text):
    text = text if isinstance(text, bytes) else text.encode()
    return rc == code and text in lib.rarc_last_error()


def test_every_piece_is_bound():
    lib = B.load_library()
    for name in ENTRIES:
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_pointers(entry):
    lib, fn = B.load_library(), ENTRIES[entry]
    text = f"{entry}: bad arguments" if "pool" in entry else f"{entry}: null pointer"
    for arg in _pointer_args(fn):
        assert _refused(lib, fn(lib, **{arg: None}), E_INVALID, text), (entry, arg)


@pytest.mark.parametrize("entry", ["rarc_enc_embed_ln", "rarc_enc_add_ln"])
def test_the_hidden_sizes_of_the_layernorm_pieces(entry):
    lib, fn = B.load_library(), ENTRIES[entry]
    for hidden in (72, 1088, 8, 100, 2048):                   # no multiple of 64 / beyond the 16 columns a lane holds
        assert _refused(lib, fn(lib, hidden=hidden), E_UNSUPPORTED, f"{entry}: {LN_TEXT}"), hidden


@pytest.mark.parametrize("entry", ["rarc_enc_embed_ln", "rarc_enc_add_ln", "rarc_enc_pool", "rarc_enc_pool_mean"])
def test_a_hidden_size_of_zero_or_below_is_refused(entry):
    """0 % 64 == 0 and -64 % 64 == 0 in C: without its own check such a call launches kernels whose every lane is masked off and
    returns RARC_OK over an output nobody wrote"""
    lib, fn = B.load_library(), ENTRIES[entry]
    for hidden in (0, -64, -8, -1024):
        rc = fn(lib, hidden=hidden)
        if "pool" in entry:
            assert _refused(lib, rc, E_INVALID, f"{entry}: bad arguments"), hidden
        else:
            assert _refused(lib, rc, E_UNSUPPORTED, f"{entry}: {LN_TEXT}"), hidden


def test_the_hidden_sizes_of_the_pools():
    lib = B.load_library()
    for hidden in (12, 4, 1021):                              # no multiple of 8 (16-byte rows)
        assert _refused(lib, _pool(lib, hidden=hidden), E_INVALID, "rarc_enc_pool: bad arguments"), hidden
        assert _refused(lib, _pool_mean(lib, hidden=hidden), E_INVALID, "rarc_enc_pool_mean: bad arguments"), hidden
    for hidden in (1032, 2048):                               # the mean is staged in 1024 floats of LDS; CLS pooling has no such limit
        assert _refused(lib, _pool_mean(lib, hidden=hidden), E_INVALID, "rarc_enc_pool_mean: bad arguments"), hidden


def test_the_sequence_length_of_the_pools():
    """rarc_enc_pool reads hidden + b * seq_len * hidden: a negative seq_len with n_seq > 1 would read in front of the buffer.
    (n_seq = 1 here: see the module docstring.)"""
    lib = B.load_library()
    for seq_len in (0, -1):
        assert _refused(lib, _pool(lib, n_seq=1, seq_len=seq_len), E_INVALID, "rarc_enc_pool: bad arguments"), seq_len
        assert _refused(lib, _pool_mean(lib, n_seq=1, seq_len=seq_len), E_INVALID, "rarc_enc_pool_mean: bad arguments"), seq_len


def test_the_shapes_of_the_attention():
    lib = B.load_library()
    for kw in ({"seq_len": 513}, {"seq_len": 0}, {"seq_len": -1}, {"n_seq": 0}, {"n_seq": -1}, {"heads": 0}, {"heads": -2},
               {"hidden": 96, "heads": 2}, {"hidden": 256, "heads": 2}, {"hidden": 0, "heads": 2}, {"hidden": -128, "heads": -2},
               {"hidden": 0, "heads": 0}):                    # head_dim 48, 128, 0; nothing at all
        assert _refused(lib, _attn(lib, **kw), E_UNSUPPORTED, ATTN_TEXT), kw


def test_empty_batches_and_tables():
    lib = B.load_library()
    for n in (0, -1):
        assert _refused(lib, _embed(lib, n_tokens=n), E_UNSUPPORTED, f"rarc_enc_embed_ln: {LN_TEXT}")
        assert _refused(lib, _embed(lib, seq_len=n), E_UNSUPPORTED, f"rarc_enc_embed_ln: {LN_TEXT}")
        assert _refused(lib, _embed(lib, vocab=n), E_INVALID, "rarc_enc_embed_ln: vocab (rows of the word table) must be given")
        assert _refused(lib, _add(lib, n_rows=n), E_UNSUPPORTED, f"rarc_enc_add_ln: {LN_TEXT}")
        assert _refused(lib, _pool(lib, n_seq=n), E_INVALID, "rarc_enc_pool: bad arguments")
        assert _refused(lib, _pool_mean(lib, n_seq=n), E_INVALID, "rarc_enc_pool_mean: bad arguments")
