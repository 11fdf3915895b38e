"""rarc_lm_embed_last / rarc_lm_embed_last_prefixed validate their arguments through the C-ABI before anything touches a
device: error codes with a rarc_last_error text on a box without a GPU.  The pointers below are never dereferenced — no
call here is complete: each stops at the check it is about, the "accepted" ones at the workspace check one byte short."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3
H = 256


def _model(lm_head=4096, **kw):
    layers = (B.LmLayer * 1)(B.LmLayer(**{n: 4096 for n, _ in B.LmLayer._fields_}))
    f = dict(hidden=H, n_layers=1, n_q_heads=4, n_kv_heads=2, head_dim=64, inter=512, vocab=1000, rms_eps=1e-6, rope_theta=1e6,
             embed=4096, lm_head=lm_head, final_norm=4096, zero_bias=4096, layers=layers)
    f.update(kw)
    m = B.LmModel(**f)
    m._keep = layers
    return m


def _embed(lib, m=None, ids=P, start=P, n_seq=4, seq_len=32, out_dim=H, normalize=1, ws=P, ws_bytes=1 << 40, out=P, ld=H):
    m = m if m is not None else _model()
    return lib.rarc_lm_embed_last(ctypes.addressof(m) if m else None, ids, start, n_seq, seq_len, out_dim, normalize, ws, ws_bytes,
                                  out, ld, None)


def _embed_prefixed(lib, m=None, ids=P, start=P, n_seq=4, seq_len=32, prefix_of=P, cache=P, n_prefix=4, prefix_len=32, pstart=P,
                    out_dim=H, normalize=1, ws=P, ws_bytes=1 << 40, out=P, ld=H):
    m = m if m is not None else _model()
    return lib.rarc_lm_embed_last_prefixed(ctypes.addressof(m) if m else None, ids, start, n_seq, seq_len, prefix_of, cache, n_prefix,
                                           prefix_len, pstart, out_dim, normalize, ws, ws_bytes, out, ld, None)


def test_symbols_are_exported_and_the_version_stays():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in ("rarc_lm_embed_last", "rarc_lm_embed_last_prefixed"):
        assert name in B.SIGNATURES and getattr(lib, name) is not None


@pytest.mark.parametrize("null", ["ids", "start", "ws", "out"])
def test_null_pointers(null):
    lib = B.load_library()
    assert _embed(lib, **{null: None}) == E_INVALID
    assert b"rarc_lm_embed_last: null pointer" in lib.rarc_last_error()
    assert _embed_prefixed(lib, **{null: None}) == E_INVALID
    assert b"rarc_lm_embed_last_prefixed: null pointer" in lib.rarc_last_error()


@pytest.mark.parametrize("null", ["prefix_of", "cache", "pstart"])
def test_null_prefix_pointers(null):
    lib = B.load_library()
    assert _embed_prefixed(lib, **{null: None}) == E_INVALID
    assert b"rarc_lm_embed_last_prefixed: null pointer" in lib.rarc_last_error()


def test_null_model():
    lib = B.load_library()
    assert lib.rarc_lm_embed_last(None, P, P, 4, 32, H, 1, P, 1 << 40, P, H, None) == E_INVALID
    assert b"rarc_lm_embed_last: null pointer" in lib.rarc_last_error()
    assert _embed(lib, m=_model(final_norm=None)) == E_INVALID and b"incomplete model" in lib.rarc_last_error()


@pytest.mark.parametrize("kw,text", [({"out_dim": 0}, b"out_dim"), ({"out_dim": -3}, b"out_dim"), ({"out_dim": H + 1, "ld": H + 1}, b"out_dim"),
                                     ({"ld": H - 1}, b"ld_out"), ({"out_dim": 64, "ld": 63}, b"ld_out"),
                                     ({"n_seq": 3}, b"multiple of 128"), ({"seq_len": 33}, b"multiple of 128"),
                                     ({"n_seq": 0}, b"multiple of 128")])
def test_bad_arguments(kw, text):
    lib = B.load_library()
    for call, who in ((_embed, b"rarc_lm_embed_last:"), (_embed_prefixed, b"rarc_lm_embed_last_prefixed:")):
        assert call(lib, **kw) == E_INVALID
        msg = lib.rarc_last_error()
        assert text in msg and msg.startswith(who), msg


def test_bad_prefix_shape():
    lib = B.load_library()
    for kw in ({"n_prefix": 0}, {"prefix_len": 0}, {"prefix_len": 4097}):
        assert _embed_prefixed(lib, **kw) == E_INVALID and b"bad prefix shape" in lib.rarc_last_error()


def test_the_limits_themselves_are_accepted():
    """out_dim 1 and hidden, ld_out == out_dim and larger, normalize 0 and 1 pass validation: with a workspace one byte short
    the call gets as far as the workspace check (and no further: nothing is launched)."""
    lib = B.load_library()
    m = _model()
    need = lib.rarc_lm_workspace_bytes(ctypes.addressof(m), 128)
    assert need > 0
    for kw in ({"out_dim": 1, "ld": 1}, {"out_dim": H}, {"out_dim": 64, "ld": 64}, {"out_dim": 64, "ld": 1 << 33}, {"normalize": 0}):
        for call in (_embed, _embed_prefixed):
            assert call(lib, m=m, ws_bytes=need - 1, **kw) == E_WORKSPACE, kw
            assert b"workspace too small" in lib.rarc_last_error()


def test_a_model_without_a_head_embeds_but_gives_no_logits():
    """Qwen3Model checkpoints have no lm_head: the embedding calls accept a null head (they get as far as the workspace
    check), rarc_lm_yes_no_logits and its prefixed twin still refuse the same model as incomplete."""
    lib = B.load_library()
    m = _model(lm_head=None)
    need = lib.rarc_lm_workspace_bytes(ctypes.addressof(m), 128)
    assert _embed(lib, m=m, ws_bytes=need - 1) == E_WORKSPACE and b"rarc_lm_embed_last: workspace" in lib.rarc_last_error()
    assert _embed_prefixed(lib, m=m, ws_bytes=need - 1) == E_WORKSPACE
    rc = lib.rarc_lm_yes_no_logits(ctypes.addressof(m), P, P, 4, 32, 1, 2, P, need - 1, P, None)
    assert rc == E_INVALID and b"rarc_lm_yes_no_logits: incomplete model" in lib.rarc_last_error()
    rc = lib.rarc_lm_yes_no_logits_prefixed(ctypes.addressof(m), P, P, 4, 32, P, P, 4, 32, P, 1, 2, P, need - 1, P, None)
    assert rc == E_INVALID and b"incomplete model" in lib.rarc_last_error()
    # ... and with a head the logits call reaches the same workspace check, under its own name
    full = _model()
    rc = lib.rarc_lm_yes_no_logits(ctypes.addressof(full), P, P, 4, 32, 1, 2, P, need - 1, P, None)
    assert rc == E_WORKSPACE and b"rarc_lm_yes_no_logits: workspace too small" in lib.rarc_last_error()
