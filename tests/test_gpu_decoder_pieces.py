"""The decoder's layer pieces alone, through the C-ABI (rarc_lm_rope_table, rarc_lm_rmsnorm, rarc_lm_rowscale_parts,
rarc_lm_swiglu, rarc_lm_attention, rarc_lm_last_logits, rarc_lm_last_embed, rarc_lm_gather_last), against the float64
references of tests/lm_ref.py with the tolerances derived there, at the shapes and inputs where the whole forward's end-to-end
tolerance sees nothing.  Whatever is claimed to hold on the bits is compared on the bits.  Every output buffer starts as NaN
with one guard row behind it that must stay NaN.  Each test prints its worst |got - ref| / tolerance."""

import numpy as np
import pytest

from tests import lm_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
EPS = 1e-6


def _lib():
    import torch  # noqa: F401  (before the library, as everywhere in the package: both then share one HIP runtime)

    from rag_arc_amd.hip import binding as B

    return B, B.load_library()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _st():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _guarded(rows, cols, dtype=None):
    import torch

    return torch.full((rows + 1, cols), NAN, dtype=dtype or torch.float16, device="cuda")


def _result(out, rows):
    import torch

    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[rows]).all(), "the guard row behind the output was written"
    return o[:rows]


# --------------------------------------------------------------------------------------------------------------- rotary table
def _rope(rows, dh, theta):
    B, lib = _lib()
    out = _guarded(rows, dh)
    B.check(lib.rarc_lm_rope_table(rows, dh, theta, out.data_ptr(), _st()), "rarc_lm_rope_table")
    return _result(out, rows)


@pytest.mark.parametrize("dh,theta", [(64, 1e4), (64, 1e6), (128, 1e4), (128, 1e6)])
def test_rope_table_up_to_position_8191(dh, theta):
    got = R.f64(_rope(8192, dh, theta))
    ref, tol = R.rope_table(8192, dh, theta), R.rope_tolerance(8192, dh, theta)
    err = np.abs(got - ref)                                     # reported in fp16 ulps of a value in [0.5, 1): 2^-11
    pos, col = np.unravel_index(int(np.argmax(err)), err.shape)
    flips = int((got != R.r16(ref)).sum())
    print(f"LM-PIECE rope dh={dh} theta={theta:g}: worst |got - ref| / tolerance = {R.worst(got, ref, tol):.3f}; worst error "
          f"{err[pos, col] * 2.0 ** 11:.2f} fp16 ulps of a cosine near 1 ({err[pos, col]:.2e}) at position {pos}, column {col} (ref "
          f"{ref[pos, col]:+.4f}); {flips} of {got.size} entries are not the fp16 rounding of the reference")
    assert R.worst(got, ref, tol) <= 1.0


# -------------------------------------------------------------------------------------------------------------------- RMSNorm
def _rmsnorm(x, delta, w, with_y=True):
    """(x as the kernel left it, y or None)"""
    B, lib = _lib()
    rows, H = x.shape
    dx, y = _guarded(rows, H), _guarded(rows, H)
    dx[:rows] = _dev(x)
    dd, dw = (None if delta is None else _dev(delta)), _dev(w)
    B.check(lib.rarc_lm_rmsnorm(dx.data_ptr(), None if dd is None else dd.data_ptr(), dw.data_ptr(), EPS, rows, H,
                                y.data_ptr() if with_y else None, _st()), "rarc_lm_rmsnorm")
    xo = _result(dx, rows)
    return xo, (_result(y, rows) if with_y else None)


@pytest.mark.parametrize("H", R.RMS_HIDDEN)
def test_rmsnorm_at_every_width_and_row_count(H):
    w_an = 0.0
    for kind in R.RMS_INPUTS:
        for wkind in R.RMS_WEIGHTS:
            for rows in R.RMS_ROWS:
                x, delta, w = R.rms_input(kind, wkind, rows, H)
                what = f"rmsnorm {kind} {wkind} H={H} rows={rows}"
                for d in (None, delta):
                    xo, y = _rmsnorm(x, d, w)
                    xs = x if d is None else R.h16(R.add_residual(x, d))
                    assert np.array_equal(R.bits(xo), R.bits(xs)), what + ": x written back is not half(x + delta)"
                    lo, hi = R.rms_bounds(xs, w, EPS)
                    assert R.within(y, lo, hi), what + ": outside the rounding interval"
                    w_an = max(w_an, R.worst(y, R.rmsnorm(xs, w, EPS), R.rms_tolerance(xs, w, EPS)))
                    xo2, none = _rmsnorm(x, d, w, with_y=False)            # y = null: only the add
                    assert none is None and np.array_equal(R.bits(xo2), R.bits(xs)), what + ": y = null"
    print(f"LM-PIECE rmsnorm H={H}: worst |got - ref| / tolerance = {w_an:.3f}")
    assert w_an <= 1.0


@pytest.mark.parametrize("H", R.PARTS_HIDDEN)
def test_rowscale_parts(H):
    import torch

    B, lib = _lib()
    worst = 0.0
    for rows in R.PARTS_ROWS:
        x, _, _ = R.rms_input("random", "near_one", rows, H, seed=1)
        ssq = (R.f64(x).reshape(rows, H // 32, 32) ** 2).sum(-1).astype(np.float32)
        out = _guarded(rows, 1, torch.float32)
        B.check(lib.rarc_lm_rowscale_parts(_dev(ssq).data_ptr(), H // 32, EPS, rows, H, out.data_ptr(), _st()), "rarc_lm_rowscale_parts")
        r = _result(out, rows)[:, 0]
        worst = max(worst, R.worst(r, R.rowscale_parts(ssq, H, EPS), R.rowscale_tolerance(ssq, H, EPS)))
        # the same data through rmsnorm (w = 1: y = half(x * inv)): its inv and this r agree within the fp32 sum bound, so
        # half(x * r) lies in the interval of y — and equals y wherever the interval is a single value
        _, y = _rmsnorm(x, None, np.ones(H, np.float16))
        lo, hi = R.rms_bounds(x, np.ones(H), EPS)
        mine = R.r16(R.f64(x) * R.f64(r)[:, None])
        assert R.within(mine, lo, hi) and np.array_equal(mine[lo == hi], R.f64(y)[lo == hi]), (H, rows)
    print(f"LM-PIECE rowscale_parts H={H}: worst |got - ref| / tolerance = {worst:.3f}")
    assert worst <= 1.0


# --------------------------------------------------------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("inter", [8, 128, 136])
def test_swiglu_kernel(inter):
    B, lib = _lib()
    worst = 0.0
    for rows in (1, 5):
        gu = R.swiglu_input(rows, inter)
        out = _guarded(rows, inter)
        B.check(lib.rarc_lm_swiglu(_dev(gu).data_ptr(), rows, inter, out.data_ptr(), _st()), "rarc_lm_swiglu")
        torch_sync = _result(out, rows)
        worst = max(worst, R.swiglu_check(torch_sync, gu, inter))
    print(f"LM-PIECE swiglu inter={inter}: worst |got - want| / (2 fp16 ulps) = {worst:.3f}")
    assert worst <= 1.0


# -------------------------------------------------------------------------------------------------------------------- endings
@pytest.mark.parametrize("H", [128, 1024, 1088])
def test_endings(H):
    import torch

    B, lib = _lib()
    rng = np.random.default_rng(H)
    n, L, V = 5, 7, 50
    w, head = R.h16(1 + rng.uniform(-0.3, 0.3, H)), R.h16(rng.standard_normal((V, H)) * 0.1)
    w_log = w_emb = 0.0
    for stride, off in ((L, L - 1), (1, 0)):
        x = R.h16(rng.standard_normal((n * stride, H)) * rng.uniform(0.1, 8, (n * stride, 1)))
        x[2 * stride + off] = 0                                   # a zero row: zero logits, a zero embedding
        dx, dw, dh = _dev(x), _dev(w), _dev(head)
        out = _guarded(n, 2)
        B.check(lib.rarc_lm_last_logits(dx.data_ptr(), dw.data_ptr(), dh.data_ptr(), EPS, n, stride, off, H, V, 11, 42, out.data_ptr(),
                                        _st()), "rarc_lm_last_logits")
        got = _result(out, n)
        ref, tol = R.last_logits(x, w, head, EPS, n, stride, off, [11, 42])
        w_log = max(w_log, R.worst(got, ref, tol))
        assert (got[2] == 0).all()
        for out_dim, ld, normalize in ((H, H, 0), (H - 8, H + 3, 0), (H - 8, H + 3, 1), (H, H, 1), (1, 1, 1)):
            eo = _guarded(n, ld, torch.float32)
            B.check(lib.rarc_lm_last_embed(dx.data_ptr(), dw.data_ptr(), EPS, n, stride, off, H, out_dim, normalize, eo.data_ptr(), ld,
                                           _st()), "rarc_lm_last_embed")
            e = _result(eo, n)
            assert np.isnan(e[:, out_dim:]).all(), "columns past out_dim were written"
            ref, tol = R.last_embed(x, w, EPS, n, stride, off, out_dim, normalize)
            if normalize:
                w_emb = max(w_emb, R.worst(e[:, :out_dim], ref, tol))
            else:                                                  # nv itself: inside the rounding interval, fp16 numbers
                lo, hi = R.rms_bounds(R.last_rows(x, n, stride, off), w, EPS)
                assert R.within(e[:, :out_dim], lo[:, :out_dim], hi[:, :out_dim])
                assert np.array_equal(e[:, :out_dim], e[:, :out_dim].astype(np.float16).astype(np.float32))
            assert (e[2, :out_dim] == 0).all()
    print(f"LM-PIECE endings H={H}: worst |got - ref| / tolerance: logits {w_log:.3f}, normalised embedding {w_emb:.3f}")
    assert w_log <= 1.0 and w_emb <= 1.0


def test_gather_last_and_its_zero_rows():
    B, lib = _lib()
    rng = np.random.default_rng(9)
    for L, W, n_seq, n_rows in ((1, 8, 1, 1), (7, 136, 3, 5), (40, 256, 5, 128)):
        src = R.h16(rng.standard_normal((n_seq * L, W)))
        out = _guarded(n_rows, W)
        B.check(lib.rarc_lm_gather_last(_dev(src).data_ptr(), L, W, n_seq, n_rows, out.data_ptr(), _st()), "rarc_lm_gather_last")
        assert np.array_equal(R.bits(_result(out, n_rows)), R.bits(R.gather_last(src, L, n_seq, n_rows))), (L, W, n_seq, n_rows)


# ------------------------------------------------------------------------------------------------------------------ attention
_TABLES = {}


def _table(rows, dh, theta=1e6):
    """the device's own rotary table (compared with its reference above), computed once per shape and left unchanged"""
    key = (dh, theta)
    if key not in _TABLES or _TABLES[key].shape[0] < rows:
        _TABLES[key] = _rope(max(rows, 1024), dh, theta)
    return _TABLES[key][:rows]


def _attention(case, kernel, table):
    B, lib = _lib()
    c = case
    T, QD = c.n_seq * c.L, c.n_q * c.dh
    out = _guarded(T, QD)
    d = [_dev(a) for a in (c.qkv, c.start, c.q_norm, c.k_norm, table)]
    pre = [None, None, None] if c.cache is None else [_dev(a) for a in (c.cache, c.prefix_of, c.pstart)]
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.rarc_lm_attention(d[0].data_ptr(), d[1].data_ptr(), c.n_seq, c.L, c.n_q, c.n_kv, c.dh, d[2].data_ptr(), d[3].data_ptr(), c.eps,
                               d[4].data_ptr(), table.shape[0], ptr(pre[0]), ptr(pre[1]), ptr(pre[2]), c.n_prefix, c.P, kernel,
                               out.data_ptr(), _st())
    if rc:
        return rc
    return _result(out, T)


def _fits(case):
    keys = (case.P + case.L + 31) // 32 * 32
    return keys <= (288 if case.dh == 128 else 544)


@pytest.mark.parametrize("cid,kw", R.attn_cases(), ids=[c for c, _ in R.attn_cases()])
def test_attention_both_kernels_every_row(cid, kw):
    """Every context row of every sequence (padding queries included: exact zeros without a prefix; the first real query: the v
    row of its single key) from the streaming kernel, the resident kernel where the keys fit, and the forward's own choice,
    against the two-stage reference; the kernels against each other on the bits; the same call with NaN in every row the
    contract says is never read (and 65504 in the cache rows that are read with probability 0) on the bits again."""
    case = R.attn_case(**kw)
    table = _table(case.rope_rows, case.dh)
    ref, tol = R.attention(case, table)
    facts = R.attention(case, table, online=True)[1]
    stream = _attention(case, 1, table)
    w = R.worst(stream, ref, tol)
    print(f"LM-PIECE attention {cid}: worst |got - ref| / tolerance = {w:.3f}; the reference's walk: {facts['tiles']} tiles, "
          f"{facts['rescales_after_first']} rescales after a wave's first tile, {facts['deferred']} deferred, max log2 p = {facts['max_log2_p']:.2f}")
    assert w <= 1.0
    default = _attention(case, 0, table)
    if _fits(case):
        resident = _attention(case, 2, table)
        assert np.array_equal(R.bits(resident), R.bits(stream)), "resident and streaming kernels differ"
        assert np.array_equal(R.bits(default), R.bits(resident)), "the forward's choice is not the resident kernel"
    else:
        assert _attention(case, 2, table) == -4, "kernel = 2 must be refused when the keys do not fit"
        assert np.array_equal(R.bits(default), R.bits(stream))
    g = stream.reshape(case.n_seq, case.L, case.n_q, case.dh)
    t = case.qkv.reshape(case.n_seq, case.L, case.n_q + 2 * case.n_kv, case.dh)
    for b in range(case.n_seq):
        s0, pq, P, u_min, _ = case.geometry(b)
        if pq < 0:
            assert (R.bits(g[b, :s0]) == 0).all(), "a padding query's context row is not +0"
            for hd in range(case.n_q):                             # one key: p = 1 exactly, the output is its v row
                assert np.array_equal(R.bits(g[b, s0, hd]), R.bits(t[b, s0, case.n_q + case.n_kv + hd // (case.n_q // case.n_kv)]))
    # poison: nothing the contract calls unread may matter
    bad = R.poisoned(case if case.cache is None else R.attn_case(**kw, low_rows=R.F16_MAX))
    for kernel in (1, 2) if _fits(case) else (1,):
        got = _attention(bad, kernel, table)
        keep = np.ones(stream.shape[0], bool)
        if case.cache is not None:                                 # (the padding queries of a prefixed sequence: written, read by
            for b in range(case.n_seq):                            #  nothing, not part of the contract)
                s0, pq = case.geometry(b)[:2]
                if pq >= 0:
                    keep[b * case.L:b * case.L + s0] = False
        assert np.array_equal(R.bits(got[keep]), R.bits(stream[keep])), f"kernel {kernel}: a row that is never read changed the output"


# ---------------------------------------------------------------------------------------------------------------------- chain
def _chain(lm, ids, start, no_id, yes_id, prefix=None, prefix_of=None):
    """the forward of HipCausalLM by hand: the pieces and rarc_enc_gemm, unfused (128 tokens: no fused epilogue takes part)"""
    import torch

    B, lib = _lib()
    n, L = ids.shape
    T, H, I, DH, NQ, NKV = n * L, lm.hidden, lm.inter, lm.head_dim, lm.n_q, lm.n_kv
    QKV, QD = (NQ + 2 * NKV) * DH, NQ * DH
    st = _st()
    f = lambda *s: torch.full(s, NAN, dtype=torch.float16, device="cuda")
    x = lm.embed[torch.from_numpy(ids.reshape(-1).astype(np.int64)).cuda()].contiguous()
    h, delta, qkv, ctx, gu, act = f(T, H), f(T, H), f(T, QKV), f(T, QD), f(T, 2 * I), f(T, I)
    P = prefix["P"] if prefix else 0
    rope = f(P + L, DH)
    B.check(lib.rarc_lm_rope_table(P + L, DH, 1e6, rope.data_ptr(), st))
    d_start = _dev(start)
    zero = lm._zero.data_ptr()
    gemm = lambda a, w, c, m, nn, k: B.check(lib.rarc_enc_gemm(a.data_ptr(), w.data_ptr(), zero, c.data_ptr(), m, nn, k, 0, st), "rarc_enc_gemm")
    cache_layer = 0 if not prefix else (prefix["n"] * P * 2 * NKV * DH * 2 + 255) // 256 * 256
    for l, Ly in enumerate(lm.layers):
        B.check(lib.rarc_lm_rmsnorm(x.data_ptr(), delta.data_ptr() if l else None, Ly["in_norm"].data_ptr(), EPS, T, H, h.data_ptr(), st))
        gemm(h, Ly["qkv_w"], qkv, T, QKV, H)
        pre = [None, None, None] if not prefix else [prefix["cache"].data_ptr() + l * cache_layer, prefix_of.data_ptr(), prefix["start"].data_ptr()]
        B.check(lib.rarc_lm_attention(qkv.data_ptr(), d_start.data_ptr(), n, L, NQ, NKV, DH, Ly["q_norm"].data_ptr(), Ly["k_norm"].data_ptr(),
                                      EPS, rope.data_ptr(), P + L, pre[0], pre[1], pre[2], prefix["n"] if prefix else 0, P, 0,
                                      ctx.data_ptr(), st), "rarc_lm_attention")
        gemm(ctx, Ly["o_w"], delta, T, H, QD)
        B.check(lib.rarc_lm_rmsnorm(x.data_ptr(), delta.data_ptr(), Ly["post_norm"].data_ptr(), EPS, T, H, h.data_ptr(), st))
        gemm(h, Ly["gate_up_w"], gu, T, 2 * I, H)
        B.check(lib.rarc_lm_swiglu(gu.data_ptr(), T, I, act.data_ptr(), st))
        gemm(act, Ly["down_w"], delta, T, H, I)
    B.check(lib.rarc_lm_rmsnorm(x.data_ptr(), delta.data_ptr(), None, EPS, T, H, None, st))
    out = f(n, 2)
    B.check(lib.rarc_lm_last_logits(x.data_ptr(), lm.final_norm.data_ptr(), lm.lm_head.data_ptr(), EPS, n, L, L - 1, H, lm.vocab, no_id,
                                    yes_id, out.data_ptr(), st))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("with_prefix", [False, True])
def test_pieces_chained_by_hand_equal_the_forward_on_the_bits(oracle, monkeypatch, with_prefix):
    """H = 256, 2 layers, 4 / 2 heads of 64, I = 512, 4 x 32 tokens left padded (128 tokens: every GEMM of the forward is a
    plain one, SwiGLU is its own kernel and the last layer runs on all rows): rarc_lm_yes_no_logits[_prefixed] against the same
    kernels called one by one"""
    import torch

    from rag_arc_amd.core.rerank import HipCausalLM

    monkeypatch.setenv("RARC_LM_FUSE_NORM", "0")
    monkeypatch.delenv("RARC_LM_ATTN", raising=False)
    V = 300
    sd = oracle.random_qwen3_state_dict(256, 2, 4, 2, 64, 512, vocab=V, seed=11)
    lm = HipCausalLM(sd, 4, 2, 64, rms_norm_eps=EPS, rope_theta=1e6, fold_norms=False)
    rng = np.random.default_rng(11)
    n, L = 4, 32
    ids = rng.integers(5, V, (n, L)).astype(np.int32)
    start = np.array([0, 7, 31, 16], np.int32)
    for r in range(n):
        ids[r, :start[r]] = 0
    d_ids, d_start = _dev(ids), _dev(start)
    prefix = prefix_of = None
    if with_prefix:
        pre = rng.integers(5, V, (4, 32)).astype(np.int32)
        pstart = np.array([0, 9, 31, 3], np.int32)
        for i in range(4):
            pre[i, :pstart[i]] = 0
        prefix = lm.prefix_kv_device(_dev(pre), _dev(pstart))
        prefix_of = _dev(np.array([0, -1, 1, 2], np.int32))
    want = lm.yes_no_logits_device(d_ids, d_start, 11, 42, prefix=prefix, prefix_of=prefix_of).cpu().numpy()
    got = _chain(lm, ids, start, 11, 42, prefix, prefix_of)
    assert np.isfinite(R.f64(want)).all()
    assert np.array_equal(R.bits(got), R.bits(want))
