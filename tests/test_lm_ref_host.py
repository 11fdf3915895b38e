"""tests/lm_ref.py checked without a GPU.  (1) The float64 references of the decoder's pieces, chained into a whole forward in
their exact mode (no fp16 emulation), give the logits of oracle.qwen3_last_logits_f32 to the float32 rounding of the oracle
itself.  (2) Every comparator REJECTS every planted error at the shapes tests/test_gpu_decoder_pieces.py runs: an error the
references would let through is an error the GPU tests cannot see."""
import numpy as np
import pytest

from tests import lm_ref as R

CFG = dict(num_attention_heads=4, num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6, rope_theta=1e6)
CASES = R.attn_cases()


def _small_model(oracle):
    sd = oracle.random_qwen3_state_dict(128, 2, 4, 2, 64, 256, vocab=200, seed=3)
    rng = np.random.default_rng(3)
    for k in sd:                                               # q / k-norm weights well above 1, as real checkpoints have
        if "q_norm" in k or "k_norm" in k:
            sd[k] = (sd[k] * 0 + rng.uniform(1.5, 4.0, sd[k].shape)).astype(np.float32)
    ids = rng.integers(5, 200, (5, 40))
    start = np.array([0, 7, 33, 39, 16], np.int32)
    mask = (np.arange(40)[None, :] >= start[:, None]).astype(np.int64)
    return sd, ids, start, mask


def test_chained_references_equal_the_float32_oracle(oracle):
    """Two layers, 4 / 2 heads of 64, five left-padded sequences.  The oracle works in float32: ~2000 roundings of 2^-24 on the
    way of a logit of size ~1 through dot products of up to 256 terms; measured here its distance from the float64 chain is
    7.5e-6 on logits up to 3.7.  Asserted: 1e-4 (13 times that; a masking, head-mapping or rotary mistake moves a logit by 1e-2 and more)."""
    sd, ids, start, mask = _small_model(oracle)
    want = oracle.qwen3_last_logits_f32(sd, CFG, ids, mask, [11, 42])
    got = R.forward_logits(sd, CFG, ids, start, [11, 42], exact=True)
    err = float(np.abs(got - want).max())
    print(f"LM-REF chain vs float32 oracle: max|dlogit| = {err:.2e} on logits up to {np.abs(want).max():.2f}")
    assert err <= 1e-4
    wrong_row = R.forward_logits(sd, CFG, ids, start, [11, 42], exact=True, row_off=38)       # final norm over the wrong row
    assert float(np.abs(wrong_row - want).max()) > 1e-2


# ----------------------------------------------------------------------------------------------------- planted errors: attention
def _max_keys(kw):
    return kw.get("P", 0) + kw["L"] - min(max(s, 0) for s in kw["starts"])


def _applies(plant, kw):
    prof, L = kw["profile"], kw["L"]
    s_in = [R.clamp(s, 0, L - 1) for s in kw["starts"]]
    if plant == "causal+1":                                    # the next key scores above every visible one
        return prof == "ramp_fast" and any(s < L - 1 for s in s_in)
    if plant == "start+1":                                     # the first key is the maximum; a sequence without a prefix
        return prof == "peak_first" and any(s < L - 1 and (not kw.get("P") or kw["prefix_of"][b] < 0) for b, s in enumerate(s_in))
    if plant == "umin-1":                                      # the cache row in front of pstart scores above the maximum
        return prof == "peak_first" and bool(kw.get("P")) and any(
            o >= 0 and R.clamp(kw["pstarts"][o], 0, kw["P"] - 1) > 0 for o in kw["prefix_of"])
    if plant in ("no_rescale", "l_not_rescaled"):
        return prof in ("ramp_fast", "ramp_slow", "spike_one") and _max_keys(kw) >= 64
    if plant == "wrong_kv_head":
        return prof == "flat" and kw["n_kv"] > 1
    if plant in ("rotate_sign", "knorm_for_q"):
        return prof == "flat" and _max_keys(kw) >= 16
    raise ValueError(plant)


PLANTS = ("causal+1", "umin-1", "start+1", "no_rescale", "l_not_rescaled", "wrong_kv_head", "rotate_sign", "knorm_for_q")


@pytest.mark.parametrize("plant", PLANTS)
def test_attention_comparator_rejects(plant):
    n, least = 0, np.inf
    for cid, kw in CASES:
        if not _applies(plant, kw):
            continue
        case = R.attn_case(**kw)
        table = R.h16(R.rope_table(case.rope_rows, case.dh, case.theta))       # an fp16 table, as the device's is
        ref, tol = R.attention(case, table)
        online = plant in ("no_rescale", "l_not_rescaled")
        bad = R.attention(case, table, plant=plant, online=online)[0]
        if online:                                             # the walk itself, without the error, is the reference
            good, facts = R.attention(case, table, online=True)
            assert R.worst(good, ref, tol) < 0.01, cid
            if facts["rescales_after_first"] == 0:
                continue
        w = R.worst(bad, ref, tol)
        assert w > 1.0, f"{cid}: {plant} stays within the tolerance ({w:.3f} of it)"
        n, least = n + 1, min(least, w)
    print(f"LM-REF planted {plant}: rejected in {n} cases, the closest at {least:.1f} tolerances")
    assert n >= 4


def test_the_ramps_do_what_their_names_say():
    """ramp_fast: every tile after the first raises the maximum (no deferral past the first tile of a wave); ramp_slow: deferral
    runs to its limit, p reaches almost 2^11; both read off the reference's own scores"""
    for prof, L in (("ramp_fast", 160), ("ramp_slow", 160)):
        case = R.attn_case(prof, 64, 4, 2, L, [0, 1, 33, L - 1])
        facts = R.attention(case, online=True)[1]
        print(f"LM-REF {prof}: {facts}")
        if prof == "ramp_fast":
            assert facts["rescales_after_first"] > 0 and facts["max_log2_p"] <= 0.5
        else:
            assert facts["deferred"] > 0 and 10.0 < facts["max_log2_p"] <= R.DEFER


# ---------------------------------------------------------------------------------------------- planted errors: RMSNorm, endings
def test_rmsnorm_interval_rejects_one_ulp():
    """one fp16 ulp in one output, at every width and input kind of the GPU test: outside [lo, hi] unless that element sits on a
    rounding boundary (where the interval is two values wide and the neighbour on the far side is still rejected)"""
    for H in R.RMS_HIDDEN:
        for kind in ("random", "spike", "full_range"):
            x, _, w = R.rms_input(kind, "near_one", 5, H)
            lo, hi = R.rms_bounds(x, w, 1e-6)
            good = R.rmsnorm_chain(x, w, 1e-6)
            assert R.within(good, lo, hi)
            r, c = 3, int(np.argmax(np.abs(good[3])))
            for sign in (1, -1):
                bad = good.copy()
                bad[r, c] = (hi if sign > 0 else lo)[r, c] + sign * R.f16_ulp(good[r, c])
                assert not R.within(bad, lo, hi), (H, kind, sign)


def test_ending_comparators_reject_the_wrong_row():
    rng = np.random.default_rng(5)
    for H in (128, 1024, 1088):
        L, n = 6, 3
        x, w, head = R.h16(rng.standard_normal((n * L, H))), R.h16(1 + rng.uniform(-0.2, 0.2, H)), R.h16(rng.standard_normal((50, H)) * 0.1)
        ref, tol = R.last_logits(x, w, head, 1e-6, n, L, L - 1, [11, 42])
        off, _ = R.last_logits(x, w, head, 1e-6, n, L, L - 2, [11, 42])
        assert R.worst(off, ref, tol) > 1.0
        for normalize in (0, 1):
            ref, tol = R.last_embed(x, w, 1e-6, n, L, L - 1, H - 8, normalize)
            off, _ = R.last_embed(x, w, 1e-6, n, L, L - 2, H - 8, normalize)
            assert R.worst(off, ref, np.maximum(tol, 2.0 ** -30)) > 1.0
