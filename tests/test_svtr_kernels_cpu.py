"""The yardsticks and the inputs of tests/test_svtr_kernels_gpu.py, proven without a GPU.

1. svtr_attention_reference equals torch float64 autograd of the plain formula (any head dimension); svtr_block_reference equals
   oracle.mrn_oracle._svtr_block with the DropPath draws injected, plus autograd, for the output, dx and all 12 / 13 parameter
   gradients on every block case, to 1e-12 relative.  hl_split equals a written 22-bit statement of the HL32 format.
2. The conditions the attention cases were made for hold, from the case data alone: no query fully masked and every float64 output
   finite; at N = 200 and N = 300 the local mask leaves queries whose wave's first visited key tile shows them nothing while a wave
   neighbour sees it (and N = 50 has none); "rising" raises every query's float64 tile maximum from tile to tile; "dominant" leads by
   60 nats; magnitude 300 keeps the x3 kernel's operands inside fp16.
3. The inputs discriminate: a deliberately WRONG kernel, evaluated on the CPU, misses float64 by at least 10 x the bound the GPU test
   applies (helpers.baseline_bound: max(8 x the baseline's error, 4 * 2^-24), and for the recomputing backward kernels the derived
   allowances of svtr_cases.grad_extra where they apply).  The tile-level mistakes (keys past N kept with score 0,
   no rescale of the running sums, m_safe not substituted, the last query chunk dropped) run on online_attention below, a float64
   transcription of the kernel's 32-key online softmax; the formula-level ones are `mutant` variants of the yardsticks.  Where a case
   cannot see a mistake -- one key tile never rescales, one head has no neighbour -- the test lists the cases that must.
4. ops.svtr_attention and ops.svtr_attention_bwd refuse a mask that is not symmetric, before anything touches a device."""
import pytest
import torch

from tests import svtr_cases as K
from tests.helpers import (LN2, LOG2E, baseline_bound, hl_parts, hl_split, rel_err, svtr_attention_reference, svtr_block_reference)

MARGIN = 10.0
BLIND = 1e-6                        # a case that cannot see a mistake: the wrong result is the right one to float64 rounding


def close64(a, b, tol=1e-12):
    return rel_err(a, b) <= tol


def miss(wrong, ref, base):
    """by how many times the bound a wrong result misses the reference (NaN: infinitely)"""
    err = rel_err(wrong, ref)
    return float("inf") if err != err else err / baseline_bound(ref, base)


def gmiss(c, wrong, k):
    """the same for a gradient of the recomputing backward kernels, against the WIDER of the two bounds the GPU test applies: on the
    kernel's own forward the plain bound (OR the allowance of the baseline_exact_by_accident cases), on the float64 forward the plain
    bound plus the rounding of the test's own out / lse inputs (svtr_cases.recompute_allowance)"""
    err = rel_err(wrong[k], c["ref"][k])
    plain = baseline_bound(c["ref"][k], c["base"][k])
    return float("inf") if err != err else err / max(plain, K.grad_extra(c, k), plain + K.grad_extra(c, k, 1.0, "float64"))


def case(i):
    return K.att_case(*K.ATT_CASES[i])


ALL = range(len(K.ATT_CASES))


# ---------------------------------------------------------------------------------------------------------
# 1. the yardsticks are what torch computes
# ---------------------------------------------------------------------------------------------------------
def autograd_attention(c):
    B, N, h, d = c["B"], c["N"], c["heads"], c["d"]
    qkv = c["qkv"].double().requires_grad_(True)
    x = qkv.reshape(B, N, 3, h, d).permute(2, 0, 3, 1, 4)
    s = (x[0] * c["scale"]) @ x[1].transpose(-1, -2)
    if c["mask"] is not None:
        s = s + c["mask"].double()
    out = (torch.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(B, N, h * d)
    out.backward(c["dout"].double())
    return out.detach(), torch.logsumexp(s.detach(), -1), qkv.grad


@pytest.mark.parametrize("i", ALL, ids=K.ATT_IDS)
def test_attention_reference_is_torch_autograd(i):
    c = case(i)
    out, lse, g = autograd_attention(c)
    r, C = c["ref"], c["C"]
    tol = 1e-12 if c["mag"] < 100 else 1e-9               # (scores of 1e5 nats: their own rounding, 1e5 x 2^-53, moves a probability by 1e-11)
    assert close64(r["out"], out, tol) and close64(r["lse"], lse) and close64(r["dv"], g[..., 2 * C:], tol)
    if K.saturated(c):          # dS = P o (dP - D) is zero to float64 rounding: two evaluations agree to that rounding, not to 1e-12 of a result of 1e-60
        noise = 1e-12 * c["scale"] * float(c["qkv"].abs().max()) * float(c["ref"]["dv"].abs().max()) * 32
        assert float((r["dq"] - g[..., :C]).abs().max()) <= noise and float((r["dk"] - g[..., C:2 * C]).abs().max()) <= noise * c["N"]
    else:
        assert close64(r["dq"], g[..., :C], tol) and close64(r["dk"], g[..., C:2 * C], tol)
    assert r["out"].dtype == torch.float64 and c["base"]["dq"].dtype == torch.float32


@pytest.mark.parametrize("d,N,mk", K.FALLBACK_CASES)
def test_attention_reference_at_other_head_dimensions(d, N, mk):
    c = K.fallback_case(d, N, mk)
    out, lse, g = autograd_attention(c)
    r, C = c["ref"], c["C"]
    assert C == 2 * d and close64(r["out"], out) and close64(r["lse"], lse)
    assert close64(torch.cat([r["dq"], r["dk"], r["dv"]], -1), g)


@pytest.mark.parametrize("i", range(len(K.BLOCK_CASES)), ids=K.BLOCK_IDS)
def test_block_reference_is_the_oracle_block_and_its_autograd(i):
    from oracle import mrn_oracle as O
    c = K.block_case(*K.BLOCK_CASES[i])
    sd = {"b." + k: (None if v is None else v.double().requires_grad_(True)) for k, v in c["params"].items()}
    x = c["x"].double().requires_grad_(True)
    masks = [] if not c["drop"] else [c["drop1"].double() * K.KEEP, c["drop2"].double() * K.KEEP]      # the oracle divides by keep again
    mask = None if c["mask"] is None else c["mask"].double()
    out = O._svtr_block(sd, "b.", x, c["heads"], mask, True, (1 - K.KEEP) if c["drop"] else 0.0, masks)
    out.backward(c["dout"].double())
    ref_out, G = c["ref"]
    assert close64(ref_out, out.detach())
    assert close64(G["dx"], x.grad)
    assert len(c["names"]) == (13 if c["qkv_bias"] else 12) and sorted(G) == sorted(c["names"])
    for k in c["names"][1:]:
        assert close64(G[k], sd["b." + k[1:]].grad), k
    assert ref_out.dtype == torch.float64 and c["base"][0].dtype == torch.float32
    if c["mixer"] == "Local":
        assert torch.equal(c["mask"], O.svtr_local_mask(*c["HW"]))


def test_hl_split_is_the_22_bit_format():
    """HL32: hi = the nearest fp16 of t = s x (11 significand bits, ties to even), lo = the nearest fp16 of the remainder t - hi.
    Written out with integers: for 2^e <= |t| < 2^(e+1), e >= -14, the nearest fp16 is 2^(e-10) round(t / 2^(e-10)); below 2^-14 the
    quantum stays 2^-24 (the subnormals are kept).  The bound: |hi + lo - t| <= 2^-22 |t| while lo is a normal fp16, and <= 2^-25 (half
    the subnormal quantum) once it is not."""
    def rne16(t):
        t = t.double()
        e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -300))).clamp_min(-14.0)
        quantum = torch.exp2(e - 10)
        return torch.round(t / quantum) * quantum                  # torch.round: half to even
    g = torch.Generator().manual_seed(5)
    x = torch.cat([(torch.rand(4096, generator=g) * 2 - 1) * m for m in (1e-3, 1.5, 12.0, 300.0, 3e-7, 6e-5)]).float()
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 2049.0, 2051.0, 2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -25, 65504.0, 1.0 + 2.0 ** -11])])
    for s in (1.0, 64.0, 2.0 ** -3, 2.0 ** 14):
        t = (x.double() * s).float().double()
        keep = t.abs() < 65504.0
        hi = rne16(t)
        lo = rne16(t - hi)
        got_hi, got_lo = hl_parts(x, s)
        assert torch.equal((got_hi * s)[keep], hi[keep]) and torch.equal((got_lo * s)[keep], lo[keep])
        assert torch.equal(hl_split(x, s)[keep], ((hi + lo) / s)[keep])
        err = (hi + lo - t).abs()[keep]
        assert bool((err <= torch.maximum(2.0 ** -22 * t.abs()[keep], torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    assert float(hl_split(torch.tensor([2.0 ** -24]))) == 2.0 ** -24                    # a subnormal survives
    assert float(hl_split(torch.tensor([1023.5]), 64.0)) == 1023.5                      # 64 x 1023.5 = 65504, the largest fp16
    hi, lo = hl_parts(torch.tensor([1023.75]), 64.0)                                    # 65520: the half-way case rounds to inf, and
    assert float(hi) == float("inf") and float(lo) == float("-inf") and bool(torch.isnan(hi + lo))     # hi + lo is inf - inf


# ---------------------------------------------------------------------------------------------------------
# 2. the cases are what they were made to be
# ---------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_what_the_issue_names():
    Ns = {c[1] for c in K.ATT_CASES}
    assert Ns == {1, 31, 32, 33, 50, 100, 127, 128, 129, 200, 300}
    for N in Ns:
        kinds = {c[3] for c in K.ATT_CASES if c[1] == N}
        assert "none" in kinds and kinds & {"local", "additive"}, N
    for h in (1, 2, 4, 8):
        assert sum(c[2] == h for c in K.ATT_CASES) >= 2
    assert {c[0] for c in K.ATT_CASES} == {1, 3}
    assert {c[4] for c in K.ATT_CASES} == {"uniform", "rising", "falling", "dominant"}
    assert {c[5] for c in K.ATT_CASES} == set(K.SWEEP_MAGNITUDES)
    assert {K.LOCAL_HW[c[1]] for c in K.ATT_CASES if c[3] == "local"} == set(K.LOCAL_HW.values())


@pytest.mark.parametrize("i", ALL, ids=K.ATT_IDS)
def test_no_query_is_fully_masked_and_the_reference_is_finite(i):
    c = case(i)
    if c["mask"] is not None:
        m = c["mask"]
        assert bool(torch.isfinite(m).any(1).all()) and torch.equal(m, m.t()) and float(m.max()) <= 0
        if c["mask_kind"] == "additive":
            assert float(m.min()) >= -4.0 and bool(torch.isfinite(m).all()) and not bool(((m == 0) | torch.isinf(m)).all())
    for m in K.DOUT_MAGNITUDES:
        for k, v in c["refs"][m].items():
            assert bool(torch.isfinite(v).all()), (k, m)
    assert bool(torch.isfinite(c["x3_base"]).all())
    if c["operand"] != "dominant":
        assert abs(float(c["qkv"].abs().max()) / c["mag"] - 1) < 0.05


def test_the_local_mask_leaves_first_tile_blind_queries():
    """the m_run = -inf path of the fp32 kernels (float mask: no tile is skipped, a blind query meets a tile of nothing but -inf) and of
    the bit form (the tile is visited because a neighbour sees it)"""
    count = {N: int(K.first_tile_blind_queries(K.attention_mask("local", N)).sum()) for N in K.LOCAL_HW}
    assert count[50] == 0 and count[200] == 49 and count[300] == 97, count
    for c in K.ATT_CASES:
        if c[3] == "local" and c[1] in (200, 300):
            assert count[c[1]] >= 1
    assert any(c[1] == 200 and c[3] == "local" for c in K.ATT_CASES) and any(c[1] == 300 and c[3] == "local" for c in K.ATT_CASES)


def tile_maxima(c):
    q, k, _ = (t.double() for t in c["qkv"].reshape(c["B"], c["N"], 3, c["heads"], c["d"]).permute(2, 0, 3, 1, 4))
    s = (q @ k.transpose(-1, -2)) * c["scale"]
    return [s[..., k0:k0 + 32].amax(-1) for k0 in range(0, c["N"], 32)]


def test_rising_and_falling_operands_do_what_they_say():
    seen = 0
    for cs in K.ATT_CASES:
        if cs[4] not in ("rising", "falling"):
            continue
        t = tile_maxima(K.att_case(*cs))
        for a, b in zip(t, t[1:]):
            assert bool((b > a).all()) if cs[4] == "rising" else bool((b < a).all())
            seen += 1
    assert seen >= 10


def test_dominant_keys_lead_by_sixty_nats():
    for cs in K.ATT_CASES:
        if cs[4] != "dominant":
            continue
        c = K.att_case(*cs)
        q, k, _ = (t.double() for t in c["qkv"].reshape(c["B"], c["N"], 3, c["heads"], c["d"]).permute(2, 0, 3, 1, 4))
        s = (q @ k.transpose(-1, -2)) * c["scale"]
        if c["mask"] is not None:
            s = s + c["mask"].double()
        top = s.topk(2, -1).values
        assert float((top[..., 0] - top[..., 1]).min()) >= 60.0


def test_magnitude_300_stays_inside_fp16_in_the_x3_kernel():
    for cs in K.ATT_CASES + [(b, n, h, mk, "uniform", 300.0) for b, n, h, mk in K.SWEEP_SHAPES]:
        if cs[5] != 300.0:
            continue
        c = K.att_case(*cs)
        q, k, v = c["qkv"].split(c["C"], -1)
        assert 64 * float(k.abs().max()) < 65504 and 64 * float(v.abs().max()) < 65504
        assert 64 * c["scale"] * LOG2E * float(q.abs().max()) < 65504


# ---------------------------------------------------------------------------------------------------------
# 3. wrong kernels miss the bound
# ---------------------------------------------------------------------------------------------------------
def online_attention(c, mutant=None):
    """the forward kernels' schedule in float64: base-2 scores, keys in tiles of 32 (rows past N read as zeros), running maximum m_run,
    m_safe, corr = exp2(m_run - m_safe), l and O rescaled per tile; queries in chunks of 128 -> (out [B, N, C], lse base 2)"""
    B, N, h, d = c["B"], c["N"], c["heads"], c["d"]
    q, k, v = (t.double() for t in c["qkv"].reshape(B, N, 3, h, d).permute(2, 0, 3, 1, 4))
    T = (N + 31) // 32
    pad = T * 32 - N
    kp, vp = torch.nn.functional.pad(k, (0, 0, 0, pad)), torch.nn.functional.pad(v, (0, 0, 0, pad))
    s = (q * (c["scale"] * LOG2E)) @ kp.transpose(-1, -2)
    if c["mask"] is not None:
        s[..., :N] += c["mask"].double() * LOG2E
    if mutant != "pad_keys_score_0":
        s[..., N:] = float("-inf")
    m_run = torch.full((B, h, N, 1), float("-inf"), dtype=torch.float64)
    l, o = torch.zeros(B, h, N, 1, dtype=torch.float64), torch.zeros(B, h, N, d, dtype=torch.float64)
    for t in range(T):
        st = s[..., 32 * t:32 * t + 32]
        m_new = torch.maximum(m_run, st.amax(-1, keepdim=True))
        m_safe = m_new if mutant == "no_m_safe" else torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        corr = torch.ones_like(m_new) if mutant == "corr_1" else torch.exp2(m_run - m_safe)
        p = torch.exp2(st - m_safe)
        l = l * corr + p.sum(-1, keepdim=True)
        o = o * corr + p @ vp[..., 32 * t:32 * t + 32, :]
        m_run = m_new
    out, lse = o / l, (m_run + torch.log2(l)).squeeze(-1)
    if mutant == "drop_last_chunk":
        first = (N - 1) // 128 * 128
        out[..., first:, :] = 0.0
        lse[..., first:] = 0.0
    return out.permute(0, 2, 1, 3).reshape(B, N, h * d), lse


@pytest.mark.parametrize("i", ALL, ids=K.ATT_IDS)
def test_online_attention_is_the_reference(i):
    c = case(i)
    out, lse = online_attention(c)
    tol = 1e-12 if c["mag"] < 100 else 1e-7
    assert close64(out, c["ref"]["out"], tol) and close64(lse * LN2, c["ref"]["lse"])


def fwd_miss(c, mutant):
    out, lse = online_attention(c, mutant)
    return max(miss(out, c["ref"]["out"], c["base"]["out"]), miss(lse * LN2, c["ref"]["lse"], c["base"]["lse"]))


def test_keys_past_n_kept_with_score_zero_miss_the_bound():
    """every ragged N with uniform operands of magnitude up to 1.5; from 12 on (and with a dominant key) the leading score is so far
    above 0 that a key of score 0 weighs exp(-50) or less"""
    seen = 0
    for cs in K.ATT_CASES:
        c = K.att_case(*cs)
        if c["N"] % 32 == 0:
            assert fwd_miss(c, "pad_keys_score_0") < BLIND
        elif c["mag"] <= 1.5 and c["operand"] in ("uniform",):
            assert fwd_miss(c, "pad_keys_score_0") >= MARGIN, cs
            seen += 1
    assert seen >= 8


def test_running_sums_without_rescale_miss_the_bound():
    for cs in K.ATT_CASES:
        c = K.att_case(*cs)
        if c["N"] <= 32:
            assert fwd_miss(c, "corr_1") < BLIND
        elif c["operand"] == "rising":
            assert fwd_miss(c, "corr_1") >= MARGIN, cs
    assert sum(c[4] == "rising" and c[1] > 32 for c in K.ATT_CASES) >= 2


def test_m_safe_not_substituted_is_nan_where_a_first_tile_is_blind():
    for cs in K.ATT_CASES:
        c = K.att_case(*cs)
        blind = c["mask_kind"] == "local" and c["N"] in (200, 300)
        got = fwd_miss(c, "no_m_safe")
        assert got == float("inf") if blind else got < BLIND, cs


@pytest.mark.parametrize("i", ALL, ids=K.ATT_IDS)
def test_formula_level_mistakes_miss_the_bound(i):
    c = case(i)
    r, b = c["ref"], c["base"]
    assert fwd_miss(c, "drop_last_chunk") >= MARGIN
    # lse kept in base e where base 2 is stored: the forward check multiplies what it reads by ln 2
    assert miss(r["lse"] * LN2, r["lse"], b["lse"]) >= MARGIN and miss(r["lse"] * LOG2E, r["lse"], b["lse"]) >= MARGIN
    ev = lambda m: svtr_attention_reference(c["qkv"], c["mask"], c["heads"], c["scale"], c["dout"], mutant=m)
    w = ev("lse_base")
    assert max(gmiss(c, w, k) for k in ("dq", "dk", "dv")) >= MARGIN
    if c["N"] > 1:                      # (one key: P = 1, dP = D, dS = 0 -- dq and dk are zero with or without D, scaled or not)
        assert gmiss(c, ev("no_D"), "dq") >= MARGIN and gmiss(c, ev("no_D"), "dk") >= MARGIN
    else:
        assert float(r["dq"].abs().max()) <= 1e-12 * c["mag"] and float(r["dk"].abs().max()) <= 1e-12 * c["mag"]
    # a saturated softmax (magnitude 300, a dominant key) has dS = 0 to rounding: dq and dk are the fp32 baseline's noise there, and
    # what scales them cannot be seen; the other cases see it
    if c["N"] > 1 and not K.saturated(c):
        assert gmiss(c, ev("dk_no_scale"), "dk") >= MARGIN
    if c["heads"] > 1:
        w = ev("next_head_v")
        assert miss(w["out"], r["out"], b["out"]) >= MARGIN
        if not K.saturated(c) and c["N"] > 1:
            assert gmiss(c, w, "dq") >= MARGIN and gmiss(c, w, "dk") >= MARGIN
    assert sum(cs[2] > 1 and cs[1] > 1 and cs[5] < 100 and cs[4] != "dominant" for cs in K.ATT_CASES) >= 10


@pytest.mark.parametrize("N", [33, 129])
def test_a_mask_transposed_in_dk_dv_only_misses_the_bound(N):
    """what the kernels would compute from a mask that is not symmetric: forward and dq from mask[key][query] read as the mask, dk / dv
    from its transpose.  The yardstick of that (consistent) mask against the mixed one -- which is why ops refuses such a mask"""
    qkv, mask, dout = K.attention_qkv(1, N, 2, "uniform", 1.5), K.asymmetric_mask(N), K.attention_dout(1, N, 64)
    assert not torch.equal(mask, mask.t()) and float(mask.min()) >= -4.0 and float(mask.max()) <= 0.0
    ev = lambda dt, m=None: svtr_attention_reference(qkv, mask, 2, 32 ** -0.5, dout, dtype=dt, mutant=m)
    r, b, w = ev(torch.float64), ev(torch.float32), ev(torch.float64, "mask_transposed_dkv")
    assert miss(w["dk"], r["dk"], b["dk"]) >= MARGIN and miss(w["dv"], r["dv"], b["dv"]) >= MARGIN
    assert miss(w["dq"], r["dq"], b["dq"]) == 0.0


@pytest.mark.parametrize("i", range(len(K.BLOCK_CASES)), ids=K.BLOCK_IDS)
def test_wrong_blocks_miss_the_bound(i):
    c = K.block_case(*K.BLOCK_CASES[i])
    (_, R), (_, Bs) = c["ref"], c["base"]
    ev = lambda m: svtr_block_reference(c["x"], c["params"], c["drop1"], c["drop2"], c["mask"], c["heads"], c["dout"], mutant=m)[1]
    # the bound the GPU test applies is the LARGER of the fp32 and the x3 baselines' (a mode's own); take the larger here
    def bound(k):
        return max(baseline_bound(R[k], Bs[k]), *(baseline_bound(R[k], c["x3"][m][1][k]) for m in c["x3"]))

    def misses(w, k):
        return rel_err(w[k], R[k]) / bound(k)
    w = ev("ln2_no_xhat")
    assert misses(w, "dx") >= MARGIN and misses(w, "dmixer.proj.weight") >= MARGIN
    w = ev("fc2_bias_wrong_axis")
    assert misses(w, "dmlp.fc2.bias") >= MARGIN
    w = ev("no_drop_in_gradient")
    if c["drop"]:
        for k in ("dmlp.fc2.weight", "dmlp.fc2.bias", "dmlp.fc1.weight", "dnorm2.weight", "dmixer.proj.weight", "dmixer.qkv.weight",
                  "dnorm1.bias", "dx"):
            assert misses(w, k) >= MARGIN, k
    else:
        assert all(rel_err(w[k], R[k]) == 0.0 for k in c["names"])


def test_block_cases_are_the_ones_the_issue_lists():
    got = {(c[0], c[1], c[2], c[3], c[4]) for c in K.BLOCK_CASES}
    assert got == {(64, 2, (8, 25), "Local", False), (128, 4, (4, 25), "Local", True), (256, 8, (2, 25), "Global", True),
                   (64, 2, (3, 11), "Global", False)}
    assert any(not c[5] for c in K.BLOCK_CASES) and any(c[6] == "loose" for c in K.BLOCK_CASES)
    c = K.block_case(*[b for b in K.BLOCK_CASES if b[6] == "loose"][0])
    g = c["params"]["norm1.weight"]
    others = torch.cat([g[:K.LOOSE_CHANNEL], g[K.LOOSE_CHANNEL + 1:]])
    assert float(g[K.LOOSE_CHANNEL].abs() / others.abs().max()) >= 512            # the bound-derived scale is loose by 2^9 .. 2^10
    assert c["drop1"].tolist() == pytest.approx([0, 1 / 0.7, 1 / 0.7]) and c["drop2"].tolist() == pytest.approx([1 / 0.7, 0, 1 / 0.7])


def test_a_branch_whose_multiplier_is_zero_has_zero_gradients():
    """both DropPath multipliers 0 for every sample: out = x, dx = dout, and every parameter gradient is exactly zero in the yardstick
    (what test_svtr_kernels_gpu.py::test_block_with_both_branches_dropped asserts of the kernels)"""
    c = K.block_case(*K.BLOCK_CASES[1])
    zero = torch.zeros(K.BLOCK_B)
    out, G = svtr_block_reference(c["x"], c["params"], zero, zero, c["mask"], c["heads"], c["dout"])
    assert torch.equal(out, c["x"].double()) and torch.equal(G["dx"], c["dout"].double())
    assert all(not bool(G[k].any()) for k in c["names"][1:]) and len(c["names"]) == 13


# ---------------------------------------------------------------------------------------------------------
# 4. a mask that is not symmetric is refused (no device needed: the check comes first)
# ---------------------------------------------------------------------------------------------------------
def test_a_mask_that_is_not_symmetric_is_refused():
    from mrn_amd import ops
    N = 33
    qkv, mask = K.attention_qkv(1, N, 2, "uniform", 1.5), K.asymmetric_mask(N)
    with pytest.raises(ValueError, match=r"ops\.svtr_attention:.*symmetric"):
        ops.svtr_attention(qkv, 2, 32 ** -0.5, mask)
    out, lse = torch.zeros(1, N, 64), torch.zeros(1, 2, N)
    with pytest.raises(ValueError, match=r"ops\.svtr_attention_bwd:.*symmetric"):
        ops.svtr_attention_bwd(qkv, mask, out, out, lse, 2, 32 ** -0.5)
    assert mask._mrn_symmetric == (mask._version, False)
    mask.copy_((mask + mask.t()) / 2)                              # an in-place change invalidates the cached verdict
    with pytest.raises(RuntimeError, match="need CUDA"):           # symmetric now: accepted, and stopped only by the CPU tensors
        ops.svtr_attention(qkv, 2, 32 ** -0.5, mask)
    assert mask._mrn_symmetric == (mask._version, True)
    with pytest.raises(ValueError, match="symmetric"):
        ops.svtr_attention(qkv, 2, 32 ** -0.5, torch.zeros(N, N + 1))
