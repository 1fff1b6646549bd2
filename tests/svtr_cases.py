"""Shapes and inputs shared by test_svtr_kernels_cpu.py (which proves the yardsticks, the conditions the inputs were made for and that
they discriminate) and test_svtr_kernels_gpu.py (which runs attention.hip, SvtrAttentionFn, the operand producers and
modules.svtr.Block.forward_train on them).  Every input is fp32, made on the CPU from a seeded generator, and cached with its float64
reference and its baselines (tests/helpers.py): each is computed once."""
import functools

import torch

from mrn_amd.modules.svtr import local_attention_mask
from tests.helpers import (SVTR_BLOCK_PARAMS, svtr_attention_reference, svtr_attention_x3_baseline, svtr_block_reference)
from tests.router_cases import rnd

# ---------------------------------------------------------------------------------------------------------
# attention: (B, N, heads, mask kind, operand kind, magnitude of qkv).  The kernels give a wave 32 queries and a workgroup 128, and walk
# the keys in tiles of 32: N = 1, 31 / 32 / 33, 127 / 128 / 129 (the second chunk holds one query, the last tile one key), and the sizes
# of the shipped stages (50, 100, 200) and of a 12-row map (300).
# ---------------------------------------------------------------------------------------------------------
LOCAL_HW = {50: (2, 25), 100: (4, 25), 200: (8, 25), 300: (12, 25), 128: (4, 32)}
ATT_CASES = [
    (1, 1, 1, "none", "uniform", 1.5), (1, 1, 2, "additive", "uniform", 1.5),
    (3, 31, 1, "none", "uniform", 1.5), (1, 31, 4, "additive", "uniform", 12.0),
    (1, 32, 2, "none", "rising", 1.5), (3, 32, 2, "additive", "uniform", 1e-3),
    (1, 33, 8, "none", "uniform", 1.5), (3, 33, 1, "additive", "falling", 1.5),
    (1, 50, 2, "none", "uniform", 300.0), (3, 50, 2, "local", "uniform", 1.5),
    (1, 100, 4, "none", "dominant", 1.5), (1, 100, 4, "local", "uniform", 12.0),
    (1, 127, 1, "none", "rising", 1.5), (1, 127, 2, "additive", "uniform", 1.5),
    (3, 128, 4, "none", "uniform", 1e-3), (1, 128, 4, "local", "uniform", 1.5),
    (1, 129, 2, "none", "falling", 1.5), (1, 129, 8, "additive", "uniform", 300.0),
    (1, 200, 2, "none", "uniform", 12.0), (3, 200, 2, "local", "uniform", 1.5), (1, 200, 8, "local", "dominant", 1.5),
    (1, 300, 1, "none", "rising", 1.5), (1, 300, 4, "local", "uniform", 1.5), (1, 300, 8, "local", "uniform", 1e-3),
]
ATT_IDS = ["B%d-N%d-h%d-%s-%s-%g" % c for c in ATT_CASES]
SWEEP_MAGNITUDES = [1e-3, 1.5, 12.0, 300.0]
SWEEP_SHAPES = [(1, 129, 2, "none"), (1, 200, 2, "local"), (1, 33, 4, "additive")]          # every magnitude on each, uniform operands
DOUT_MAGNITUDES = [1.0, 1e-6, 1e4]
HEAD_DIM = 32


def attention_mask(kind, N):
    """None; the local 7 x 11 window on the map of N tokens; or a symmetric finite mask with values in [-4, 0] that is not binary"""
    if kind == "none":
        return None
    if kind == "local":
        H, W = LOCAL_HW[N]
        return local_attention_mask(H, W, 7, 11)
    assert kind == "additive"
    a = rnd(N, N, seed=300)
    return -(a + a.t()).abs() * 2.0            # |a + a^T| <= 2


def asymmetric_mask(N):
    """finite, values in [-4, 0], mask[i][j] != mask[j][i] off the diagonal: what ops.svtr_attention must refuse"""
    return -(rnd(N, N, seed=301) + 1.0) * 2.0


def attention_qkv(B, N, heads, operand, mag, d=HEAD_DIM):
    """qkv [B, N, 3 heads d], max|.| = mag (for "dominant": of v; q and k are what the score gap needs).
    "rising" / "falling": every q has positive coordinates and k_j = c_j u with u positive, c_j = tile(j) + 1 + a jitter below 1/2
    (reversed for "falling"), so every query's tile maximum grows (shrinks) from each 32-key tile to the next.
    "dominant": k_j a vector of +-1, q_i = g k_i with g such that query i's score for key i leads every other by 64 nats at least."""
    C = heads * d
    shape = (B, N, heads, d)
    if operand == "uniform":
        q, k, v = (rnd(*shape, seed=310 + i) * mag for i in range(3))
    elif operand in ("rising", "falling"):
        q = (rnd(*shape, seed=310) * 0.25 + 0.75) * mag
        u = rnd(1, 1, heads, d, seed=311) * 0.25 + 0.75
        j = torch.arange(N)
        c = (j // 32 + 1).float() + (rnd(N, seed=312) + 1) * 0.25
        if operand == "falling":
            c = c.flip(0)
        k = (u * (c / c.max()).view(1, N, 1, 1) * mag).expand(*shape)
        v = rnd(*shape, seed=313) * mag
    else:
        assert operand == "dominant"
        k = torch.sign(rnd(*shape, seed=310) + 1e-9)
        dots = torch.einsum("bihd,bjhd->bhij", k, k)
        gap = (d - (dots - torch.eye(N) * 1e9).amax(-1)).min()
        assert float(gap) > 0, "two keys coincide"
        q = k * (64.0 / (d ** -0.5 * float(gap)))
        v = rnd(*shape, seed=313) * mag
    return torch.cat([t.reshape(B, N, C) for t in (q, k, v)], -1).contiguous()


def attention_dout(B, N, C, mag=1.0):
    return (rnd(B, N, C, seed=320) * mag).float()


@functools.lru_cache(maxsize=None)
def att_case(B, N, heads, mask_kind, operand, mag, d=HEAD_DIM):
    """inputs, the float64 reference and the fp32 baseline (forward and, per dout magnitude, backward), and the x3 baseline of the
    forward.  refs[m] / bases[m]: the yardstick on dout(m); ref / base: at magnitude 1"""
    qkv = attention_qkv(B, N, heads, operand, mag, d)
    mask = attention_mask(mask_kind, N)
    scale = d ** -0.5
    douts = {m: attention_dout(B, N, heads * d, m) for m in DOUT_MAGNITUDES}
    refs = {m: svtr_attention_reference(qkv, mask, heads, scale, g, torch.float64) for m, g in douts.items()}
    bases = {m: svtr_attention_reference(qkv, mask, heads, scale, g, torch.float32) for m, g in douts.items()}
    c = dict(B=B, N=N, heads=heads, mask_kind=mask_kind, operand=operand, mag=mag, d=d, C=heads * d, scale=scale, qkv=qkv, mask=mask,
             douts=douts, refs=refs, bases=bases, dout=douts[1.0], ref=refs[1.0], base=bases[1.0])
    if d == HEAD_DIM:
        c["x3_base"] = svtr_attention_x3_baseline(qkv, mask, heads, scale)
    return c


def saturated(c):
    """scores of 1e4 nats and more, or a key that leads by 60: the softmax is one-hot to rounding, dS = P o (dP - D) is zero in exact
    arithmetic wherever P is not, and dq / dk are far below the rounding of the sums they come from"""
    return c["mag"] >= 100 or c["operand"] == "dominant"


def saturated_grad_allowance(c, key, dout_mag=1.0):
    """the `extra` of within_baseline for dq / dk of a saturated case (0 for every other case and for dv), relative to max|reference|.
    There the exact dq and dk are 1e-20 and less, and what any fp32 evaluation returns is the rounding of dS = P o (dP - D): dP[i][j] and
    D[i] are sums of d products of dO and v (O is a convex combination of rows of v), each off by at most d 2^-24 times the sum of the
    absolute products, so |dP - D| is off by at most E = 3 d^2 2^-24 max|dO| max|v| (2 for the two sums, 1 for O's own rounding);
    sum_j P[i][j] = 1 gives |dq[i]| <= scale max|k| E, and sum_i P[i][j] <= N gives |dk[j]| <= scale max|q| N E."""
    if not saturated(c) or key not in ("dq", "dk"):
        return 0.0
    q, k, v = c["qkv"].split(c["C"], -1)
    E = 3 * c["d"] ** 2 * 2.0 ** -24 * float(c["douts"][dout_mag].abs().max()) * float(v.abs().max())
    allow = c["scale"] * E * (float(k.abs().max()) if key == "dq" else float(q.abs().max()) * c["N"])
    m = float(c["refs"][dout_mag][key].abs().max())
    return allow / (m if m > 0 else 1.0)


def baseline_exact_by_accident(c):
    """the cases, told from the case data alone, where the fp32 baseline's probabilities are exact for no reason a kernel shares: one
    key (P = exp(0) / 1), or a softmax that is one-hot to rounding (magnitude 300, a dominant key: P = exp(S - max) / l = 1 / 1).
    A backward that keeps nothing of size N x N recomputes P = exp2(s - lse) from a second evaluation of the score, whose rounding
    does not cancel against the one inside lse (the dk/dv kernel scales k where the forward scales q)"""
    return c["N"] == 1 or saturated(c)


def recompute_allowance(c, dout_mag=1.0, setting="kernel"):
    """the `extra` of within_baseline for dq / dk / dv of ops.svtr_attention_bwd, relative to max|reference| -> dict.  Zero for an
    ordinary case run on the kernel's own forward: there the plain bound max(8 x fp32 baseline, 4 * 2^-24) holds alone.
    Two terms, each an absolute error of the exponent s - lse (base 2) of P = exp2(s - lse), so a relative error ln 2 * that of P:
    * setting "float64" (out and lse are the float64 forward ROUNDED to fp32 by the test): the test's own rounding of its inputs,
      2^-24 |lse_i| on the exponent of every key of query i (one sign for the whole row: it does not average out), and 2^-24
      sum_d |dO_id O_id| on D_i.  Every case.
    * baseline_exact_by_accident cases, either setting: the rounding of one fp32 evaluation of the score per (query, key), bounded
      from the case's own numbers in the kernels' order -- 16 steps, step t adding q'_t k_t + q'_(16+t) k_(16+t) (q' = scale log2e q)
      to the running sum with at most two roundings, so 2 * 2^-24 sum_t |running sum after t|, plus 2^-24 sum_d |q'_d k_d| for the
      rounding of q' (or of the scaled k) and 2^-24 |s| for the mask's multiply-add.  The kernel's forward setting counts it twice (the
      evaluation inside lse and the backward's) with 2 * 2^-24 |lse| for the stored lse and its log2; the float64 setting once.
    Carried to the gradients through the float64 P, dP and D:
    |d dv[j]| <= sum_i P_ij e_ij |dO_i|, |d dq[i]| <= scale sum_j (P_ij e_ij |dP_ij - D_i| + P_ij dD_i) |k_j|, dk likewise with |q_i|."""
    got = c.setdefault("_recompute", {})
    if (dout_mag, setting) in got:
        return got[(dout_mag, setting)]
    accident = baseline_exact_by_accident(c)
    if setting == "kernel" and not accident:
        got[(dout_mag, setting)] = dict(dq=0.0, dk=0.0, dv=0.0)
        return got[(dout_mag, setting)]
    u, log2e, ln2 = 2.0 ** -24, 1.4426950408889634, 0.6931471805599453
    B, N, h, d, scale = c["B"], c["N"], c["heads"], c["d"], c["scale"]
    q, k, v = (t.double() for t in c["qkv"].reshape(B, N, 3, h, d).permute(2, 0, 3, 1, 4))
    ref = c["refs"][dout_mag]
    S = (q @ k.transpose(-1, -2)) * scale
    if c["mask"] is not None:
        S = S + c["mask"].double()
    lse2 = (ref["lse"] * log2e).abs().unsqueeze(-1)                                  # [B, h, N, 1]
    P = torch.exp(S - ref["lse"].unsqueeze(-1))
    dO = c["douts"][dout_mag].double().reshape(B, N, h, d).permute(0, 2, 1, 3)
    O = ref["out"].reshape(B, N, h, d).permute(0, 2, 1, 3)
    e = torch.zeros_like(S)
    dD = torch.zeros_like(lse2)
    if setting == "float64":
        e = e + u * lse2
        dD = u * (dO * O).abs().sum(-1, keepdim=True)
    if accident:
        qs = q * (scale * log2e)
        half = d // 2
        steps = torch.einsum("bhit,bhjt->bhijt", qs[..., :half], k[..., :half]) + torch.einsum("bhit,bhjt->bhijt", qs[..., half:], k[..., half:])
        one = u * (2 * steps.cumsum(-1).abs().sum(-1) + qs.abs() @ k.abs().transpose(-1, -2) + torch.nan_to_num(S * log2e, neginf=0.0).abs())
        e = e + (2 * one + 2 * u * lse2 if setting == "kernel" else one)
    e = e * ln2
    W = P * e * (dO @ v.transpose(-1, -2) - (dO * O).sum(-1, keepdim=True)).abs() + P * dD
    sens = dict(dv=(P * e).transpose(-1, -2) @ dO.abs(), dq=(W @ k.abs()) * scale, dk=(W.transpose(-1, -2) @ q.abs()) * scale)
    out = {}
    for key, t in sens.items():
        m = float(ref[key].abs().max())
        out[key] = float(t.max()) / (m if m > 0 else 1.0)
    got[(dout_mag, setting)] = out
    return out


def grad_extra(c, key, dout_mag=1.0, setting="kernel"):
    """the derived `extra` of the recomputing backward kernels, relative to max|reference|: see the two allowances"""
    return recompute_allowance(c, dout_mag, setting)[key] + saturated_grad_allowance(c, key, dout_mag)


# the GEMM fallback of SvtrAttentionFn: head dimensions 16 and 64 never reach the fused kernels, 32 does unless they are switched off
FALLBACK_CASES = [(d, N, mk) for d in (16, 32, 64) for N in (33, 129) for mk in ("none", "additive")]


def fallback_case(d, N, mask_kind):
    return att_case(3 if N == 33 else 1, N, 2, mask_kind, "uniform", 1.5, d)


# ---------------------------------------------------------------------------------------------------------
# the kernels' view of a mask: 32-query waves, 32-key tiles, a tile skipped only when no query of the wave sees it
# ---------------------------------------------------------------------------------------------------------
def first_tile_blind_queries(mask):
    """the queries whose wave's first VISITED key tile shows them nothing (m_run stays -inf there: m_safe = 0, corr = exp2(-inf - 0))
    while a neighbour in the wave sees a key of it -> bool [N]"""
    N = mask.shape[0]
    vis = torch.isfinite(mask)
    blind = torch.zeros(N, dtype=torch.bool)
    for w0 in range(0, N, 32):
        wave = vis[w0:w0 + 32]
        for k0 in range(0, N, 32):
            sees = wave[:, k0:k0 + 32].any(1)
            if bool(sees.any()):                 # the first tile this wave does not skip
                blind[w0:w0 + 32] = ~sees
                break
    return blind


# ---------------------------------------------------------------------------------------------------------
# one block under autograd: (dim, heads, HW, mixer, qkv bias, DropPath, gamma kind)
# ---------------------------------------------------------------------------------------------------------
KEEP = 0.7
BLOCK_CASES = [
    (64, 2, (8, 25), "Local", False, True, "plain"),
    (128, 4, (4, 25), "Local", True, True, "plain"),
    (256, 8, (2, 25), "Global", True, True, "plain"),
    (64, 2, (3, 11), "Global", False, True, "plain"),            # N = 33: ragged in every kernel
    (128, 4, (4, 25), "Local", True, False, "plain"),            # no DropPath
    (64, 2, (3, 11), "Global", False, True, "loose"),            # one gamma1 entry 2^10 x the others: the LayerNorm bound is loose by 2^10
]
BLOCK_IDS = ["C%d-h%d-%dx%d-%s-%s-%s-%s" % (c[0], c[1], c[2][0], c[2][1], c[3], "bias" if c[4] else "nobias", "drop" if c[5] else "nodrop",
                                            c[6]) for c in BLOCK_CASES]
BLOCK_B = 3
LOOSE_CHANNEL = 5


def block_inputs(dim, heads, HW, mixer, qkv_bias, drop, gamma_kind):
    """x in +-1, Linear weights uniform in +-1 / sqrt(fan-in), biases +-0.3, gamma 1 +- 0.3 (one entry of gamma1 times 2^10 in the
    "loose" case), beta +-0.3; DropPath multipliers [0, 1/0.7, 1/0.7] on the attention branch and [1/0.7, 0, 1/0.7] on the Mlp's"""
    N = HW[0] * HW[1]

    def lin(n, k, seed, bias=True):
        return rnd(n, k, seed=seed) / k ** 0.5, (rnd(n, seed=seed + 1) * 0.3 if bias else None)

    p = {}
    p["norm1.weight"], p["norm1.bias"] = rnd(dim, seed=400) * 0.3 + 1.0, rnd(dim, seed=401) * 0.3
    if gamma_kind == "loose":
        p["norm1.weight"][LOOSE_CHANNEL] *= 1024.0
    p["mixer.qkv.weight"], p["mixer.qkv.bias"] = lin(3 * dim, dim, 402, qkv_bias)
    p["mixer.proj.weight"], p["mixer.proj.bias"] = lin(dim, dim, 404)
    p["norm2.weight"], p["norm2.bias"] = rnd(dim, seed=406) * 0.3 + 1.0, rnd(dim, seed=407) * 0.3
    p["mlp.fc1.weight"], p["mlp.fc1.bias"] = lin(4 * dim, dim, 408)
    p["mlp.fc2.weight"], p["mlp.fc2.bias"] = lin(dim, 4 * dim, 410)
    if gamma_kind == "loose":       # (the qkv weights of that one channel shrink with it: the scores stay where the other cases have them)
        p["mixer.qkv.weight"][:, LOOSE_CHANNEL] /= 1024.0
    x, dout = rnd(BLOCK_B, N, dim, seed=412), rnd(BLOCK_B, N, dim, seed=413)
    keep1 = torch.tensor([0.0, 1.0, 1.0]) if drop else None
    keep2 = torch.tensor([1.0, 0.0, 1.0]) if drop else None
    mask = local_attention_mask(HW[0], HW[1], 7, 11) if mixer == "Local" else None
    return x, p, keep1, keep2, mask, dout


def block_grad_names(p):
    return ["dx"] + ["d" + k for k in SVTR_BLOCK_PARAMS if p.get(k) is not None]


@functools.lru_cache(maxsize=None)
def block_case(dim, heads, HW, mixer, qkv_bias, drop, gamma_kind):
    """keep1 / keep2: the 0 / 1 DropPath draws as DropPath.forced_masks takes them; drop1 / drop2 = keep / 0.7 the multipliers.
    ref / base: float64 / fp32; x3[mode]: the x3 baselines ("fused": the default mode, "separate": TRAIN_OPERAND_FUSION off)"""
    x, p, keep1, keep2, mask, dout = block_inputs(dim, heads, HW, mixer, qkv_bias, drop, gamma_kind)
    d1 = None if keep1 is None else keep1 / KEEP
    d2 = None if keep2 is None else keep2 / KEEP
    ev = lambda **k: svtr_block_reference(x, p, d1, d2, mask, heads, dout, **k)
    return dict(dim=dim, heads=heads, HW=HW, N=HW[0] * HW[1], mixer=mixer, qkv_bias=qkv_bias, drop=drop, gamma_kind=gamma_kind, x=x,
                params=p, keep1=keep1, keep2=keep2, drop1=d1, drop2=d2, mask=mask, dout=dout, names=block_grad_names(p),
                ref=ev(dtype=torch.float64), base=ev(dtype=torch.float32),
                x3={m: ev(dtype=torch.float64, x3=m) for m in ("fused", "separate")})
