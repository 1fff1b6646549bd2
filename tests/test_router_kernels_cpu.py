"""The yardsticks and the inputs of tests/test_router_kernels_gpu.py, proven without a GPU.

1. Every written-out yardstick of tests/helpers.py for the DM-Router (layernorm_, colnorm_, gelu_, gelu_grad_, gate_tail_, fanin_ and
   dm_router_reference) equals torch float64 autograd of the plain ops; dm_router_reference equals oracle.mrn_oracle.dm_router_forward
   plus autograd for the output and all 17 gradients, at all four shapes.
2. The behaviour of torch that the GPU tests rely on (torch.max on a row of -inf and on a NaN, GELU at the infinities) and the
   properties of the crafted cases (exact ties, the saturated range, ragged class counts).
3. The inputs discriminate: on every shape of the GPU lists (tests/router_cases.py) a deliberately WRONG fp32 variant of the yardstick
   misses float64 by at least 10 x the bound the GPU test applies (helpers.baseline_bound: max(8 x the fp32 baseline's error,
   4 * 2^-24)).  Where a shape cannot tell a variant from the yardstick -- no lanes past Wd when Wd is a multiple of 256, no padding
   with one expert, no column past 1024, beta = 1, one sample, one expert -- the test asserts exactly that, so the blind shapes are
   written down here and checked, and the list names a shape of the same family that does discriminate."""
import pytest
import torch
import torch.nn.functional as F

from tests import router_cases as K
from tests.helpers import (DM_ROUTER_GRADS, DM_ROUTER_PARAMS, baseline_bound, colnorm_reference, dm_router_reference, fanin_reference,
                           gate_tail_reference, gelu_grad_reference, gelu_reference, layernorm_reference, rel_err)

MARGIN = 10.0
F32 = torch.float32


def close64(a, b, tol=1e-12):
    """float64 against float64: a few roundings of 2^-53, relative to max|b|"""
    return rel_err(a, b) <= tol


def miss(wrong, ref, base):
    """by how many times the bound a wrong result misses the reference (NaN: infinitely)"""
    err = rel_err(wrong, ref)
    return float("inf") if err != err else err / baseline_bound(ref, base)


# ---------------------------------------------------------------------------------------------------------
# 1. the yardsticks are what torch computes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.LN_KINDS)
@pytest.mark.parametrize("rows,C", [(1, 4), (5, 252), (65, 1024)])
def test_layernorm_reference_is_torch_layer_norm(rows, C, kind):
    c = K.ln_case(rows, C, kind, 1e-6)
    x, g, b = (c[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = F.layer_norm(x, (C,), g, b, eps=1e-6)
    y.backward(c["dy"].double())
    ref = c["ref"]
    tol = 1e-12 if kind != "offset" else 1e-9                # (x - mean loses 10 bits at an offset of 1000, in either evaluation)
    assert close64(ref["y"], y.detach(), tol) and close64(ref["dx"], x.grad, tol)
    assert close64(ref["dgamma"], g.grad, tol) and close64(ref["dbeta"], b.grad)
    assert close64(ref["mean"], x.detach().mean(1)) and close64(ref["rstd"], 1 / torch.sqrt(x.detach().var(1, unbiased=False) + 1e-6), tol)
    assert ref["y"].dtype == torch.float64 and c["base"]["dx"].dtype == F32
    if kind == "const":
        assert float(ref["rstd"][rows // 2]) == 1e-6 ** -0.5 and bool(torch.isfinite(ref["dx"]).all())


@pytest.mark.parametrize("P,Wd,B", K.COLNORM_SHAPES[:5])
def test_colnorm_reference_is_layer_norm_over_the_patch_axis(P, Wd, B):
    c = K.colnorm_case(P, Wd, B)
    x, g, b = (c[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = F.layer_norm(x.permute(0, 2, 1), (P,), g, b).permute(0, 2, 1)
    y.backward(c["dy"].double())
    ref = c["ref"]
    assert close64(ref["y"], y.detach()) and close64(ref["dbeta"], b.grad)
    assert ref["mean"].shape == (B, Wd) and ref["dgamma"].shape == (P,)
    if P == 1:                                    # xhat = 0: the yardstick's dx and dgamma are zero exactly, torch's a few 1e-14 of rounding
        assert not bool(ref["dx"].any()) and not bool(ref["dgamma"].any())
        assert float(x.grad.abs().max()) <= 1e-12 and float(g.grad.abs().max()) <= 1e-12
    else:
        assert close64(ref["dx"], x.grad) and close64(ref["dgamma"], g.grad)


def test_gelu_references_are_torch_gelu():
    a = K.ew_case(300, 512)["a"].double().requires_grad_(True)
    y = F.gelu(a)
    y.backward(torch.ones_like(a))
    assert close64(gelu_reference(a), y.detach()) and close64(gelu_grad_reference(a), a.grad)
    assert set(torch.tensor(K.EW_GRID).double().tolist()) <= set(a.detach().flatten().tolist()) and float(a.detach().abs().max()) == 40.0
    for rows, C in K.EW_SHAPES:
        c = K.ew_case(rows, C)
        want = c["a"].double() + c["b"].double() * c["d"].double().repeat_interleave(c["rows_per_d"]).view(-1, 1)
        assert torch.equal(K.ew_reference("residual", c["a"], c["b"], c["d"], c["rows_per_d"]), want) and bool((c["d"] == 0).any() or rows == 1)


@pytest.mark.parametrize("I,B,P,beta", [(1, 1, 1, 1.0), (2, 63, 31, 5.0), (8, 65, 129, 5.0), (8, 64, 1, 1.0)])
def test_gate_tail_reference_is_linear_squeeze_softmax(I, B, P, beta):
    c = K.gate_case(I, B, P, beta)
    r, Wr, br = c["r"].double().requires_grad_(True), c["Wr"].double().view(1, P).requires_grad_(True), c["br"].double().requires_grad_(True)
    s = F.linear(r.permute(0, 2, 1).contiguous(), Wr, br).squeeze(-1)                 # (modules/model.py: route over the patch axis)
    w = F.softmax(beta * s, -1)
    w.backward(c["dw"].double())
    ref = c["ref"]
    assert close64(ref["s"], s.detach()) and close64(ref["w"], w.detach()) and close64(ref["dr"], r.grad, 1e-11)
    assert close64(ref["dWr"], Wr.grad.view(-1), 1e-10)
    assert float(ref["dbr"].abs()) <= 1e-12 and float(br.grad.abs()) <= 1e-12          # the softmax gradient sums to zero: dbr is all rounding
    assert torch.equal(ref["argmax"], s.detach().argmax(1))


@pytest.mark.parametrize("I,C,B,T", [(1, 5, 1, 1), (3, 1025, 5, 26), (8, 5, 5, 26), (8, 5374, 1, 1)])
def test_fanin_reference_is_the_oracle_fanin(I, C, B, T):
    from oracle import mrn_oracle as O
    from tests.helpers import oracle_dtype
    c = K.fanin_case(I, K.fanin_classes(I, C), B, T)
    with oracle_dtype(torch.float64):
        w = c["w"].double().requires_grad_(True)
        out = O.fanin([l.double() for l in c["logits"]], w)
        out.backward(c["dout"].double())
        sel = O.select_expert([l.double() for l in c["logits"]], c["index"])
    assert close64(c["ref"][0], out.detach()) and close64(c["ref"][1], w.grad)
    assert torch.equal(K.select_reference(c["logits"], c["index"]).double(), sel)
    assert bool((K.select_reference(c["logits"], torch.full((B,), I)) == 1).all())


ORACLE_KEYS = ("norm.weight", "norm.bias", "proj_1.weight", "proj_1.bias", "spatial_gating.norm.weight", "spatial_gating.norm.bias",
               "spatial_gating.proj.weight", "spatial_gating.proj.bias", "proj_2.weight", "proj_2.bias", "channel_gating.norm.weight",
               "channel_gating.norm.bias", "channel_gating.proj.weight", "channel_gating.proj.bias", "proj_3.weight", "proj_3.bias")


@pytest.mark.parametrize("B,P,I,C", K.DM_SHAPES)
def test_dm_router_reference_is_the_oracle_and_its_autograd(B, P, I, C):
    """the output and all 17 gradients; the oracle works on the reference layout [B, I, P, C], the yardstick on DMRouterFn's [B, P, I, C]"""
    from oracle import mrn_oracle as O
    c = K.dm_case(B, P, I, C)
    sd = {"r." + n: p.double().requires_grad_(True) for n, p in zip(ORACLE_KEYS, c["params"])}
    x = c["x"].double().permute(0, 2, 1, 3).contiguous().requires_grad_(True)
    out = O.dm_router_forward(sd, "r.", x)
    out.backward(c["dout"].double().permute(0, 2, 1, 3))
    ref_out, ref_g = c["ref"]
    assert len(ref_g) == 17 and tuple(ref_g) != () and set(ref_g) == set(DM_ROUTER_GRADS)
    assert close64(ref_out, out.detach().permute(0, 2, 1, 3)) and close64(ref_g["dx"], x.grad.permute(0, 2, 1, 3), 1e-11)
    for k, n in zip(DM_ROUTER_PARAMS, ORACLE_KEYS):
        assert ref_g["d" + k].shape == sd["r." + n].shape and close64(ref_g["d" + k], sd["r." + n].grad, 1e-11), k
    assert c["base"][0].dtype == F32 and all(v.dtype == F32 for v in c["base"][1].values())


# ---------------------------------------------------------------------------------------------------------
# 2. torch's edge behaviour and the crafted cases
# ---------------------------------------------------------------------------------------------------------
def test_torch_max_on_rows_of_minus_infinity_and_on_nan():
    x = torch.full((2, 70), float("-inf"))
    assert torch.max(x, 1).indices.tolist() == [0, 0]
    x = K.rnd(3, 70, seed=1)
    x[1, 41] = float("nan")
    x[2, 69] = float("nan")
    assert torch.max(x, 1).indices.tolist()[1:] == [41, 69] and bool(torch.isnan(torch.softmax(x, 1).max(1).values[1:]).all())
    for C in K.ARGMAX_C:
        for rows in K.ARGMAX_ROWS:
            plain, tie, nan, ninf = (K.argmax_case(rows, C, v) for v in K.ARGMAX_VARIANTS)
            assert bool(torch.isnan(nan["x"]).sum(1).eq(1).all()) and bool(torch.isnan(nan["x"][torch.arange(rows), nan["idx"]]).all())
            assert int(ninf["idx"][rows // 2]) == 0 and bool(torch.isnan(ninf["prob"][rows // 2]))
            if C >= 2:
                top = tie["x"] == tie["x"].max(1, keepdim=True).values
                assert bool(top.sum(1).eq(2).all()) and torch.equal(tie["idx"], top.int().argmax(1))
                second = top.int().flip(1).argmax(1).mul(-1).add(C - 1)
                assert bool(((second - tie["idx"]) % 64 != 0).all())                   # the two maxima stand in different lanes
            assert not bool(torch.isnan(plain["prob"]).any())


def test_gelu_at_the_infinities_is_what_the_formula_gives():
    a = torch.tensor(K.EW_SPECIALS, dtype=torch.float64)
    y = F.gelu(a)
    assert float(y[0]) == float("inf") and bool(torch.isnan(y[1:3]).all())             # -inf * (1 + erf(-inf)) = -inf * 0
    assert torch.equal(torch.isnan(gelu_reference(a)), torch.isnan(y))


def test_the_crafted_gate_cases():
    c = K.saturated_gate_case()
    top = float((c["beta"] * c["ref"]["s"]).abs().max())
    assert 150 <= top <= 250, top
    assert float((c["base"]["w"] == 0).float().mean()) > 0.25 and bool(torch.isfinite(c["ref"]["dr"]).all())
    assert miss(dr_without_beta(c), c["ref"]["dr"], c["base"]["dr"]) >= MARGIN
    for I in (2, 8):
        for B in K.GATE_B:
            for P in K.GATE_P:
                t = K.tie_case(I, B, P)
                for dtype in (torch.float64, F32):
                    g = gate_tail_reference(t["r"], t["Wr"], t["br"], 1.0, dtype=dtype)
                    top = g["s"] == g["s"].max(1, keepdim=True).values
                    assert bool(top.sum(1).eq(2).all()) and torch.equal(g["argmax"], t["want"])
                assert len(set(t["want"].tolist())) == min(B, I - 1)


def test_fanin_class_counts_are_ragged():
    for I in K.FANIN_I:
        for C in K.FANIN_NEWEST:
            cls = K.fanin_classes(I, C)
            assert len(cls) == I and cls[-1] == C and list(cls) == sorted(cls) and all(c % 4 for c in cls[:-1]) and cls[0] >= 1
    assert K.FANIN_BIG[2] * K.FANIN_BIG[3] == 65536


# ---------------------------------------------------------------------------------------------------------
# 3. the inputs discriminate
# ---------------------------------------------------------------------------------------------------------
def ln_blocks(rows):
    """the backward's partition (mrn_layernorm_bwd_blocks): min(1024, ceil(rows / 64)) blocks of ceil(rows / blocks) rows"""
    nblk = max(1, min(1024, (rows + 63) // 64))
    per = (rows + nblk - 1) // nblk
    return nblk, per


@pytest.mark.parametrize("rows,C", K.LN_SHAPES)
def test_wrong_layernorms_miss_the_bound(rows, C):
    """a one-pass variance E[x^2] - mean^2 (on the rows offset by 1000, at every shape that runs on them: all but the two of
    65537 rows); dx without its xhat term; dgamma / dbeta without the last block's rows"""
    c = K.ln_case(rows, C)
    ref, base = c["ref"], c["base"]
    x, gamma, dy = c["x"], c["gamma"], c["dy"]
    mean = x.mean(1, keepdim=True)

    def one_pass(x):
        mean = x.mean(1, keepdim=True)
        return 1 / torch.sqrt((x * x).mean(1, keepdim=True) - mean * mean + c["eps"])
    if rows != K.LN_BIG_ROWS:
        for eps in K.LN_EPS:
            o = K.ln_case(rows, C, "offset", eps)
            xo = o["x"]
            rstd = one_pass(xo)
            y = (xo - xo.mean(1, keepdim=True)) * rstd * o["gamma"] + o["beta"]
            assert miss(rstd.squeeze(1), o["ref"]["rstd"], o["base"]["rstd"]) >= MARGIN and miss(y, o["ref"]["y"], o["base"]["y"]) >= MARGIN
    rstd = base["rstd"].unsqueeze(1)
    xhat, g = (x - mean) * rstd, dy * gamma
    assert miss(rstd * (g - g.mean(1, keepdim=True)), ref["dx"], base["dx"]) >= MARGIN
    nblk, per = ln_blocks(rows)
    last = (rows - 1) // per * per                               # first row of the last block that owns rows
    assert miss((dy * xhat)[:last].sum(0), ref["dgamma"], base["dgamma"]) >= MARGIN
    assert miss(dy[:last].sum(0), ref["dbeta"], base["dbeta"]) >= MARGIN
    if rows == K.LN_BIG_ROWS:
        assert (nblk, per, last) == (1024, 65, 65520)


@pytest.mark.parametrize("P,Wd,B", K.COLNORM_SHAPES)
def test_colnorm_partials_that_count_idle_lanes_miss_the_bound(P, Wd, B):
    """colnorm_bwd_kernel's lanes past Wd address column 0 of their sample; counted, they add its terms once per idle lane.  Blind where
    Wd is a multiple of 256 (256, 4096: no idle lane; 255 and 257 stand next to them) and at P = 1 for dgamma (xhat = 0)"""
    c = K.colnorm_case(P, Wd, B)
    ref, base = c["ref"], c["base"]
    idle = (Wd + 255) // 256 * 256 - Wd
    x, dy = c["x"], c["dy"]
    xhat = (x - base["mean"].unsqueeze(1)) * base["rstd"].unsqueeze(1)
    dgamma = base["dgamma"] + idle * (dy * xhat)[:, :, 0].sum(0)
    dbeta = base["dbeta"] + idle * dy[:, :, 0].sum(0)
    if idle == 0:
        assert torch.equal(dgamma, base["dgamma"]) and torch.equal(dbeta, base["dbeta"])
    else:
        assert miss(dbeta, ref["dbeta"], base["dbeta"]) >= MARGIN
        assert P == 1 or miss(dgamma, ref["dgamma"], base["dgamma"]) >= MARGIN
    assert {s[1] % 256 for s in K.COLNORM_SHAPES} >= {0, 255, 1, 4}


@pytest.mark.parametrize("rows,C", K.EW_SHAPES)
def test_tanh_gelu_misses_the_bound(rows, C):
    c = K.ew_case(rows, C)
    a = c["a"]
    ref, base = K.ew_reference("gelu", a), K.ew_reference("gelu", a, dtype=F32)
    assert miss(F.gelu(a, approximate="tanh"), ref, base) >= MARGIN
    a64 = a.double().requires_grad_(True)
    F.gelu(a64, approximate="tanh").backward(c["b"].double())
    assert miss(a64.grad.float(), K.ew_reference("gelu_bwd", a, c["b"]), K.ew_reference("gelu_bwd", a, c["b"], dtype=F32)) >= MARGIN


@pytest.mark.parametrize("I,C,B,T", K.FANIN_SHAPES + [(K.FANIN_BIG[0], K.FANIN_BIG[1][-1], *K.FANIN_BIG[2:])])
def test_wrong_fanins_miss_the_bound(I, C, B, T):
    """padding with zeros instead of ones (blind with one expert: nothing is padded; I = 3 and 8 are not); a backward that stops at
    column 1024 (blind up to 1024 classes; 1025 and 5374 are not)"""
    classes = K.FANIN_BIG[1] if B * T == 65536 else K.fanin_classes(I, C)
    c = K.fanin_case(I, classes, B, T)
    (ref_out, ref_dw), (base_out, base_dw) = c["ref"], c["base"]
    zeros = [torch.cat([l, torch.zeros(B, T, C - l.shape[-1])], -1) for l in c["logits"]]
    out = sum(c["w"][:, i].view(-1, 1, 1) * p for i, p in enumerate(zeros))
    dw = torch.stack([(c["dout"] * p).sum((1, 2)) for p in zeros], 1)
    if I == 1:
        assert torch.equal(out, base_out)
    else:
        assert miss(out, ref_out, base_out) >= MARGIN and miss(dw, ref_dw, base_dw) >= MARGIN
    short = fanin_reference([l[..., :1024] for l in c["logits"]], c["w"], c["dout"][..., :1024], dtype=F32)[1]
    if C > 1024:
        assert miss(short, ref_dw, base_dw) >= MARGIN
    else:
        assert rel_err(short, ref_dw) <= baseline_bound(ref_dw, base_dw)


def dr_without_beta(c):
    w, dw = c["base"]["w"], c["dw"]
    ds = w * (dw - (dw * w).sum(1, keepdim=True))
    return c["Wr"].view(1, -1, 1) * ds.unsqueeze(1)


@pytest.mark.parametrize("I,B,P,beta", K.GATE_SHAPES)
def test_gate_tail_without_beta_misses_the_bound(I, B, P, beta):
    """ds = w (dw - sum dw w) without the factor beta: blind at beta = 1 and with one expert (ds = 0); every shape also runs at beta = 5"""
    c = K.gate_case(I, B, P, beta)
    ref, base = c["ref"], c["base"]
    dr = dr_without_beta(c)
    if beta == 1.0 or I == 1:
        assert rel_err(dr, ref["dr"]) <= baseline_bound(ref["dr"], base["dr"])
    else:
        assert miss(dr, ref["dr"], base["dr"]) >= MARGIN
    assert all((i, b, p, 5.0) in K.GATE_SHAPES for i, b, p, _ in K.GATE_SHAPES)


@pytest.mark.parametrize("B,P,I,C", K.DM_SHAPES)
def test_wrong_routers_miss_the_bound(B, P, I, C):
    """dbsp summed over the wrong axis (the [B * N] row sums read as [N, B]: blind with one sample; B = 3 and 2 are not); the token
    permutation applied to the rows of the spatial weight only (blind with one expert, where it is the identity; I = 2, 3, 8 are not)"""
    c = K.dm_case(B, P, I, C)
    ref_out, ref_g = c["ref"]
    base_out, base_g = c["base"]
    N = P * I
    stages = {}
    dm_router_reference(c["x"], c["params"], c["dout"], dtype=F32, stages=stages)
    perm, inv = K.token_perm(P, I)
    rowsum = stages["dvp_r"][:, perm.long()].sum(2)                                    # [B, N] in DMRouterFn's token order
    wrong = rowsum.reshape(N, B).sum(1)[inv.long()]
    if B == 1:
        assert torch.equal(wrong, rowsum.sum(0)[inv.long()]) and rel_err(wrong, ref_g["dbsp"]) <= baseline_bound(ref_g["dbsp"], base_g["dbsp"])
    else:
        assert miss(wrong, ref_g["dbsp"], base_g["dbsp"]) >= MARGIN
    params = list(c["params"])
    params[6] = params[6][:, inv.long()]                                               # Wsp[perm][:, :] where Wsp[perm][:, perm] belongs
    out, g = dm_router_reference(c["x"], params, c["dout"], dtype=F32)
    if I == 1:
        assert torch.equal(out, base_out)
    else:
        assert miss(out, ref_out, base_out) >= MARGIN
        for k in ("dx", "dw1", "dsn_w", "dbsp", "dw2"):
            assert miss(g[k], ref_g[k], base_g[k]) >= MARGIN, k
    assert {s[0] for s in K.DM_SHAPES} >= {1, 2, 3} and {s[2] for s in K.DM_SHAPES} >= {1, 2, 3, 8}
