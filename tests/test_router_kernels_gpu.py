"""The DM-Router's kernels and all its gradients, called directly and compared with float64.

rowops.hip (LayerNorm over the last dim and over the patch axis, GELU and the gating products, gather2d, argmax), router.hip (gate
tail, fan-in, select-expert), the two strided gemm_raw forms of the spatial projection, and functional.DMRouterFn end to end with all
17 gradients.  The router is the only thing loop B trains, and until now 12 of those gradients were asserted nowhere below a
whole-model test; the direct kernel tests ran one shape each against fp32 torch.

Conventions (tests/test_block_backward_gpu.py's, tests/test_loss_optim_gpu.py's): fp32 inputs made on the CPU (tests/router_cases.py);
the float64 reference is the written-out yardstick of tests/helpers.py, proven against torch autograd and the oracle in
test_router_kernels_cpu.py, and the fp32 baseline the same yardstick in float32; the kernel must stay within max(8 x the baseline's
error, 4 * 2^-24) relative to max|reference| (helpers.within_baseline, which prints the ratio).  test_router_kernels_cpu.py also proves
that on the shapes below a wrong kernel -- a one-pass variance, dx without its xhat term, dgamma without the last block's rows,
partials that count idle lanes, tanh-GELU, zero padding in the fan-in, a backward that stops at column 1024, ... -- would miss that
bound by a factor of 10 at least.  Strided or padded operands carry a sentinel around them, which must be bit-identical afterwards.

Two defects were fixed with this file.  fanin_fwd_kernel and select_expert_kernel rode their rows on grid.y, which a launch limits
to 65535: 256 samples x 256 steps is one more (test_fanin_65536_rows; the rows are on grid.x now, as fanin_bwd_kernel's always were).
argmax_kernel and argmax_prob_kernel answered 0x7fffffff for a row of nothing but -inf, where torch.max answers 0 and the caller
looks the index up in a character table (test_argmax).

Measured on an MI355X, the largest ratio of a kernel's error to the fp32 baseline's ("ratio" is what within_baseline prints: kernel
error / max(baseline error, 2^-24 / 2)), over all shapes of a family: LayerNorm 3.29 (mean, 3 x 252), column norm 2.92 (dbeta, P = 2,
Wd = 257), elementwise 1.01, the spatial gemm_raw forms 2.37, fan-in 4.73 (dw at 65536 rows), argmax probability 1.16.  The gate
tail: gate_tail_fwd_kernel added a score's P products one after the other in plain fp32 and missed the plain bound on a single score
(B = I = 1, P = 129: kernel 5.0e-7, ratio 16.9); its sum is compensated now (ratio at most 0.99, kernel at most 5.0e-8).  dWr at P = 1 is ONE sum of B I numbers
(ratio 31.4 at B I = 512, kernel 9.4e-7, where torch's pairwise fp32 sum happens to land within 1e-8 of float64): there, and only
there, and to dbr, which is one number always, one_sum_allowance applies.  dbr is also run on weights that are no softmax, where it is
not zero in exact arithmetic (run_gate).  DMRouterFn: the table in
test_dm_router_all_gradients_against_float64."""
import pytest
import torch
import torch.nn.functional as F

from tests import router_cases as K
from tests.helpers import DM_ROUTER_GRADS, DM_ROUTER_PARAMS, within_baseline

pytestmark = pytest.mark.gpu

SENTINEL = 7.0e30                   # finite (a kernel that READ it would show it in every sum) and far from any result


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def cu(t):
    return t.cuda()


def bits(t):
    """the tensor's bit patterns: equality that tells -0.0 from +0.0 and holds for NaN"""
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def framed(t, left=None, right=4, fill=SENTINEL):
    """t [rows, C] (CPU, or None for an output) inside a GPU buffer with `left` (default C: the right half of a [rows, 2C] buffer, as
    chunk() gives it) sentinel columns before and `right` after -> (buffer, view).  Kernels with 16-byte loads need left and the row
    stride to be multiples of 4."""
    rows, C = t.shape
    left = C if left is None else left
    buf = torch.full((rows, left + C + right), fill, device="cuda", dtype=torch.float32)
    view = buf[:, left:left + C]
    view.copy_(t)
    return buf, view


def frame_untouched(buf, left, C):
    frame = torch.cat([buf[:, :left], buf[:, left + C:]], 1)
    return bool((bits(frame) == bits(torch.full_like(frame, SENTINEL))).all())


def padded(t, fill=SENTINEL):
    """t [B, T, C] (CPU) in a GPU buffer whose rows are padded to the next multiple of 4 floats plus 4 -> (buffer, view [..., :C])"""
    C = t.shape[-1]
    ld = (C + 3) // 4 * 4 + 4
    wide = torch.full((*t.shape[:-1], ld), fill, device="cuda", dtype=torch.float32)
    wide[..., :C] = cu(t)
    return wide, wide[..., :C]


def padding_untouched(wide, first):
    pad = wide[..., first:]
    return bool((bits(pad) == bits(torch.full_like(pad, SENTINEL))).all())


# ---------------------------------------------------------------------------------------------------------
# 1. LayerNorm over the last dim
# ---------------------------------------------------------------------------------------------------------
def run_layernorm(ops, c, forms):
    """forward and backward on a case with x the right half of a [rows, 2C] buffer and dx written into the right half of a
    sentinel-filled one; forms: also accumulate=True onto preloaded values and grad_acc onto a preloaded, guarded [2C] vector"""
    rows, C, eps = c["rows"], c["C"], c["eps"]
    name = f"layernorm {rows}x{C} {c['kind']} eps {eps:g}"
    ref, base = c["ref"], c["base"]
    xbuf, x = framed(c["x"])
    gamma, beta, dy = cu(c["gamma"]), cu(c["beta"]), cu(c["dy"])
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, eps)
    dxbuf, dxv = framed(torch.zeros(rows, C))
    dxv.fill_(SENTINEL)
    dx, dg, db = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx=dxv)
    torch.cuda.synchronize()
    assert dx.data_ptr() == dxv.data_ptr() and frame_untouched(dxbuf, C, C) and frame_untouched(xbuf, C, C)
    assert same_bits(x, cu(c["x"]))
    for k, got in (("y", y), ("mean", mean), ("rstd", rstd), ("dx", dx), ("dgamma", dg), ("dbeta", db)):
        assert bool(torch.isfinite(got).all()), (name, k)
        within_baseline(f"{name} {k}", got, ref[k], base[k])
    if not forms:
        return
    dx0 = K.rnd(rows, C, seed=109)
    accbuf, acc = framed(dx0)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx=acc, accumulate=True)
    pre = K.rnd(2 * C, seed=105)
    gbuf = torch.full((4 + 2 * C + 4,), SENTINEL, device="cuda")
    gacc = gbuf[4:4 + 2 * C]
    gacc.copy_(pre)
    got = ops.layernorm_bwd(dy, x, gamma, mean, rstd, grad_acc=gacc)
    torch.cuda.synchronize()
    assert got[1] is None and got[2] is None and frame_untouched(accbuf, C, C)
    within_baseline(f"{name} dx accumulated", acc, ref["dx"] + dx0.double(), base["dx"] + dx0)
    within_baseline(f"{name} dx (grad_acc call)", got[0], ref["dx"], base["dx"])
    guards = torch.cat([gbuf[:4], gbuf[4 + 2 * C:]])
    assert bool((bits(guards) == bits(torch.full_like(guards, SENTINEL))).all())
    want = torch.cat([ref["dgamma"], ref["dbeta"]]) + pre.double()
    within_baseline(f"{name} grad_acc", gacc, want, torch.cat([base["dgamma"], base["dbeta"]]) + pre)


@pytest.mark.parametrize("C", K.LN_C)
def test_layernorm_against_float64(ops, C):
    """ops.layernorm_fwd / layernorm_bwd at rows 1, 3, 5, 65 x three inputs (unit range; every row offset by 1000, which only a
    two-pass variance survives; one constant row: rstd = 1 / sqrt(eps), dx finite) x eps 1e-5, 1e-6, on strided x and dx; the
    accumulate and grad_acc forms once per row count.  C = 4: 63 lanes idle; 252 / 256 / 260: around one float4 per lane; 512,
    1024: two and four trips."""
    for rows in K.LN_ROWS:
        for kind in K.LN_KINDS:
            for eps in K.LN_EPS:
                run_layernorm(ops, K.ln_case(rows, C, kind, eps), forms=(kind == "unit" and eps == 1e-5))


@pytest.mark.parametrize("C", K.LN_BIG_C)
def test_layernorm_backward_block_cap(ops, C):
    """65537 rows: mrn_layernorm_bwd_blocks stops at 1024 blocks, each walks 65 rows, blocks 1009 .. 1023 own none and must still
    write ZERO partials into the uninitialised buffer (the column sum over all 1024 reads them).  The entry point is also called
    with a sentinel-filled partial buffer: the empty blocks' partials are zero bits afterwards."""
    from mrn_amd._lib import call
    c = K.ln_case(K.LN_BIG_ROWS, C)
    run_layernorm(ops, c, forms=True)
    rows = c["rows"]
    x, gamma, beta, dy = cu(c["x"]), cu(c["gamma"]), cu(c["beta"]), cu(c["dy"])
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, c["eps"])
    nblk = call("mrn_layernorm_bwd_blocks", rows)
    assert nblk == 1024
    per = (rows + nblk - 1) // nblk
    first_empty = (rows + per - 1) // per
    assert per == 65 and first_empty == 1009
    part = torch.full((nblk, 2 * C), SENTINEL, device="cuda")
    dx = torch.empty(rows, C, device="cuda")
    call("mrn_layernorm_bwd_f32", dy.data_ptr(), C, x.data_ptr(), C, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
         C, 0, part.data_ptr(), rows, C, stream())
    torch.cuda.synchronize()
    assert bool((bits(part[first_empty:]) == 0).all())
    assert not bool((part[:first_empty] == SENTINEL).any())
    within_baseline(f"layernorm {rows}x{C} partials summed", part.double().sum(0).cpu(), torch.cat([c["ref"]["dgamma"], c["ref"]["dbeta"]]),
                    torch.cat([c["base"]["dgamma"], c["base"]["dbeta"]]))


@pytest.mark.parametrize("C", K.LN_HL_C)
def test_layernorm_operand_form_is_the_plain_kernel(ops, C):
    """ops.layernorm_fwd_operand (the HL32 form) returns the plain kernel's y, mean and rstd, bit for bit"""
    for rows in (5, 65):
        c = K.ln_case(rows, C)
        x, gamma, beta = cu(c["x"]), cu(c["gamma"]), cu(c["beta"])
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
        y2, mean2, rstd2, hl, sc = ops.layernorm_fwd_operand(x, gamma, beta)
        torch.cuda.synchronize()
        assert same_bits(y, y2) and same_bits(mean, mean2) and same_bits(rstd, rstd2)
        assert hl.numel() == rows * C * 4 and float(sc[0]) * float(sc[1]) == 1.0


@pytest.mark.parametrize("C", [1028, 6])
def test_layernorm_refuses_widths_it_cannot_hold(ops, C):
    """more than four float4 per lane, or no whole float4s: an error that names the entry point, and nothing is launched"""
    x = cu(K.rnd(3, C, seed=106))
    out = torch.full((3, C), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="mrn_layernorm_fwd_f32"):
        ops.layernorm_fwd(x, cu(torch.ones(C)), cu(torch.zeros(C)), out=out)
    torch.cuda.synchronize()
    assert same_bits(out, torch.full_like(out, SENTINEL))


# ---------------------------------------------------------------------------------------------------------
# 2. column norm
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Wd,B", K.COLNORM_SHAPES)
def test_colnorm_against_float64(ops, P, Wd, B):
    """ops.colnorm_fwd / colnorm_bwd(accumulate=True) onto preloaded dx, as DMRouterFn.backward calls it.  Wd = 4, 255, 257: the last
    block is ragged and its idle lanes must add nothing to the partials; P = 1: xhat = 0, so dx and dgamma are zero exactly."""
    c = K.colnorm_case(P, Wd, B)
    name = f"colnorm P {P} Wd {Wd} B {B}"
    ref, base = c["ref"], c["base"]
    x, dy, gamma, beta = cu(c["x"]), cu(c["dy"]), cu(c["gamma"]), cu(c["beta"])
    y, mean, rstd = ops.colnorm_fwd(x, gamma, beta, c["eps"])
    dx = cu(c["dx0"]).clone()
    got, dg, db = ops.colnorm_bwd(dy, x, gamma, mean, rstd, dx=dx, accumulate=True)
    torch.cuda.synchronize()
    assert got.data_ptr() == dx.data_ptr()
    for k, g in (("y", y), ("mean", mean), ("rstd", rstd), ("dgamma", dg), ("dbeta", db)):
        within_baseline(f"{name} {k}", g, ref[k], base[k])
    within_baseline(f"{name} dx accumulated", dx, ref["dx"] + c["dx0"].double(), base["dx"] + c["dx0"])
    if P == 1:
        assert same_bits(dx, cu(c["dx0"])) and not bool(dg.any())
    plain, dg2, db2 = ops.colnorm_bwd(dy, x, gamma, mean, rstd)
    within_baseline(f"{name} dx", plain, ref["dx"], base["dx"])
    assert same_bits(dg, dg2) and same_bits(db, db2)


# ---------------------------------------------------------------------------------------------------------
# 3. elementwise
# ---------------------------------------------------------------------------------------------------------
def run_elementwise(ops, a, b, d, per):
    """-> {name: result} of every elementwise entry point on contiguous operands"""
    return {
        "gelu": ops.ew_rows(ops.EW_GELU, a),
        "gelu_bwd": ops.ew_rows(ops.EW_GELU_BWD, a, b),
        "mul": ops.ew_rows(ops.EW_MUL, a, b),
        "residual": ops.residual_scale_rows(a, b, d, per),
        "operand gelu": ops.ew_operand(ops.EW_GELU, a)[0],
        "operand gelu_bwd": ops.ew_operand(ops.EW_GELU_BWD, a, b)[0],
        "operand add": ops.ew_operand(ops.EW_ADD, a, b)[0],
        "operand residual": ops.ew_operand(ops.EW_RESIDUAL_SCALE, a, b, drop=d, rows_per_drop=per)[0],
    }


@pytest.mark.parametrize("rows,C", K.EW_SHAPES)
def test_elementwise_against_float64(ops, rows, C):
    """EW_GELU, EW_GELU_BWD, EW_MUL (ops.ew_rows), ops.residual_scale_rows and ops.ew_operand's ops 0 / 1 / 3 / 8 on a value grid
    (+-0, +-1e-30, +-1e-3, +-1, +-6, +-40) followed by uniform values in +-3; ew_rows also on column slices of wider sentinel-filled
    buffers, in and out.  Every launch walks the grid-stride loop (1024 float4 per 256-thread block)."""
    c = K.ew_case(rows, C)
    a, b, d, per = cu(c["a"]), cu(c["b"]), cu(c["d"]), c["rows_per_d"]
    got = run_elementwise(ops, a, b, d, per)
    torch.cuda.synchronize()
    for k, g in got.items():
        op = k.replace("operand ", "")
        args = (c["a"], c["b"], c["d"], per)
        within_baseline(f"ew {rows}x{C} {k}", g, K.ew_reference(op, *args), K.ew_reference(op, *args, dtype=torch.float32))
    assert same_bits(got["gelu"], got["operand gelu"]) and same_bits(got["gelu_bwd"], got["operand gelu_bwd"])
    assert same_bits(got["residual"], got["operand residual"])
    abuf, av = framed(c["a"], left=4)
    bbuf, bv = framed(c["b"], left=8)
    for op, name in ((ops.EW_GELU, "gelu"), (ops.EW_GELU_BWD, "gelu_bwd"), (ops.EW_MUL, "mul")):
        obuf, ov = framed(torch.zeros(rows, C), left=12, right=8)
        ov.fill_(SENTINEL)
        ops.ew_rows(op, av, None if name == "gelu" else bv, out=ov)
        torch.cuda.synchronize()
        assert same_bits(ov, got[name]), name                      # the strided form computes what the contiguous one does
        assert frame_untouched(obuf, 12, C) and frame_untouched(abuf, 4, C) and frame_untouched(bbuf, 8, C)


def test_elementwise_non_finite_values(ops):
    """+inf, -inf and NaN: the same class (NaN / +inf / -inf / finite value) as torch's float64 result cast to fp32"""
    a64 = torch.tensor([K.EW_SPECIALS], dtype=torch.float64, requires_grad=True)
    b64 = torch.tensor([[1.0, -2.0, 1.0, 0.5]], dtype=torch.float64)
    gelu = F.gelu(a64)
    gelu.backward(b64)
    d64 = torch.tensor([0.5], dtype=torch.float64)
    want = {"gelu": gelu.detach(), "gelu_bwd": a64.grad, "mul": a64.detach() * b64, "residual": a64.detach() + b64 * d64,
            "operand add": a64.detach() + b64}
    a, b, d = cu(a64.detach().float()), cu(b64.float()), cu(d64.float())
    got = run_elementwise(ops, a, b, d, 1)
    torch.cuda.synchronize()
    for k, g in got.items():
        w = want[k.replace("operand ", "")] if k != "operand add" else want[k]
        w, g = w.float(), g.cpu()
        print(f"ew specials {k}: kernel {g.tolist()} torch {w.tolist()}")
        assert torch.equal(torch.isnan(g), torch.isnan(w)), k
        fin = torch.isfinite(w)
        assert torch.equal(g[~fin & ~torch.isnan(w)], w[~fin & ~torch.isnan(w)]), k             # the infinities, with their signs


# ---------------------------------------------------------------------------------------------------------
# 4. gather2d and the spatial projection
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,I", K.PERM_SHAPES)
def test_gather2d_token_permutation(ops, P, I):
    """ops.gather2d with functional.token_permutation, as DMRouterFn permutes the spatial weight: exact, the padding columns of the
    [N, ldw] buffer zero, the inverse permutation restores the input bit for bit, a null index is the identity"""
    from mrn_amd.functional import token_permutation
    N = P * I
    ldw = (N + 3) // 4 * 4
    perm, inv = token_permutation(P, I, "cuda")
    cperm, cinv = K.token_perm(P, I)
    assert torch.equal(perm.cpu(), cperm) and torch.equal(inv.cpu(), cinv) and perm.dtype == torch.int32
    w = K.rnd(N, N, seed=134)
    wd = cu(w)
    wp = ops.gather2d(wd, perm, perm, ld_out=ldw)
    whole = wp.as_strided((N, ldw), (ldw, 1))
    back = ops.gather2d(wp, inv, inv)
    torch.cuda.synchronize()
    assert wp.stride(0) == ldw and same_bits(wp, cu(w[cperm.long()][:, cperm.long()]))
    assert bool((bits(whole[:, N:]) == 0).all())
    assert same_bits(back, wd)
    assert same_bits(ops.gather2d(wd, None, None), wd)
    assert same_bits(ops.gather2d(wd, perm, None), cu(w[cperm.long()]))
    assert same_bits(ops.gather2d(wd, None, perm, ld_out=ldw), cu(w[:, cperm.long()]))
    bias = K.rnd(N, seed=135)
    assert same_bits(ops.gather2d(cu(bias).view(1, N), None, perm).view(N), cu(bias[cperm.long()]))


@pytest.mark.parametrize("C", K.SPATIAL_C)
@pytest.mark.parametrize("B", K.SPATIAL_B)
@pytest.mark.parametrize("P,I", K.PERM_SHAPES)
def test_spatial_projection_gemm_forms(ops, P, I, B, C):
    """the two strided gemm_raw forms of DMRouterFn's spatial gate: vp[b] = Wsp' vn[b] + bsp'[:, None] (A at batch stride 0 and row
    stride ldw, bias along the rows) and dvn[b] = Wsp'^T dvp[b] (A read transposed: strides (0, 1, ldw))"""
    c = K.spatial_case(P, I, B, C)
    N = c["N"]
    ldw = (N + 3) // 4 * 4
    perm = cu(c["perm"])
    wsp_p = ops.gather2d(cu(c["wsp"]), perm, perm, ld_out=ldw)
    bsp_p = ops.gather2d(cu(c["bsp"]).view(1, N), None, perm).view(N)
    vn, dvp = cu(c["vn"]), cu(c["dvp"])
    vp = torch.full((B * N + 1, C), SENTINEL, device="cuda")
    dvn = torch.full((B * N + 1, C), SENTINEL, device="cuda")
    ops.gemm_raw(wsp_p, vn, vp, N, C, N, B, (0, ldw, 1), (N * C, 1, C), (N * C, C, 1), bias=bsp_p, bias_axis=1)
    ops.gemm_raw(wsp_p, dvp, dvn, N, C, N, B, (0, 1, ldw), (N * C, 1, C), (N * C, C, 1))
    torch.cuda.synchronize()
    name = f"spatial P {P} I {I} B {B} C {C}"
    within_baseline(f"{name} vp", vp[:B * N].view(B, N, C), c["ref"][0], c["base"][0])
    within_baseline(f"{name} dvn", dvn[:B * N].view(B, N, C), c["ref"][1], c["base"][1])
    guard = torch.cat([vp[B * N:], dvn[B * N:]])
    assert bool((bits(guard) == bits(torch.full_like(guard, SENTINEL))).all())


# ---------------------------------------------------------------------------------------------------------
# 5. gate tail
# ---------------------------------------------------------------------------------------------------------
def one_sum_allowance(ds, r, B, I, out):
    """The derived allowance for an output of gate_tail_wgrad_kernel that is ONE number: dbr = sum(ds) always, dWr = sum(ds r) at
    P = 1.  A single sum of B I terms of mixed sign has no other outputs to set its error against, and torch's pairwise fp32 sum over
    the same terms often lands within 1e-8 of float64, so 8 x that baseline can lie under the rounding of the terms themselves: each
    ds is stored in fp32 before the kernel reads it, a thread adds ceil(B I / 256) products, the block's tree has 8 levels, a
    product is rounded once: |error| <= (ceil(B I / 256) + 10) * 2^-24 * sum_{b,i} |ds r| (dbr: r = 1), from the REFERENCE's values
    (about 1e-6 to 1e-5 of the output; a sum of the wrong terms is off by its own size).  With more than one output (dWr at
    P = 31, 129) the plain bound holds and nothing is allowed.  -> relative to max|out| (absolute where out is zero)"""
    depth = -(-B * I // 256) + 10
    terms = ds.double().abs() if r is None else (ds.double().unsqueeze(1) * r.double()).abs().sum(1)
    scale = float(out.abs().max())
    return depth * 2.0 ** -24 * float(terms.sum()) / (scale if scale > 0 else 1.0)


def run_gate(ops, c, tag=""):
    """forward and backward as GateTailFn runs them, then the backward once more on weights that are NO softmax (it takes w as an
    operand).  Every output under the plain bound, but the two that are one number (one_sum_allowance).  dbr = sum(ds) with the
    softmax's own w is ZERO in exact arithmetic (sum_i w_i = 1), and the float64 yardstick's 1e-17 is its rounding, not a reference:
    the kernel's dbr is set against exactly zero there; on the free weights dbr is a real number, and a kernel that summed the wrong
    thing misses it"""
    I, B, P, beta = c["I"], c["B"], c["P"], c["beta"]
    name = f"gate I {I} B {B} P {P} beta {beta:g}{tag}"
    ref, base = c["ref"], c["base"]
    r, Wr, br, dw = cu(c["r"]), cu(c["Wr"]), cu(c["br"]), cu(c["dw"])
    s, w = ops.gate_tail_fwd(r, Wr, br, beta)
    s2, am = ops.gate_tail_fwd(r, Wr, br, beta, hard=True)
    dr, dWr, dbr = ops.gate_tail_bwd(w, dw, r, Wr, beta)
    free = dict(zip(("dr", "dWr", "dbr"), ops.gate_tail_bwd(cu(c["w_free"]), dw, r, Wr, beta)))
    torch.cuda.synchronize()
    assert same_bits(s, s2) and torch.equal(am, s.argmax(1))

    def allowed(k, rf, out):
        if k == "dbr":
            return one_sum_allowance(rf["ds"], None, B, I, out)
        return one_sum_allowance(rf["ds"], c["r"], B, I, out) if k == "dWr" and P == 1 else 0.0
    assert float(ref["dbr"].abs()) <= 1e-12
    zero = torch.zeros(1, dtype=torch.float64)
    for k, g in (("s", s), ("w", w), ("dr", dr), ("dWr", dWr)):
        assert bool(torch.isfinite(g).all()), (name, k)
        within_baseline(f"{name} {k}", g, ref[k], base[k], extra=allowed(k, ref, ref[k]))
    within_baseline(f"{name} dbr (exact: 0)", dbr, zero, base["dbr"], extra=allowed("dbr", ref, zero))
    if I == 1:
        assert bool((w == 1).all()) and not bool(dr.any()) and not bool(dWr.any()) and not bool(dbr.any())
    fref, fbase = c["free_ref"], c["free_base"]
    assert float(fref["dbr"].abs()) > 1e-3                                          # a real number, not rounding
    for k, g in free.items():
        within_baseline(f"{name} free w {k}", g, fref[k], fbase[k], extra=allowed(k, fref, fref[k]))


@pytest.mark.parametrize("I", K.GATE_I)
def test_gate_tail_against_float64(ops, I):
    """ops.gate_tail_fwd / gate_tail_bwd, the 8-wide form, at B = 1, 63, 64, 65 (one thread per sample, 64 per block), P = 1, 31,
    129 and beta = 1, 5: s, w, dr, dWr and dbr, and the backward on free weights (run_gate).  I = 1: w = 1 and every gradient zero,
    exactly.  gate_tail_fwd_kernel's score was a plain sequential fp32 sum and missed the plain bound where the output is one score
    (B = I = 1, P = 129: 5.0e-7, ratio 16.9); it is a compensated sum now.

    Measured on an MI355X, largest ratio over the 72 shapes and the saturated case: s 0.99, w 1.18, dr 3.46, dWr 13.22 (at P = 1,
    B I = 512, kernel 3.9e-7; with more than one output at most 3.92), dbr against zero 16.56 (saturated: 2.0e-6 absolute, allowed
    4.5e-6); on free weights dr 1.00, dWr 4.87, dbr 10.71 (I = 2, B = 63: 3.7e-7, allowed 2.3e-5).  The one-sum allowance is what
    passes dWr at (I 8, B 64, P 1, beta 5), dbr on free weights at (I 2, B 63, beta 5) and dbr of the saturated case; everything else
    is inside the plain bound."""
    for (i, B, P, beta) in K.GATE_SHAPES:
        if i == I:
            run_gate(ops, K.gate_case(i, B, P, beta))


def test_gate_tail_saturated(ops):
    """|beta * s| near 200: the softmax saturates, most weights underflow to zero, and every output stays finite"""
    run_gate(ops, K.saturated_gate_case(), " saturated")


@pytest.mark.parametrize("I", [2, 8])
def test_gate_tail_hard_routing_ties(ops, I):
    """hard routing on exact ties answers the FIRST index, in every sample"""
    for B in K.GATE_B:
        for P in K.GATE_P:
            c = K.tie_case(I, B, P)
            s, am = ops.gate_tail_fwd(cu(c["r"]), cu(c["Wr"]), cu(c["br"]), 1.0, hard=True)
            torch.cuda.synchronize()
            s = s.cpu()
            top = s.max(1, keepdim=True).values
            assert bool(((s == top).sum(1) == 2).all()), "the crafted ties are exact in the kernel's arithmetic too"
            assert torch.equal(am.cpu(), c["want"]), (I, B, P)


# ---------------------------------------------------------------------------------------------------------
# 6. fan-in and select-expert
# ---------------------------------------------------------------------------------------------------------
def run_fanin(ops, c):
    """-> (out, dw, selected) on the GPU, logits / dout / out in sentinel-padded rows; asserts the padding"""
    from mrn_amd._lib import call
    I, B, T, C = c["I"], c["B"], c["T"], c["C"]
    C4 = (C + 3) // 4 * 4
    held = [padded(l) for l in c["logits"]]
    logits = [v for _, v in held]
    w = cu(c["w"])
    owide, out = padded(torch.zeros(B, T, C))
    _, ptrs, lds, cls = ops._fanin_args(logits)
    call("mrn_fanin_fwd_f32", ptrs, lds, cls, I, w.data_ptr(), out.data_ptr(), out.stride(1), B, T, C, stream())
    dwide, dout = padded(c["dout"])
    dw = ops.fanin_bwd(logits, dout)
    index = cu(c["index"])
    sel = ops.select_expert(logits, index)
    torch.cuda.synchronize()
    assert padding_untouched(owide, C4) and padding_untouched(dwide, C)        # (the forward writes whole quads: up to C4)
    for (wide, _), l in zip(held, c["logits"]):
        assert padding_untouched(wide, l.shape[-1])
    assert same_bits(ops.fanin_fwd(logits, w), out)
    assert same_bits(sel, cu(K.select_reference(c["logits"], c["index"])))
    return out, dw, sel, logits


@pytest.mark.parametrize("C", K.FANIN_NEWEST)
@pytest.mark.parametrize("I", K.FANIN_I)
def test_fanin_against_float64(ops, I, C):
    """ops.fanin_fwd / fanin_bwd / select_expert, the 8-wide form, with ragged class counts that are no multiples of 4, at 1 x 1 and
    5 x 26 rows.  Newest class count 1023 / 1024 / 1025: around one trip of fanin_bwd_kernel's column loop (256 lanes x 4);
    5374: six trips.  An expert index outside 0 .. I - 1 selects the row of ones."""
    for B, T in K.FANIN_BT:
        c = K.fanin_case(I, K.fanin_classes(I, C), B, T)
        name = f"fanin I {I} classes {c['classes'][0]}..{C} rows {B}x{T}"
        out, dw, _, logits = run_fanin(ops, c)
        within_baseline(f"{name} out", out, c["ref"][0], c["base"][0])
        within_baseline(f"{name} dw", dw, c["ref"][1], c["base"][1])
        outside = torch.full((B,), I, dtype=torch.int64)
        outside[::2] = -1
        ones = ops.select_expert(logits, cu(outside))
        torch.cuda.synchronize()
        assert ones.shape == (B, T, C) and bool((ones == 1).all())


def test_fanin_65536_rows(ops):
    """256 samples x 256 steps (a TRBA router batch with labels up to 255): 65536 rows, one more than grid.y may hold.  Rows 0, 65534
    and 65535 element by element, every row by its sum; fanin_bwd and select_expert on the same case."""
    I, classes, B, T = K.FANIN_BIG
    c = K.fanin_case(I, classes, B, T)
    out, dw, _, _ = run_fanin(ops, c)                              # (select_expert: compared inside, every element)
    C = c["C"]
    flat, ref, base = out.reshape(B * T, C), c["ref"][0].reshape(B * T, C), c["base"][0].reshape(B * T, C)
    assert B * T == 65536
    for row in (0, 65534, 65535):
        within_baseline(f"fanin 65536 rows, row {row}", flat[row], ref[row], base[row])
    within_baseline("fanin 65536 rows, row sums", flat.double().sum(1), ref.sum(1), base.sum(1))
    within_baseline("fanin 65536 rows, every element", flat, ref, base)
    within_baseline("fanin 65536 rows dw", dw, c["ref"][1], c["base"][1])


# ---------------------------------------------------------------------------------------------------------
# 7. argmax
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.ARGMAX_C)
def test_argmax(ops, C):
    """ops.argmax_lastdim / argmax_prob_lastdim over strided rows at 1 and 5 rows (one wave per row, four rows per block): plain
    rows; the maximum tied in two lanes (first index); a NaN in the row (its index, as torch.max); a row of nothing but -inf
    (index 0, as torch.max -- the kernels answered 0x7fffffff).  The probability against the float64 softmax maximum."""
    for rows in K.ARGMAX_ROWS:
        for variant in K.ARGMAX_VARIANTS:
            c = K.argmax_case(rows, C, variant)
            buf, x = framed(c["x"], left=0, right=3)
            idx = ops.argmax_lastdim(x)
            idx2, prob = ops.argmax_prob_lastdim(x)
            torch.cuda.synchronize()
            name = f"argmax {rows}x{C} {variant}"
            assert x.stride(0) == C + 3 and frame_untouched(buf, 0, C)
            assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), c["idx"]), (name, idx.cpu().tolist(), c["idx"].tolist())
            assert torch.equal(idx2.cpu(), c["idx"]), name
            nan = torch.isnan(c["prob"])
            assert torch.equal(torch.isnan(prob.cpu()), nan), name
            want_nan = {"nan": list(range(rows)), "ninf": [rows // 2]}.get(variant, [])
            assert nan.nonzero().flatten().tolist() == want_nan, name
            z = torch.zeros(())
            within_baseline(f"{name} probability", torch.where(nan, z, prob.cpu()), torch.where(nan, z.double(), c["prob"]),
                            torch.where(nan, z, c["prob32"]))


# ---------------------------------------------------------------------------------------------------------
# 8. DMRouterFn end to end
# ---------------------------------------------------------------------------------------------------------
# The error of ONE output of a split-fp16 x3 GEMM (functional.x3_linear: "22-bit products, fp32 accumulation"), relative to the width of
# its outputs.  Each operand is a = hi + lo in two fp16 halves, |a - hi - lo| <= 2^-22 |a|, and the product drops lo * lo <= 2^-22 |a b|:
# three terms of 2^-22 per product, where an fp32 product has one rounding of 2^-24.  Over the reduction their independent signs add to
# 3 * 2^-22 * sqrt(K) products, and sqrt(K) products is how wide the outputs themselves are.
X3_OUTPUT_ERROR = 3 * 2.0 ** -22


def dcn_b_term(B, I, C):
    """The allowance for dcn_b, the one gradient that needs more than the plain bound, at the one shape where it does.
    dcn_b[p] = sum over (b, d, c) of dzn, the x3 data gradient of the channel projection (K = I C): n = B I C outputs of mixed sign,
    whose sum is about sqrt(n) outputs wide.  Each output carries the GEMM's error of 3 * 2^-22 of an output (X3_OUTPUT_ERROR); if
    those errors share a sign they add to n * 3 * 2^-22 outputs in the sum, sqrt(n) * 3 * 2^-22 of the sum itself, where independent
    ones would leave 3 * 2^-22.  The GEMMs upstream of dzn on dcn_b's path -- proj_1 and proj_2 (through y), the data gradient of
    proj_3 (dz2) -- feed dzn through the fp32 product dz2 * y and add their own 3 * 2^-22 each, not amplified.  The channel
    projection's and proj_3's forward products are not on the path.  -> 3 * 2^-22 * (sqrt(B I C) + 3), relative to max|reference|"""
    return X3_OUTPUT_ERROR * ((B * I * C) ** 0.5 + 3)


# (shape: gradients allowed their derived x3 term).  Every other quantity at every shape holds the plain bound (the table below); so does
# dcn_b at the three smaller shapes (ratios 0.53, 1.36, 2.40), where it is allowed nothing.
DM_X3_ALLOWED = {(2, 65, 8, 512): ("dcn_b",)}


@pytest.mark.parametrize("B,P,I,C", K.DM_SHAPES)
def test_dm_router_all_gradients_against_float64(ops, B, P, I, C):
    """functional.DMRouterFn, forward and ALL 17 gradients, against helpers.dm_router_reference in float64.  (1, 31, 1, 128): identity
    permutation, the B == 1 branches, the N < 64 fallback of the token weight gradient; (1, 33, 2, 256): B == 1 with the x3 token weight
    gradient; (3, 31, 3, 256): N = 93, ldw = 96; (2, 65, 8, 512): eight experts.  Every quantity is printed by max-norm (the
    within_baseline line) and by relative L2, then all are asserted.

    The GEMMs are split-fp16 x3 products, not fp32 sums, and still every quantity but one holds the convention's plain bound of 8 x
    the fp32 baseline.  Measured on an MI355X, ratio of the kernel's error to the baseline's (largest relative L2: 6.8e-6, dcn_b):

        (B, P, I, C)      out   dx    dn_w  dn_b  dw1   db1   dsn_w dsn_b dwsp  dbsp  dw2   db2   dcn_w dcn_b dwch  dbch  dw3   db3
        (1, 31, 1, 128)   0.77  0.69  1.14  0.59  0.66  0.34  0.69  0.39  0.45  0.99  1.05  1.03  0.83  0.53  1.09  0.64  0.87  1.12
        (1, 33, 2, 256)   0.80  1.97  1.35  1.27  0.75  0.79  1.06  1.48  0.94  1.49  0.70  1.13  1.97  1.36  0.83  0.74  1.17  1.08
        (3, 31, 3, 256)   1.31  0.95  0.84  1.63  1.23  0.88  0.87  1.31  0.78  1.11  1.61  0.87  0.74  2.40  0.85  0.92  1.37  0.90
        (2, 65, 8, 512)   1.62  2.65  1.65  1.20  1.19  1.47  1.34  1.63  1.23  1.54  1.50  2.12  1.84  11.18 0.98  1.25  1.26  0.75

    dcn_b at (2, 65, 8, 512): kernel 3.67e-6 against a baseline of 3.28e-7 -- a sum of 8192 outputs of the x3 data gradient of the
    channel projection (K = 4096).  There, and only there, it is allowed dcn_b_term: 3 * 2^-22 * (sqrt(8192) + 3) = 6.7e-5, written
    down from the format and the length of the sum, not from the 3.67e-6."""
    from mrn_amd.functional import DMRouterFn
    assert ops.ROUTER_GEMM_PRECISION == "fp16x3" and ops.ROUTER_WGRAD_X3 and ops.ROUTER_TOKEN_WGRAD_X3, \
        "the shapes below are chosen for the default split-fp16 x3 paths (and their N < 64 / R < 4096 fallbacks)"
    c = K.dm_case(B, P, I, C)
    x = cu(c["x"]).requires_grad_(True)
    params = [cu(p).requires_grad_(True) for p in c["params"]]
    out = DMRouterFn.apply(x, *params)
    out.backward(cu(c["dout"]))
    torch.cuda.synchronize()
    name = f"dm_router B {B} P {P} I {I} C {C}"
    ref_out, ref_g = c["ref"]
    base_out, base_g = c["base"]
    got = dict(zip(DM_ROUTER_GRADS, [x.grad] + [p.grad for p in params]))
    assert all(g is not None for g in got.values()) and len(got) == 17 == 1 + len(DM_ROUTER_PARAMS)
    failures = []

    def check(k, g, r, b, extra):
        l2 = float((g.detach().cpu().double() - r).norm() / r.norm())
        print(f"{name} {k}: relative L2 {l2:.2e}")
        try:
            within_baseline(f"{name} {k}", g, r, b, extra=extra)
        except AssertionError as e:
            failures.append(str(e))
    check("out", out, ref_out, base_out, 0.0)
    for k in DM_ROUTER_GRADS:
        assert got[k].shape == ref_g[k].shape, k
        assert k == "dcn_b" or k not in DM_X3_ALLOWED.get((B, P, I, C), ())
        check(k, got[k], ref_g[k], base_g[k], dcn_b_term(B, I, C) if k in DM_X3_ALLOWED.get((B, P, I, C), ()) else 0.0)
    assert not failures, "\n".join(failures)
