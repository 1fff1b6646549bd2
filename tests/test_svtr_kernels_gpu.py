"""The SVTR attention kernels, the operand producers and one trained block, called directly and compared with float64.

attention.hip (svtr_attention_kernel in its three mask forms, svtr_attention_x3_kernel, the dq and dk/dv kernels), SvtrAttentionFn's
GEMM fallback, layernorm_fwd_operand / ew_operand by value, and modules.svtr.Block.forward_train end to end with all 12 / 13
gradients in four modes.

Conventions (tests/test_router_kernels_gpu.py's): fp32 inputs made on the CPU (tests/svtr_cases.py); the float64 reference is the
written-out yardstick of tests/helpers.py, proven against torch autograd and the oracle in test_svtr_kernels_cpu.py; the kernel must
stay within max(8 x the baseline's error, 4 * 2^-24) relative to max|reference| (helpers.within_baseline, which prints the ratio).  The
baseline is the same yardstick in float32 for an exact-fp32 path, and for a split-fp16 x3 path the yardstick in float64 with every
operand of an x3 product replaced by its HL32 value at the scale the code uses (helpers.svtr_attention_x3_baseline,
svtr_block_reference(x3=...)).  test_svtr_kernels_cpu.py also proves that on these shapes a wrong kernel would miss that bound by a
factor of 10 at least.

Two derived allowances enter the bound as within_baseline's `extra`; neither is read off a kernel (svtr_cases.recompute_allowance).
(1) ops.svtr_attention_bwd keeps nothing of size N x N and recomputes P = exp2(s - lse), so P inherits the ABSOLUTE rounding of the
exponent.  On the kernel's own forward every ordinary case meets the plain bound and gets no allowance.  The exceptions are chosen
from the case data (baseline_exact_by_accident): N = 1, a dominant key and magnitude 300, where the fp32 baseline's
P = exp(S - max) / l is exactly 1 by accident while the kernels evaluate the score twice, in two orders (the dk/dv kernel scales k
where the forward scales q).  Their allowance is the rounding of those evaluations bounded per (query, key) from the case's own
running sums, in the kernels' order, carried to dv (and dq, dk) through the float64 P: dv 1.9e-6 / 3.0e-6 at N = 1 (measured 4.0e-7),
4.1e-4 / 6.1e-4 with a dominant key, 0.24 / 0.29 at magnitude 300 (measured 3.6e-3 / 5.2e-3: scores of 1e5 nats cannot be recomputed
in fp32 to better than 0.01 nat; a worst case over 16 roundings per score, 55 to 67 x the measurement, and a dv of zeros misses it).  dq and
dk of the saturated cases are 1e-20 and less in exact arithmetic; saturated_grad_allowance bounds the rounding of dP - D there.
On the float64 forward the test itself rounds out and lse to fp32: 2^-24 |lse| on the exponent of a whole row, 2^-24 sum |dO O| on D.
That is added to the plain bound of every case (0.1 to 0.9 of it): N 100, local, magnitude 12 has dv 9.8e-6 against a plain 9.5e-6.
(2) The block's x3 modes OR in 8 x the fp32 baseline's error (fp32_share below): an x3 product still accumulates in fp32, and the
weight / bias gradients, LayerNorms and attention of those modes are plain fp32, which the float64-on-split-operands baseline cannot
show (its error on a bias gradient, a plain column sum, is 0).  Needed by: out at C = 256 (kernel 5.9e-7, x3 baseline 5.0e-8, fp32
baseline 2.4e-7), dmlp.fc2.weight and dmixer.proj.weight at C = 256 (5.5e-7 at most), dmlp.fc2.bias at C = 128 (2.6e-7 against a floor
of 2.4e-7) and dmixer.proj.bias at N = 33 (2.6e-7).

One code change came with this file: ops.svtr_attention and ops.svtr_attention_bwd refuse a mask that is not symmetric (the forward
and dq kernels read mask[key][query], the dk/dv kernel and the bit form mask[query][key]); test_mask_symmetry_is_checked_once_per_mask
and test_svtr_kernels_cpu.py::test_a_mask_that_is_not_symmetric_is_refused.  No kernel was changed: the operand range of the x3 kernel
is now written above mrn_svtr_attention_f32 and in include/mrn_hip.h.

Measured on an MI355X, the largest ratio of a kernel's error to the baseline's ("ratio" is what within_baseline prints: kernel error /
max(baseline error, 2^-24 / 2)) per family, and where:
  fp32 forward out 1.93 (N 100, local, magnitude 12: kernel 1.7e-5, baseline 9.1e-6); lse 7.47 (N = 1, one head: kernel 2.2e-7 -- one
    score, v_log_f32 and a base change against a baseline of 1.7e-8; inside the floor).
  x3 forward, all cases 6.39 (N 33, additive, falling: kernel 6.6e-7, x3 baseline 1.0e-7).  The sweep, worst shape per magnitude:
    1e-3: 2.12 (kernel 9.2e-7, baseline 4.3e-7), 1.5: 3.81 (3.8e-7 / 1.0e-7), 12: 2.19 (5.9e-6 / 2.7e-6), 300: 1.00 (1.0e-7 / 1.0e-7).
  backward with the kernel's forward: dq 2.10, dk 2.15 (N 300, magnitude 1e-3, dout 1e-6), dv within the plain bound except the cases
    named under (1); with the float64 forward (dv 8.3 at N 100, magnitude 12, see (1)): dq 3.33 (N 32, rising, dout 1e-6), dk 3.48 (N 200, magnitude 12).
  GEMM fallback: out 1.19, dq 1.17, dk 1.30, dv 1.20 (all at head dimension 16).
  Block: f32 mode 2.98 (out, C = 256: kernel 7.3e-7, fp32 baseline 2.4e-7); x3 modes 11.88 against the x3 baseline alone (out, C = 256,
    see (2)), the same figure in the default mode, with fusion off and with the GEMM attention.
  Operand producers: LayerNorm 1.50 (mean, 5 x 64), GELU 1.00, GELU' 1.06, DropPath residual 0.99; every HL32 value equals
    hl_split of the kernel's own fp32 result bit for bit, the loose-gamma case included.
The backward is bit-exactly homogeneous in a power-of-two dout scale (2^-20, 2^13) for every result above 2^-100; below that, fp32
underflow (a probability of 2^-120 times a gradient of 2^-20 is a subnormal in one run and a normal number in the other) made 3 to 498
tiny results differ in five cases (magnitude 12 and 300, a dominant key), by less than 2^-100.

The suspicions of the issue, plainly.  The x3 range ends: clean -- finite and within the x3 baseline's bound from 1e-3 (lo halves in
fp16's subnormals) to 300.  The loose LayerNorm scale (one gamma 2^10 x the others): clean -- hi keeps its 11 bits at any magnitude and
lo stays a normal fp16; the block passes in all four modes and the small channels' HL32 values hold 2^-21.  The m_run = -inf path
(N = 200 / 300, local mask, float and bit form, fp32 and x3): clean.  The fallback backward (head dimensions 16, 32, 64): clean.
"""
from functools import partial

import pytest
import torch

from tests import svtr_cases as K
from tests.helpers import (FP16_PEAK, LN2, LOG2E, gelu_grad_reference, gelu_reference, baseline_bound, hl_split, layernorm_bound_scale,
                           layernorm_reference, pow2_scale_of, rel_err, within_baseline)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def cu(t):
    return None if t is None else t.cuda()


def same_bits(a, b):
    return a.shape == b.shape and bool((a.detach().contiguous().view(torch.int32) == b.detach().contiguous().view(torch.int32)).all())


def scale_pair(s):
    """{s, 1/s} on the device, as the kernels take a range scale"""
    return torch.tensor([s, 1.0 / s], device="cuda", dtype=torch.float32)


def hl_value(hl, rows, C, s=1.0):
    """the values an HL32 buffer holds: lines of [hi fp16 x 32 | lo fp16 x 32] per (row, 32 channels) -> (hi + lo) / s, float64 [rows, C]"""
    h = hl.view(torch.float16).view(rows, C // 32, 2, 32).cpu().double()
    return ((h[:, :, 0] + h[:, :, 1]) / s).reshape(rows, C)


def ulp_of_max(t):
    m = float(t.abs().max())
    return 2.0 ** (torch.floor(torch.log2(torch.tensor(m))).item() - 23) if m > 0 else 0.0


def att(i):
    return K.att_case(*K.ATT_CASES[i])


ALL = range(len(K.ATT_CASES))


# ---------------------------------------------------------------------------------------------------------
# a. ops.svtr_attention, exact fp32: the four call forms
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", ALL, ids=K.ATT_IDS)
def test_attention_fp32_forms(ops, i):
    c = att(i)
    B, N, h, C, name = c["B"], c["N"], c["heads"], c["C"], K.ATT_IDS[i]
    qkv, mask, ref, base = cu(c["qkv"]), cu(c["mask"]), c["ref"], c["base"]
    # 1. want_lse: the training forward -- always the additive float mask
    out, lse = ops.svtr_attention(qkv, h, c["scale"], mask, want_lse=True)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    within_baseline(f"{name} lse-form out", out, ref["out"], base["out"])
    within_baseline(f"{name} lse (x ln 2)", lse.double() * LN2, ref["lse"], base["lse"])
    # 2. / 3. no lse: the bit form for a 0 / -inf mask, the float form for any other
    plain = ops.svtr_attention(qkv, h, c["scale"], mask)
    within_baseline(f"{name} no-lse out", plain, ref["out"], base["out"])
    if c["mask_kind"] == "local":
        assert ops._mask_bits(mask) is not None
        assert float((plain - out).abs().max()) <= 2 * ulp_of_max(out), "bit form and float form of one binary mask"
    else:
        assert mask is None or ops._mask_bits(mask) is None
        assert same_bits(plain, out)                      # one kernel, one form: the lse store changes nothing
    # 4. want_hl with hl_scale: the proj Linear's operand at the scale of max|qkv|
    s = pow2_scale_of(c["qkv"])
    out4, lse4, hl = ops.svtr_attention(qkv, h, c["scale"], mask, want_lse=True, want_hl=True, hl_scale=scale_pair(s))
    assert same_bits(out4, out) and same_bits(lse4, lse)
    assert torch.equal(hl_value(hl, B * N, C, s), hl_split(out4.cpu().reshape(B * N, C), s))
    hl_only = ops.svtr_attention(qkv, h, c["scale"], mask, want_f32=False, want_hl=True)
    assert torch.equal(hl_value(hl_only, B * N, C), hl_split(plain.cpu().reshape(B * N, C)))
    torch.cuda.synchronize()
    assert same_bits(qkv.cpu(), c["qkv"])


# ---------------------------------------------------------------------------------------------------------
# b. ops.svtr_attention(x3=True): the frozen experts' kernel, against the x3 baseline
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", ALL, ids=K.ATT_IDS)
def test_attention_x3(ops, i):
    c = att(i)
    qkv, mask = cu(c["qkv"]), cu(c["mask"])
    out = ops.svtr_attention(qkv, c["heads"], c["scale"], mask, x3=True)
    assert bool(torch.isfinite(out).all())
    if mask is not None:
        assert (ops._mask_bits(mask) is not None) == (c["mask_kind"] == "local")
    within_baseline(f"{K.ATT_IDS[i]} x3 out (mag {c['mag']:g})", out, c["ref"]["out"], c["x3_base"])
    hl = ops.svtr_attention(qkv, c["heads"], c["scale"], mask, want_f32=False, want_hl=True, x3=True)
    assert torch.equal(hl_value(hl, c["B"] * c["N"], c["C"]), hl_split(out.cpu().reshape(-1, c["C"])))
    assert same_bits(qkv.cpu(), c["qkv"])


@pytest.mark.parametrize("mag", K.SWEEP_MAGNITUDES)
@pytest.mark.parametrize("B,N,h,mk", K.SWEEP_SHAPES)
def test_attention_x3_magnitude_sweep(ops, B, N, h, mk, mag):
    """the operand range of svtr_attention_x3_kernel: 64 x operand split with no range scale, from lo halves in fp16's subnormals
    (1e-3) to two octaves below its overflow (300)"""
    c = K.att_case(B, N, h, mk, "uniform", mag)
    out = ops.svtr_attention(cu(c["qkv"]), h, c["scale"], cu(c["mask"]), x3=True)
    assert bool(torch.isfinite(out).all())
    within_baseline(f"x3 sweep N {N} {mk} magnitude {mag:g}", out, c["ref"]["out"], c["x3_base"])


# ---------------------------------------------------------------------------------------------------------
# c. ops.svtr_attention_bwd: dq, dk, dv
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", ALL, ids=K.ATT_IDS)
def test_attention_backward(ops, i):
    c = att(i)
    h, C, name = c["heads"], c["C"], K.ATT_IDS[i]
    qkv, mask = cu(c["qkv"]), cu(c["mask"])
    out_k, lse_k = ops.svtr_attention(qkv, h, c["scale"], mask, want_lse=True)
    out_r, lse_r = cu(c["ref"]["out"].float()), cu((c["ref"]["lse"] * LOG2E).float())
    for setting, out, lse in (("kernel forward", out_k, lse_k), ("float64 forward", out_r, lse_r)):
        for m in K.DOUT_MAGNITUDES:
            dout, ref, base = cu(c["douts"][m]), c["refs"][m], c["bases"][m]
            dqkv = ops.svtr_attention_bwd(qkv, mask, out, dout, lse, h, c["scale"])
            assert bool(torch.isfinite(dqkv).all())
            for j, k in enumerate(("dq", "dk", "dv")):
                if setting == "kernel forward":        # the plain bound; an allowance only for the baseline_exact_by_accident cases
                    extra = K.grad_extra(c, k, m, "kernel")
                else:                                  # the plain bound PLUS what rounding out and lse to fp32 (this test's doing) costs
                    extra = baseline_bound(ref[k], base[k]) + K.grad_extra(c, k, m, "float64")
                within_baseline(f"{name} [{setting}, dout {m:g}] {k}", dqkv[..., j * C:(j + 1) * C], ref[k], base[k], extra=extra)
    # homogeneous in a power-of-two dout scale, bit for bit -- except where fp32 underflows: a probability of 2^-120 times a gradient
    # of 2^-20 is a subnormal (fewer bits, or flushed) in one run and a normal number in the other.  Such a term is below 2^-126 and
    # can move only results that are themselves tiny: every result above 2^-100 must be the same bits, the others agree to 2^-100
    dout = cu(c["dout"])
    one = ops.svtr_attention_bwd(qkv, mask, out_k, dout, lse_k, h, c["scale"])
    for e in (-20, 13):
        scaled = ops.svtr_attention_bwd(qkv, mask, out_k, dout * 2.0 ** e, lse_k, h, c["scale"])
        want = one * 2.0 ** e
        big = (want.abs() >= 2.0 ** -100) & (one.abs() >= 2.0 ** -100)
        assert same_bits(torch.where(big, scaled, 0), torch.where(big, want, 0)), f"{name}: dqkv(2^{e} dout) != 2^{e} dqkv(dout)"
        assert float(torch.where(big, 0, scaled - want).abs().max()) <= 2.0 ** -100 * max(1.0, 2.0 ** e)
        print(f"{name}: homogeneous in 2^{e}; {int((~big).sum())} of {big.numel()} results below 2^-100, "
              f"{int((scaled.view(torch.int32) != want.view(torch.int32)).sum())} of them differ")
    ranged, sc = ops.svtr_attention_bwd(qkv, mask, out_k, dout, lse_k, h, c["scale"], want_range=FP16_PEAK)
    assert same_bits(ranged, one) and float(sc[0]) == pow2_scale_of(one.cpu())
    assert same_bits(qkv.cpu(), c["qkv"])


# ---------------------------------------------------------------------------------------------------------
# d. SvtrAttentionFn on the GEMM fallback
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,mk", K.FALLBACK_CASES)
def test_attention_fn_gemm_fallback(ops, monkeypatch, d, N, mk):
    from mrn_amd.functional import SvtrAttentionFn
    c = K.fallback_case(d, N, mk)
    monkeypatch.setattr(ops, "SVTR_FUSED_ATTENTION", False)
    qkv = cu(c["qkv"]).requires_grad_(True)
    out = SvtrAttentionFn.apply(qkv, cu(c["mask"]), c["heads"], c["scale"])
    out.backward(cu(c["dout"]))
    torch.cuda.synchronize()
    name, C, ref, base = f"fallback d {d} N {N} {mk}", c["C"], c["ref"], c["base"]
    within_baseline(f"{name} out", out, ref["out"], base["out"])
    for j, k in enumerate(("dq", "dk", "dv")):
        within_baseline(f"{name} {k}", qkv.grad[..., j * C:(j + 1) * C], ref[k], base[k])


def test_attention_fn_takes_the_fused_kernels_by_default(ops):
    """the counterpart of the monkeypatch above: with the switch as it stands, head dimension 32 saves the log-sum-exp, not N x N"""
    from mrn_amd.functional import SvtrAttentionFn
    c = K.fallback_case(32, 33, "additive")
    assert ops.SVTR_FUSED_ATTENTION
    qkv = cu(c["qkv"]).requires_grad_(True)
    out = SvtrAttentionFn.apply(qkv, cu(c["mask"]), c["heads"], c["scale"])
    assert out.grad_fn.fused
    out.backward(cu(c["dout"]))
    for j, k in enumerate(("dq", "dk", "dv")):
        within_baseline(f"fused d 32 N 33 {k}", qkv.grad[..., j * c["C"]:(j + 1) * c["C"]], c["ref"][k], c["base"][k])


# ---------------------------------------------------------------------------------------------------------
# e. Block.forward_train end to end
# ---------------------------------------------------------------------------------------------------------
MODES = {"default": {}, "fusion off": {"TRAIN_OPERAND_FUSION": False}, "gemm attention": {"SVTR_FUSED_ATTENTION": False},
         "f32": {"ROUTER_GEMM_PRECISION": "f32"}}


def make_block(c):
    from mrn_amd.modules.svtr import Block
    blk = Block(c["dim"], c["heads"], mixer=c["mixer"], HW=list(c["HW"]), qkv_bias=c["qkv_bias"], drop_path=(1 - K.KEEP) if c["drop"] else 0.0,
                norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    blk.load_state_dict({k: v for k, v in c["params"].items() if v is not None})
    return blk.cuda().train()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("i", range(len(K.BLOCK_CASES)), ids=K.BLOCK_IDS)
def test_block_forward_train_all_gradients(ops, monkeypatch, i, mode):
    c = K.block_case(*K.BLOCK_CASES[i])
    for k, v in MODES[mode].items():
        monkeypatch.setattr(ops, k, v)
    blk = make_block(c)
    if c["mask"] is not None:
        assert torch.equal(blk.mixer.mask, c["mask"])
    if c["drop"]:
        blk.drop_path.forced_masks = [c["keep1"].clone(), c["keep2"].clone()]
    x = cu(c["x"]).requires_grad_(True)
    hits = ops.OPERAND_STATS["hits"]
    out = blk.forward_train(x)
    out.backward(cu(c["dout"]))
    ops.join_side_stream()
    torch.cuda.synchronize()
    hits = ops.OPERAND_STATS["hits"] - hits
    print(f"block {K.BLOCK_IDS[i]} [{mode}]: {hits} stashed operands served")
    if mode == "default":
        # forward: LN1 -> qkv, qkv -> attention, attention -> proj, LN2 -> fc1, fc1 -> GELU, GELU -> fc2 (6); backward: fc2's dx -> GELU',
        # GELU' -> fc1, the attention's dqkv -> qkv (3), and with DropPath the two branch gradients drop * dy -> fc2 and -> proj (2)
        assert hits == (11 if c["drop"] else 9), hits
    elif mode == "gemm attention":          # the fallback neither looks up qkv's scale nor leaves ctx's operand or dqkv's range: three fewer
        assert hits == (8 if c["drop"] else 6), hits
    else:                                   # fusion off: nothing is looked up by a consumer that honours the switch; f32: nothing is stashed
        assert hits == 0, hits
    (ref_out, G), base = c["ref"], (c["base"] if mode == "f32" else c["x3"]["separate" if mode == "fusion off" else "fused"])
    name = f"block {K.BLOCK_IDS[i]} [{mode}]"

    def fp32_share(ref, b32):
        """an x3 product still ACCUMULATES in fp32, and the weight and bias gradients, the LayerNorms and the attention run in plain
        fp32: whatever the fp32 baseline loses, the x3 modes lose as well, on top of the split.  The x3 baseline (float64 arithmetic
        on split operands) cannot show that share, so the fp32 baseline's own bound is OR-ed in -- both are reference-side numbers"""
        return 0.0 if mode == "f32" else 8.0 * rel_err(b32, ref)
    within_baseline(f"{name} out", out, ref_out, base[0], extra=fp32_share(ref_out, c["base"][0]))
    got = {"dx": x.grad}
    got.update({"d" + k: p.grad for k, p in blk.named_parameters()})
    assert sorted(got) == sorted(c["names"])
    for k in c["names"]:
        assert bool(torch.isfinite(got[k]).all()), k
        within_baseline(f"{name} {k}", got[k], G[k], base[1][k], extra=fp32_share(G[k], c["base"][1][k]))


@pytest.mark.parametrize("mode", ["default", "fusion off"])
def test_block_with_both_branches_dropped(ops, monkeypatch, mode):
    """DropPath multiplier 0 on both branches of every sample: out is x and dx is dout, bit for bit, and all 12 parameter gradients
    are exactly zero (+0 or -0: a product 0 * w keeps w's sign) -- through ew_operand's folded pass in the default mode and through
    residual_scale_rows(dy, dy, drop - 1) with the fusion off"""
    c = K.block_case(*K.BLOCK_CASES[1])
    for k, v in MODES[mode].items():
        monkeypatch.setattr(ops, k, v)
    blk = make_block(c)
    blk.drop_path.forced_masks = [torch.zeros(K.BLOCK_B), torch.zeros(K.BLOCK_B)]
    x = cu(c["x"]).requires_grad_(True)
    out = blk.forward_train(x)
    out.backward(cu(c["dout"]))
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert same_bits(out.cpu(), c["x"]) and same_bits(x.grad.cpu(), c["dout"])
    grads = dict(blk.named_parameters())
    assert len(grads) == 12
    for k, p in grads.items():
        assert p.grad is not None and not bool(p.grad.any()), k


def test_rows_with_a_zero_multiplier(ops):
    """DropPath multiplier 0: the forward leaves x as it is, bit for bit, and the branch gradient is exactly zero (ResidualScaleFn:
    dy + (0 - 1) dy in one fma), in the plain pass and in the pass that also folds the gradient's range"""
    N, C = 33, 64
    x, br, drop = cu(K.rnd(3, N, C, seed=500)), cu(K.rnd(3, N, C, seed=501)), torch.tensor([0.0, 1 / 0.7, 1 / 0.7], device="cuda")
    y = ops.residual_scale_rows(x, br, drop, N)
    assert same_bits(y[0], x[0])
    ref = x.cpu().double() + br.cpu().double() * drop.cpu().double().view(3, 1, 1)
    base = x.cpu() + br.cpu() * drop.cpu().view(3, 1, 1)
    within_baseline("residual_scale_rows", y, ref, base)
    db, _, sc = ops.ew_operand(ops.EW_RESIDUAL_SCALE, x, x, drop=drop - 1.0, rows_per_drop=N, want_amax=FP16_PEAK)
    assert same_bits(db[0], torch.zeros_like(db[0]))
    within_baseline("branch gradient drop * dy", db, x.cpu().double() * drop.cpu().double().view(3, 1, 1), x.cpu() * drop.cpu().view(3, 1, 1))
    assert float(sc[0]) == pow2_scale_of(db.cpu()) and float(sc[1]) == 1.0 / float(sc[0])


# ---------------------------------------------------------------------------------------------------------
# f. the operand producers, by value
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,loose", [(5, 64, False), (99, 256, False), (99, 64, True), (600, 128, False)])
def test_layernorm_operand_by_value(ops, rows, C, loose):
    x = K.rnd(rows, C, seed=510)
    gamma, beta = K.rnd(C, seed=511) * 0.3 + 1.0, K.rnd(C, seed=512) * 0.3
    if loose:
        gamma[K.LOOSE_CHANNEL] *= 1024.0            # the bound sqrt(C) max|gamma| + max|beta| is loose by 2^10 for every other channel
    ref = layernorm_reference(x, gamma, beta, 1e-6)
    base = layernorm_reference(x, gamma, beta, 1e-6, dtype=torch.float32)
    y, mean, rstd, hl, sc = ops.layernorm_fwd_operand(cu(x), cu(gamma), cu(beta), 1e-6)
    s = layernorm_bound_scale(gamma, beta, C)
    assert float(sc[0]) == s and float(sc[1]) == 1.0 / s
    assert s * float(ref["y"].abs().max()) <= FP16_PEAK
    name = f"layernorm operand {rows}x{C}" + (" loose" if loose else "")
    for k, got in (("y", y), ("mean", mean), ("rstd", rstd)):
        within_baseline(f"{name} {k}", got, ref[k], base[k])
    val = hl_value(hl, rows, C, s)
    assert torch.equal(val, hl_split(y.cpu(), s))                                  # the operand is the split of the fp32 result, exactly
    within_baseline(f"{name} HL32 value", val, hl_split(ref["y"], s), hl_split(base["y"], s))
    if loose:       # the small channels still carry 22 bits: hi has its 11 at any magnitude, lo is far above fp16's subnormals
        small = [j for j in range(C) if j != K.LOOSE_CHANNEL]
        assert rel_err(val[:, small], y.cpu().double()[:, small]) <= 2.0 ** -21


@pytest.mark.parametrize("rows,C", [(5, 64), (99, 256)])
def test_elementwise_operands_by_value(ops, rows, C):
    a, b = K.rnd(rows, C, seed=520) * 3, K.rnd(rows, C, seed=521)
    s = pow2_scale_of(a)
    y, hl, _ = ops.ew_operand(ops.EW_GELU, cu(a), scale=scale_pair(s), want_hl=True)
    within_baseline(f"gelu operand {rows}x{C} y", y, gelu_reference(a), gelu_reference(a, torch.float32))
    assert torch.equal(hl_value(hl, rows, C, s), hl_split(y.cpu(), s))
    within_baseline(f"gelu operand {rows}x{C} HL32 value", hl_value(hl, rows, C, s), hl_split(gelu_reference(a), s),
                    hl_split(gelu_reference(a, torch.float32), s))
    s = pow2_scale_of(b, FP16_PEAK / 2)                                            # half the target: gelu' <= 1.13
    y, hl, _ = ops.ew_operand(ops.EW_GELU_BWD, cu(a), cu(b), scale=scale_pair(s), want_hl=True)
    ref, base = b.double() * gelu_grad_reference(a), b * gelu_grad_reference(a, torch.float32)
    within_baseline(f"gelu' operand {rows}x{C} y", y, ref, base)
    assert torch.equal(hl_value(hl, rows, C, s), hl_split(y.cpu(), s)) and s * float(ref.abs().max()) < 65504
    within_baseline(f"gelu' operand {rows}x{C} HL32 value", hl_value(hl, rows, C, s), hl_split(ref, s), hl_split(base, s))
    drop = (K.rnd(rows, seed=522) > 0).float() / 0.7
    ref, base = a.double() + b.double() * drop.double().view(-1, 1), a + b * drop.view(-1, 1)
    s = pow2_scale_of(ref)
    y, hl, sc = ops.ew_operand(ops.EW_RESIDUAL_SCALE, cu(a), cu(b), drop=cu(drop), rows_per_drop=1, scale=scale_pair(s), want_hl=True,
                               want_amax=FP16_PEAK)
    within_baseline(f"residual operand {rows}x{C} y", y, ref, base)
    assert torch.equal(hl_value(hl, rows, C, s), hl_split(y.cpu(), s)) and float(sc[0]) == pow2_scale_of(y.cpu())
    within_baseline(f"residual operand {rows}x{C} HL32 value", hl_value(hl, rows, C, s), hl_split(ref, s), hl_split(base, s))


# ---------------------------------------------------------------------------------------------------------
# the mask contract
# ---------------------------------------------------------------------------------------------------------
def test_mask_symmetry_is_checked_once_per_mask(ops, monkeypatch):
    c = K.att_case(1, 33, 2, "additive", "uniform", 1.5)
    qkv, mask, calls = cu(c["qkv"]), cu(c["mask"]), []
    real = ops._mask_is_symmetric
    monkeypatch.setattr(ops, "_mask_is_symmetric", lambda m: calls.append(1) or real(m))
    out, lse = ops.svtr_attention(qkv, 2, c["scale"], mask, want_lse=True)
    ops.svtr_attention(qkv, 2, c["scale"], mask)
    ops.svtr_attention_bwd(qkv, mask, out, cu(c["dout"]), lse, 2, c["scale"])
    assert len(calls) == 1
    mask[0, 1] -= 1.0                                # an in-place change: checked again, and refused
    with pytest.raises(ValueError, match=r"ops\.svtr_attention_bwd:.*symmetric"):
        ops.svtr_attention_bwd(qkv, mask, out, cu(c["dout"]), lse, 2, c["scale"])
    with pytest.raises(ValueError, match=r"ops\.svtr_attention:.*symmetric"):
        ops.svtr_attention(qkv, 2, c["scale"], mask)
    assert len(calls) == 2
