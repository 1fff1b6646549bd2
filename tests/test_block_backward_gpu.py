"""The backward kernels of the trained conv block, called directly and compared with float64.

ConvBlockFn (mrn_amd/functional.py) is conv -> train-mode BatchNorm -> optional residual -> optional ReLU; its backward runs ops.bn_bwd
(mrn_bn_bwd_reduce_f32 / _finalize_f32 / _apply_f32) on the ReLU bit mask and the statistics ops.scale_shift_act / ops.bn_finalize
left behind.  Whole-model gradient tests see these kernels only through 2e-3 bands taken after the convolutions' own error; here
every one of them is a plain fp32 reduction that float64 pins to ~1e-6.

The yardstick: tests/helpers.py bn_bwd_reference / pack_relu_mask, proven against float64 autograd in test_block_backward_cpu.py.
The tolerance of every "against float64" comparison below is taken from the reference side, never from the kernel: the same
quantity is evaluated in fp32 with torch on the CPU, its error against float64 is e32 (relative to max|reference|, per output), and
the kernel must stay within max(8 * e32, 4 * 2^-24).  The factor 8 covers summation order (sequential per lane, then across lanes
and blocks, against torch's pairwise sums); 4 * 2^-24 is two roundings of the result itself, for outputs the CPU happens to get
exactly.  Each test prints kernel error, e32 and their ratio."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import F32_FLOOR, assert_close, bn_bwd_reference, pack_relu_mask, rel_err, unpack_relu_mask, within_baseline

pytestmark = pytest.mark.gpu

EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def cu(t):
    return t.cuda()


def bits(t):
    """the tensor's bit patterns: equality that tells -0.0 from +0.0 and holds for NaN"""
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------
# 2. ops.bn_bwd, mode by mode
# ---------------------------------------------------------------------------------------------------------
BN_BWD_SHAPES = [(1, 4),             # one row; C / 4 = 1: 256 row lanes per block
                 (257, 32),          # two row blocks, the second with 128 of 129 rows
                 (255, 1024),        # C / 4 = 256: one row lane
                 (1000, 512),        # two row lanes
                 (10237, 64),        # 40 partial blocks: the finalize kernel's lanes 0-7 take both loads, 8-31 the tail load
                 (600001, 4)]        # more than 2048 * 256 rows: the block count is capped, rows_per_block > 256


@functools.lru_cache(maxsize=None)
def bn_case(rows, C):
    """inputs (fp32, CPU) of one shape and, computed once, the float64 reference and the fp32 baseline of both ReLU settings"""
    y, dz, gamma = rnd(rows, C, seed=11), rnd(rows, C, seed=12), 1.5 + rnd(C, seed=13)          # gamma in [0.5, 2.5]
    y64 = y.double()
    mean = y64.mean(0).float()
    invstd = (1.0 / torch.sqrt(y64.var(0, unbiased=False) + EPS)).float()
    # z: every channel quad has both signs (lanes 0 / 1), and exact +0.0 / -0.0 (lanes 2 / 3 of every third / fifth quad)
    z = rnd(rows, C, seed=14)
    zq = z.view(rows, C // 4, 4)
    zq[..., 0] = zq[..., 0].abs() + 0.01
    zq[..., 1] = -zq[..., 1].abs() - 0.01
    quad = torch.arange(rows * (C // 4)).view(rows, C // 4)
    zq[..., 2][quad % 3 == 0] = 0.0
    zq[..., 3][quad % 5 == 0] = -0.0
    assert not torch.isnan(z).any() and bool((bits(z) == 0).any()) and bool((bits(z) == -2 ** 31).any())
    keep = (z > 0).float()
    ref, base = {}, {}
    for relu in (False, True):
        ref[relu] = bn_bwd_reference(dz, keep if relu else None, y, mean, invstd, gamma)
        base[relu] = bn_bwd_reference(dz, keep if relu else None, y, mean, invstd, gamma, dtype=torch.float32)
    return dict(rows=rows, C=C, y=y, dz=dz, gamma=gamma, mean=mean, invstd=invstd, z=z, keep=keep, ref=ref, base=base)


def bn_bwd(ops, c, relu, dz=None, **kw):
    """ops.bn_bwd on the case's inputs, masked by z unless the caller passes zmask"""
    z = None if ("zmask" in kw or not relu) else cu(c["z"])
    out = ops.bn_bwd(cu(c["dz"]) if dz is None else dz, z, cu(c["y"]), cu(c["mean"]), cu(c["invstd"]), cu(c["gamma"]), relu, **kw)
    torch.cuda.synchronize()
    return out


def check_bn_bwd(c, relu, got, tag):
    name = f"bn_bwd {c['rows']}x{c['C']} {tag}"
    return [within_baseline(f"{name} {label}", got[i], c["ref"][relu][i], c["base"][relu][i]) for i, label in enumerate(("dy", "dgamma", "dbeta"))]


@pytest.mark.parametrize("rows,C", BN_BWD_SHAPES)
def test_bn_bwd_against_float64(ops, rows, C):
    """dy, dgamma, dbeta of ops.bn_bwd without and with the ReLU mask (read from z) against the float64 formula on the same fp32
    statistics; dres is absent unless asked for.  Measured on an MI355X, kernel error / fp32 CPU baseline error (e32 was 1.5e-8 to
    5.4e-7) for dy / dgamma / dbeta:

        rows x C        no ReLU              ReLU from z
        1 x 4           exact                exact                 (dy, dgamma are exactly 0 at one row)
        257 x 32        1.00 / 0.74 / 0.89   1.00 / 0.74 / 0.86
        255 x 1024      0.93 / 5.07 / 4.10   0.87 / 6.16 / 2.19    (one block, one row lane: 255 terms in ONE sequential accumulator
        1000 x 512      0.96 / 1.78 / 1.60   1.00 / 2.77 / 1.54     against torch's pairwise sum -- the case the factor 8 is for)
        10237 x 64      1.00 / 1.10 / 1.24   1.01 / 1.30 / 1.39
        600001 x 4      1.00 / 0.72 / 2.60   1.00 / 3.15 / 6.26    (6.26: the baseline happened to reach 1.5e-8; the kernel's
                                                                    1.9e-7 is under the 4 * 2^-24 floor)"""
    c = bn_case(rows, C)
    for relu in (False, True):
        dy, dgamma, dbeta, dres = bn_bwd(ops, c, relu)
        assert dres is None
        assert dy.shape == (rows, C) and dgamma.shape == (C,) and dbeta.shape == (C,)
        check_bn_bwd(c, relu, (dy, dgamma, dbeta), "relu" if relu else "plain")


@pytest.mark.parametrize("rows,C", BN_BWD_SHAPES)
def test_bn_bwd_mask_forms_and_dres(ops, rows, C):
    """the 4-bit mask (zmask = pack_relu_mask(z), z = None) gives bit for bit what z gives; want_dres returns dz * (z > 0) bit for
    bit -- so the gradient at +0.0 and -0.0 is 0 -- and leaves the other results alone; two identical calls are bit-identical (the
    reduction has no atomics)"""
    c = bn_case(rows, C)
    from_z = bn_bwd(ops, c, True)
    zmask = cu(pack_relu_mask(c["z"]))
    assert zmask.dtype == torch.uint8 and zmask.numel() == rows * C // 4
    from_mask = bn_bwd(ops, c, True, zmask=zmask)
    for a, b in zip(from_z[:3], from_mask[:3]):
        assert torch.equal(a, b)
    masked = c["dz"] * c["keep"]
    zero = c["z"] == 0
    assert bool(zero.any()) and not bool(c["keep"][zero].any())
    for relu, want in ((True, masked), (False, c["dz"])):
        for kw in ({}, {"zmask": zmask}) if relu else ({},):
            dy, dgamma, dbeta, dres = bn_bwd(ops, c, relu, want_dres=True, **kw)
            assert torch.equal(dres.cpu(), want)
            if relu:
                assert not bool(dres.cpu()[zero].any())
                ref = from_z
            else:
                ref = bn_bwd(ops, c, False)
            assert torch.equal(dy, ref[0]) and torch.equal(dgamma, ref[1]) and torch.equal(dbeta, ref[2])
    again = bn_bwd(ops, c, True)
    for a, b in zip(from_z[:3], again[:3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rows,C", BN_BWD_SHAPES)
def test_bn_bwd_range_scale_has_no_stale_maximum(ops, rows, C):
    """range_target: the fifth result is the power-of-two scale ops.pow2_scale finds on dy, dy itself is unchanged, and a call on a
    1000 times smaller gradient right afterwards returns THAT tensor's (larger) scale: the 64-word workspace was put back to zero"""
    c = bn_case(rows, C)
    target = ops.TRAIN_OPERAND_PEAK
    plain = bn_bwd(ops, c, True)
    dy, dgamma, dbeta, dres, sc = bn_bwd(ops, c, True, range_target=target)
    assert dres is None and torch.equal(dy, plain[0]) and torch.equal(dgamma, plain[1]) and torch.equal(dbeta, plain[2])
    assert torch.equal(sc, ops.pow2_scale(dy, target))
    small = cu(c["dz"]) * 1e-3
    dy2, _, _, _, sc2 = bn_bwd(ops, c, True, dz=small, range_target=target)
    assert torch.equal(sc2, ops.pow2_scale(dy2, target))
    if float(dy.abs().max()) > 0:                      # (one row: dy is exactly 0 and both scales are 1)
        assert float(sc2[0]) > float(sc[0])
    else:
        assert sc.tolist() == [1.0, 1.0] and sc2.tolist() == [1.0, 1.0]
    # and the other way round: a large tensor after a small one
    _, _, _, _, sc3 = bn_bwd(ops, c, True, range_target=target)
    assert torch.equal(sc3, sc)


@pytest.mark.parametrize("rows,C", BN_BWD_SHAPES)
def test_bn_bwd_accumulates_into_the_parameter_gradients(ops, rows, C):
    """grad_acc = (weight.grad, bias.grad) preloaded with different non-zero values: None, None is returned, weight.grad becomes
    preload + dgamma and bias.grad preload + dbeta (a swap of the two shows at once: gamma is not 1 and the preloads differ), dy is
    unchanged"""
    c = bn_case(rows, C)
    plain = bn_bwd(ops, c, True)
    pre_w, pre_b = cu(3.0 + rnd(C, seed=15)), cu(-7.0 + rnd(C, seed=16))
    gw, gb = pre_w.clone(), pre_b.clone()
    dy, dgamma, dbeta, dres = bn_bwd(ops, c, True, grad_acc=(gw, gb))
    assert dgamma is None and dbeta is None and dres is None
    assert torch.equal(dy, plain[0])
    assert torch.equal(gw, pre_w + plain[1]) and torch.equal(gb, pre_b + plain[2])
    if rows > 1:
        assert not torch.equal(plain[1], plain[2])


@pytest.mark.parametrize("C", [96, 2048, 6])
def test_bn_bwd_refuses_unsupported_channel_counts(ops, C):
    """C / 4 must divide 256 (C = 96: 24 does not), C <= 1024, C % 4 == 0: the reduce launcher refuses by name before anything is
    launched; a canary tensor next to the operands keeps its fill and a supported call right afterwards is still correct"""
    rows = 8
    y, dz = cu(rnd(rows, C, seed=17)), cu(rnd(rows, C, seed=18))
    mean, invstd, gamma = cu(rnd(C, seed=19)), cu(1.0 + rnd(C, seed=20).abs()), cu(1.5 + rnd(C, seed=21))
    canary = torch.full((rows, C), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="mrn_bn_bwd_reduce_f32"):
        ops.bn_bwd(dz, None, y, mean, invstd, gamma, False)
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())
    c = bn_case(257, 32)
    check_bn_bwd(c, True, bn_bwd(ops, c, True), "after a refusal")


# ---------------------------------------------------------------------------------------------------------
# 3. ops.scale_shift_act with pos_mask and range_target
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["residual_relu", "relu", "linear"])
@pytest.mark.parametrize("rows,C", [(1, 4), (257, 32), (1031, 1024), (70001, 12)])
def test_scale_shift_act_mask_and_range(ops, rows, C, variant):
    """the forward side of the backward pass's contract: with pos_mask and range_target the output is bit for bit the plain call's,
    the mask is pack_relu_mask(out) (bit 0 for 0, -0.0 and NaN) and the cached range scale is ops.pow2_scale of the output without
    its NaN.  Channel 0 has scale = shift = 0 (output exactly 0), channel 1 produces -0.0, one lane of the last channel is NaN.
    (70001, 12): several grid-stride trips, n4 no multiple of 256."""
    relu, with_res = variant != "linear", variant == "residual_relu"
    x, scale, shift, res = rnd(rows, C, seed=30), rnd(C, seed=31) * 2, rnd(C, seed=32), rnd(rows, C, seed=33)
    scale[0], shift[0], res[:, 0] = 0.0, 0.0, 0.0
    x[:, 1], scale[1], shift[1], res[:, 1] = 0.0, -1.0, -0.0, -0.0
    x[rows // 2, C - 1] = float("nan")
    res = cu(res) if with_res else None
    target = ops.TRAIN_OPERAND_PEAK
    plain = ops.scale_shift_act(cu(x), cu(scale), cu(shift), relu=relu, residual=res, out=torch.empty(rows, C, device="cuda"))
    mask = torch.full((rows * C // 4,), 0xA5, device="cuda", dtype=torch.uint8)
    out = ops.scale_shift_act(cu(x), cu(scale), cu(shift), relu=relu, residual=res, out=torch.empty(rows, C, device="cuda"),
                              range_target=target, pos_mask=mask)
    sc = ops.cached_scale(out)
    assert sc is not None, "scale_shift_act(range_target=...) left no range scale for its output"
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(plain))
    host = out.cpu()
    assert bool(torch.isnan(host[rows // 2, C - 1])) and int(torch.isnan(host).sum()) == 1
    assert bool((bits(host[:, 0]) == 0).all())                                    # exactly +0.0
    assert bool((host[:, 1] == 0).all())
    if not relu:
        assert bool((bits(host[:, 1]) == -2 ** 31).all())                         # -0.0 reached the output
    assert torch.equal(mask.cpu(), pack_relu_mask(host))
    mq = mask.cpu().view(rows, C // 4)
    assert not bool((mq[:, 0] & 3).any())                                          # channels 0 (zero) and 1 (-0.0)
    assert not bool((mq[rows // 2, C // 4 - 1] >> 3) & 1)                          # the NaN lane
    if rows > 1:
        assert bool(mask.any()) and (relu or int((host < 0).sum()) > 0)
    assert torch.equal(sc, ops.pow2_scale(torch.nan_to_num(out, nan=0.0).contiguous(), target))
    # the semantics do not depend on the variant: what the backward pass reads is (out > 0)
    assert torch.equal(unpack_relu_mask(mask.cpu()).view(rows, C), host > 0)


# ---------------------------------------------------------------------------------------------------------
# 4. ConvBlockFn with BatchNorm, end to end, against float64 autograd
# ---------------------------------------------------------------------------------------------------------
POOL = ((2, 2), (2, 1), (0, 1))
#                 B  Cin Cout  H   W  stride  residual relu precision pool
BLOCK_CONFIGS = [(3, 32, 64, 8, 33, (1, 1), True, True, "fp16x3s", None),
                 (3, 64, 128, 4, 65, (1, 1), False, True, "fp16x3s", None),
                 (3, 128, 128, 4, 33, (1, 1), True, True, "fp16x3s", None),        # Winograd forward
                 (3, 4, 32, 32, 64, (1, 1), False, True, "fp16x3s", None),         # Cin = 4 falls to f32
                 (3, 64, 128, 8, 32, (2, 1), False, False, "fp16x3s", None),       # the downsample form
                 (2, 32, 64, 7, 9, (1, 1), True, True, "f32", None),
                 (2, 32, 64, 8, 16, (1, 1), False, True, "fp16x3s", POOL)]


def make_block(cfg):
    """(conv, bn) CPU float32 modules with non-trivial affine parameters and running statistics, input, residual, upstream gradient"""
    B, Cin, Cout, H, W, stride, with_res, relu, precision, pool = cfg
    torch.manual_seed(400 + Cin + Cout + H + W)
    conv = torch.nn.Conv2d(Cin, Cout, 3, stride, 1)
    bn = torch.nn.BatchNorm2d(Cout)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.5 * rnd(Cout, seed=401))
        bn.bias.copy_(0.5 * rnd(Cout, seed=402))
        bn.running_mean.copy_(rnd(Cout, seed=403))
        bn.running_var.copy_(1.0 + 0.5 * rnd(Cout, seed=404))
    x = rnd(B, Cin, H, W, seed=405)
    Ho, Wo = (H + 2 - 3) // stride[0] + 1, (W + 2 - 3) // stride[1] + 1
    res = rnd(B, Cout, Ho, Wo, seed=406) if with_res else None
    if pool is not None:
        Ho, Wo = (Ho + 2 * pool[2][0] - pool[0][0]) // pool[1][0] + 1, (Wo + 2 * pool[2][1] - pool[0][1]) // pool[1][1] + 1
    g = rnd(B, Cout, Ho, Wo, seed=407)
    return conv, bn, x, res, g


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def run_block_gpu(ops, cfg, conv, bn, x, res, g, monkeypatch=None):
    """conv_block forward + backward on the GPU -> (modules, out, z before the pool, x.grad, residual.grad), all NCHW views"""
    from mrn_amd import functional as Fn
    from mrn_amd.modules._nn import conv_block
    B, Cin, Cout, H, W, stride, with_res, relu, precision, pool = cfg
    convc, bnc = copy.deepcopy(conv).cuda(), copy.deepcopy(bn).cuda().train()
    xc = cu(nhwc(x)).requires_grad_(True)
    resc = cu(nhwc(res)).requires_grad_(True) if with_res else None
    seen = []
    if pool is not None:
        real = Fn.MaxPoolFn

        class Spy:
            @staticmethod
            def apply(y, *a):
                seen.append(y)
                return real.apply(y, *a)
        monkeypatch.setattr(Fn, "MaxPoolFn", Spy)
    out = conv_block(xc, convc, bnc, relu=relu, residual=resc, pool=pool, precision=precision)
    z = seen[0] if pool is not None else out
    out.backward(cu(nhwc(g)))
    torch.cuda.synchronize()
    to_nchw = lambda t: None if t is None else t.detach().permute(0, 3, 1, 2).cpu()
    return convc, bnc, to_nchw(out), to_nchw(z), to_nchw(xc.grad), to_nchw(resc.grad if with_res else None)


@pytest.mark.parametrize("cfg", BLOCK_CONFIGS, ids=lambda c: "B%d-%dto%d-%dx%d-s%d%d-%s%s%s-%s" % (
    c[0], c[1], c[2], c[3], c[4], c[5][0], c[5][1], "res" if c[6] else "nores", "-relu" if c[7] else "", "-pool" if c[9] else "", c[8]))
def test_conv_block_with_batchnorm_against_float64_autograd(ops, cfg, monkeypatch):
    """conv_block(x, conv, bn, relu, residual) in train mode: forward output, dx, dW, the conv's db, dgamma, dbeta, d(residual) and
    the running statistics against torch.nn.Conv2d + BatchNorm2d in float64, with the conv tolerances of
    test_strided_conv_block_gradients.  The reference's backward runs through the GPU's own ReLU mask (z_gpu > 0) as a constant (and,
    under the max-pool, the GPU's own window choice); where float64 disagrees about a sign or a choice is counted separately: at
    most 1e-4 of the elements, each with |z64| (each gap) below the forward tolerance.  The conv bias in front of train-mode
    BatchNorm has gradient exactly 0.  Measured on an MI355X: no sign and no window-choice disagreement in any configuration."""
    B, Cin, Cout, H, W, stride, with_res, relu, precision, pool = cfg
    conv, bn, x, res, g = make_block(cfg)
    convc, bnc, out, z, dx, dres = run_block_gpu(ops, cfg, conv, bn, x, res, g, monkeypatch)
    conv64, bn64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double().train()
    x64 = x.double().requires_grad_(True)
    res64 = res.double().requires_grad_(True) if with_res else None
    pre = bn64(conv64(x64))
    if with_res:
        pre = pre + res64
    z64 = F.relu(pre) if relu else pre
    fwd_tol = 2e-5 + 1e-5 * float(z64.detach().abs().max())
    assert_close("block forward", z, z64, atol=2e-5, rtol=1e-5)
    act = pre * (z > 0).double() if relu else pre
    if relu:
        wrong = (z > 0) != (pre.detach() > 0)
        print(f"conv block {cfg}: {int(wrong.sum())} of {wrong.numel()} signs differ from float64")
        assert int(wrong.sum()) <= 1e-4 * wrong.numel()
        assert not bool(wrong.any()) or float(pre.detach()[wrong].abs().max()) < fwd_tol
    if pool is not None:
        idx = F.max_pool2d(z.double(), *pool, return_indices=True)[1]
        p64, idx64 = F.max_pool2d(z64.detach(), *pool, return_indices=True)
        assert_close("block forward, pooled", out, p64, atol=2e-5, rtol=1e-5)
        flat = z64.detach().flatten(2)
        gap = (flat.gather(2, idx64.flatten(2)) - flat.gather(2, idx.flatten(2))).abs()
        moved = idx64 != idx
        print(f"conv block {cfg}: {int(moved.sum())} of {moved.numel()} pool windows choose another element than float64")
        assert int((gap > 0).sum()) <= 1e-4 * gap.numel() and float(gap.max()) < fwd_tol
        act = act.flatten(2).gather(2, idx.flatten(2)).view_as(idx)
    (act * g.double()).sum().backward()
    assert_close("block dx", dx, x64.grad, atol=2e-5, rtol=1e-4)
    assert_close("block dW", convc.weight.grad, conv64.weight.grad, atol=1e-4, rtol=1e-4)
    assert float(conv64.bias.grad.abs().max()) < 1e-12
    assert convc.bias.grad is not None and float(convc.bias.grad.abs().max()) == 0
    assert_close("block dgamma", bnc.weight.grad, bn64.weight.grad, atol=1e-4, rtol=1e-4)
    assert_close("block dbeta", bnc.bias.grad, bn64.bias.grad, atol=1e-4, rtol=1e-4)
    if with_res:
        assert_close("block dres", dres, res64.grad, atol=1e-4, rtol=1e-4)
    assert_close("running_mean", bnc.running_mean, bn64.running_mean, atol=1e-4, rtol=1e-4)
    assert_close("running_var", bnc.running_var, bn64.running_var, atol=1e-4, rtol=1e-4)
    assert int(bnc.num_batches_tracked) == 1


def test_conv_block_direct_gradients_accumulate_into_preloaded_grads(ops):
    """the path the learners use: `with ops.direct_gradients(): loss.backward()` on parameters whose .grad already holds something,
    with the weight gradients on the side stream and without.  Every .grad is preload + the autograd-mode gradient within
    max(4 x the run-to-run noise of the autograd path, 1e-6 max|g|) (the rule of test_loop_a_weight_gradients_on_the_side_stream_match);
    the BatchNorm weight / bias gradients, added by the finalize launch, are bit for bit preload + the plain ones."""
    from mrn_amd.modules._nn import conv_block
    cfg = BLOCK_CONFIGS[0]
    B, Cin, Cout, H, W, stride, with_res, relu, precision, pool = cfg
    conv, bn, x, res, g = make_block(cfg)
    convc, bnc = copy.deepcopy(conv).cuda(), copy.deepcopy(bn).cuda().train()
    params = {"weight": convc.weight, "bias": convc.bias, "gamma": bnc.weight, "beta": bnc.bias}
    preload = {n: cu(2.0 + rnd(*p.shape, seed=410 + i)) for i, (n, p) in enumerate(params.items())}

    def run(direct, pre):
        for n, p in params.items():
            p.grad = preload[n].clone() if pre else None
        xc = cu(nhwc(x)).requires_grad_(True)
        resc = cu(nhwc(res)).requires_grad_(True)
        loss = (conv_block(xc, convc, bnc, relu=relu, residual=resc, precision=precision) * cu(nhwc(g))).sum()
        if direct:
            with ops.direct_gradients():
                loss.backward()
        else:
            loss.backward()
        torch.cuda.synchronize()
        got = {n: p.grad.clone() for n, p in params.items()}
        got["x"], got["res"] = xc.grad.clone(), resc.grad.clone()
        return got

    keep = ops.WGRAD_SIDE_STREAM
    try:
        ops.WGRAD_SIDE_STREAM = False
        plain, plain2 = run(False, False), run(False, False)
        assert all(float(plain[n].abs().max()) > 0 for n in ("weight", "gamma", "beta", "x", "res"))
        for side in (True, False):
            ops.WGRAD_SIDE_STREAM = side
            got = run(True, True)
            for n in plain:
                want = plain[n] + preload[n] if n in preload else plain[n]
                noise = float((plain[n] - plain2[n]).abs().max())
                err = float((got[n] - want).abs().max())
                print(f"direct gradients, side stream {side}: {n} max|g| {float(plain[n].abs().max()):.3e} run-to-run {noise:.3e} err {err:.3e}")
                assert err <= max(4 * noise, 1e-6 * float(plain[n].abs().max())), (side, n, err, noise)
            assert torch.equal(got["gamma"], preload["gamma"] + plain["gamma"])
            assert torch.equal(got["beta"], preload["beta"] + plain["beta"])
            assert torch.equal(got["bias"], preload["bias"])
    finally:
        ops.WGRAD_SIDE_STREAM = keep


# ---------------------------------------------------------------------------------------------------------
# 5. BatchNorm2dFn (the RCNN extractor's path)
# ---------------------------------------------------------------------------------------------------------
def bn_stats_rows():
    """BN_STATS_ROWS of rowops.hip, read through mrn_bn_stats_blocks: the largest row count that still takes one block"""
    from mrn_amd._lib import call
    rows = 1
    while call("mrn_bn_stats_blocks", rows + 1) == 1:
        rows += 1
        assert rows < 1 << 16
    return rows


@pytest.mark.parametrize("offset", [0.0, 8.0])
@pytest.mark.parametrize("shape", [(1, 4), ("BN_STATS_ROWS+1", 32), (5000, 512), (3001, 20)])
def test_bn_stats_and_finalize_against_float64(ops, shape, offset):
    """ops.bn_stats -> ops.bn_finalize(save=True): mean, invstd, scale, shift and the running statistics against float64, without
    and with a per-channel offset of 8 standard deviations (conditioning-limited: var = E[x^2] - mean^2 cancels 65 to 1, and the
    baseline carries that).  The baseline is the same algorithm with plain fp32 sums: torch CPU fp32 x.sum(0) and (x * x).sum(0),
    then -- as the finalize kernel does -- the division, the subtraction and the square root in float64, results rounded to fp32.
    (Finalising the baseline in fp32 instead would make it exact by accident at one row, where fl(x * x) - fl(mean * mean) is 0.)
    One row: torch refuses to train BatchNorm on one value per channel; the kernel keeps the biased variance (0) there.
    Measured on an MI355X, kernel error / baseline error: at most 3.11 without the offset (running_var at 257 x 32), at most 2.21 with
    it, where both sides lose the same digits (invstd errors of 6e-6 to 1.5e-5 from 257 rows on, and 0.13 at ONE row with the offset:
    fl(x * x) - mean^2 is rounding noise of the size of eps there -- baseline and kernel agree to the last bit on it)."""
    rows, C = shape
    per_block = bn_stats_rows()
    if rows == "BN_STATS_ROWS+1":
        rows = per_block + 1
    x = rnd(rows, C, seed=50)
    if offset:
        x = x + offset * (x.std(0, unbiased=False) if rows > 1 else torch.ones(C))
    gamma, beta = 1.5 + rnd(C, seed=51), rnd(C, seed=52)
    rm0, rv0 = rnd(C, seed=53), 1.5 + rnd(C, seed=54)
    mom = 0.1

    def finalize(s, q):
        """float64 column sums -> the six results"""
        mean = s / rows
        var = (q / rows - mean * mean).clamp_min(0)
        invstd = 1.0 / torch.sqrt(var + EPS)
        scale = gamma.double() * invstd
        shift = beta.double() - mean * scale
        unbiased = var * rows / max(rows - 1, 1)
        return mean, invstd, scale, shift, (1 - mom) * rm0.double() + mom * mean, (1 - mom) * rv0.double() + mom * unbiased

    x64 = x.double()
    ref = list(finalize(x64.sum(0), (x64 * x64).sum(0)))
    ref[1] = 1.0 / torch.sqrt(x64.var(0, unbiased=False) + EPS)               # (float64 two-pass variance: the true one)
    ref[2] = gamma.double() * ref[1]
    ref[3] = beta.double() - ref[0] * ref[2]
    ref[5] = (1 - mom) * rv0.double() + mom * x64.var(0, unbiased=False) * rows / max(rows - 1, 1)
    base = [t.float() for t in finalize(x.sum(0).double(), (x * x).sum(0).double())]
    rm, rv = cu(rm0), cu(rv0)
    part = ops.bn_stats(cu(x))
    assert part.shape == ((rows + per_block - 1) // per_block, 2, C)
    scale, shift, mean, invstd = ops.bn_finalize(part, C, rows, cu(gamma), cu(beta), rm, rv, mom, EPS, save=True)
    torch.cuda.synchronize()
    names = ("mean", "invstd", "scale", "shift", "running_mean", "running_var")
    for name, got, r, b in zip(names, (mean, invstd, scale, shift, rm, rv), ref, base):
        within_baseline(f"bn_stats {rows}x{C} offset {offset:g} {name}", got, r, b)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7, 32), (3, 4, 33, 64)])
def test_batch_norm_nhwc_training_against_float64_autograd(ops, shape, relu):
    """batch_norm_nhwc(x, bn, relu) in train mode (BatchNorm2dFn: bn_stats -> bn_finalize -> scale_shift_act; backward: bn_bwd
    masked by the output itself): output, dx, dgamma, dbeta and the running statistics against float64 autograd through the GPU's own
    ReLU mask, within 8 x what fp32 torch autograd on the CPU reaches.  Sign disagreements with float64: at most 1e-4 of the
    elements, each with |y64| below 8 x the fp32 baseline's forward error.  Measured on an MI355X: ratios 0.65 to 3.85 (dbeta at
    (2, 5, 7, 32) with ReLU), no sign disagreement in either shape."""
    from mrn_amd import functional as Fn
    B, H, W, C = shape
    x, g = rnd(*shape, seed=60), rnd(*shape, seed=61)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(1.5 + rnd(C, seed=62))
        bn.bias.copy_(0.3 * rnd(C, seed=63))
        bn.running_mean.copy_(rnd(C, seed=64))
        bn.running_var.copy_(1.5 + rnd(C, seed=65))
    bnc = copy.deepcopy(bn).cuda().train()
    xc = cu(x).requires_grad_(True)
    y = Fn.batch_norm_nhwc(xc, bnc, relu)
    y.backward(cu(g))
    torch.cuda.synchronize()
    mask = (y.detach().cpu() > 0)

    def reference(dtype):
        m = copy.deepcopy(bn).to(dtype).train()
        xr = x.to(dtype).requires_grad_(True)
        pre = m(xr.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        out = F.relu(pre) if relu else pre
        ((pre * mask.to(dtype) if relu else pre) * g.to(dtype)).sum().backward()
        return pre.detach(), [out.detach(), xr.grad, m.weight.grad, m.bias.grad, m.running_mean, m.running_var]
    pre64, ref = reference(torch.float64)
    _, base = reference(torch.float32)
    got = [y, xc.grad, bnc.weight.grad, bnc.bias.grad, bnc.running_mean, bnc.running_var]
    for name, a, r, b in zip(("y", "dx", "dgamma", "dbeta", "running_mean", "running_var"), got, ref, base):
        within_baseline(f"batch_norm_nhwc {shape} relu={relu} {name}", a, r, b)
    if relu:
        wrong = mask != (pre64 > 0)
        print(f"batch_norm_nhwc {shape}: {int(wrong.sum())} of {wrong.numel()} signs differ from float64")
        tol = max(8 * rel_err(base[0], ref[0]), F32_FLOOR) * float(ref[0].abs().max())
        assert int(wrong.sum()) <= 1e-4 * wrong.numel()
        assert not bool(wrong.any()) or float(pre64[wrong].abs().max()) < tol


# ---------------------------------------------------------------------------------------------------------
# 6. the small kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sliced", [False, True])
def test_ew_rows_ops(ops, sliced):
    """EW_ADD, EW_ADD_RELU, EW_RELU_BWD exactly; EW_SIGMOID (values up to +-80) and EW_SIGMOID_BWD against float64; contiguous
    operands and column slices of wider matrices (lda != C), the result too -- columns outside the slice keep their fill
    (measured: both sigmoid ops at exactly the fp32 CPU baseline's error)"""
    rows, C, wide = 37, 256, 640
    A, Bm = rnd(rows, wide, seed=70), rnd(rows, wide, seed=71)
    A.view(-1)[::9] = 0.0
    A.view(-1)[4::17] = -0.0
    if sliced:
        a, b = A[:, :C], Bm[:, C:2 * C]
        ac, bc = cu(A)[:, :C], cu(Bm)[:, C:2 * C]
    else:
        a, b = A[:, :C].contiguous(), Bm[:, C:2 * C].contiguous()
        ac, bc = cu(a), cu(b)

    def run(op, p, q=None):
        if not sliced:
            return ops.ew_rows(op, p, q)
        buf = torch.full((rows, wide), 9.0, device="cuda")
        out = ops.ew_rows(op, p, q, out=buf[:, 128:128 + C])
        assert bool((buf[:, :128] == 9.0).all()) and bool((buf[:, 128 + C:] == 9.0).all())
        return out
    assert_close("add", run(ops.EW_ADD, ac, bc), a + b, atol=0, rtol=0)
    assert_close("add_relu", run(ops.EW_ADD_RELU, ac, bc), F.relu(a + b), atol=0, rtol=0)
    assert_close("relu_bwd", run(ops.EW_RELU_BWD, ac, bc), b * (a > 0), atol=0, rtol=0)
    s = a * 80.0
    s[0, :4] = torch.tensor([80.0, -80.0, 0.0, -0.0])
    sc = cu(s) if not sliced else cu(torch.cat([s, s], 1))[:, :C]
    sig64 = torch.sigmoid(s.double())
    got = run(ops.EW_SIGMOID, sc)
    within_baseline(f"sigmoid sliced={sliced}", got, sig64, torch.sigmoid(s))
    assert float(got[0, 0]) == 1.0 and 0 < float(got[0, 1]) < 1e-34 and float(got[0, 2]) == 0.5
    y = torch.sigmoid(s)                                           # the saved forward result, as SigmoidFn hands it back
    yc = cu(y) if not sliced else cu(torch.cat([y, y], 1))[:, C:]
    within_baseline(f"sigmoid_bwd sliced={sliced}", run(ops.EW_SIGMOID_BWD, yc, bc), b.double() * y.double() * (1 - y.double()), b * y * (1 - y))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 1024])
def test_softmax_rows_and_backward(ops, N):
    """in-place row softmax, one wave per row: N around the wave size and at the limit, row counts that are no multiple of the 4
    rows of a block, an additive [Nq, N] mask with -inf entries shared over the leading dims; then its backward on the kernel's own
    probabilities.  Measured on an MI355X: kernel error / fp32 CPU baseline error at most 1.09 forward, 1.89 backward."""
    for lead, Nq, masked in ((1, 1, False), (7, 1, False), (1, 7, True), (7, 1, True), (3, 5, True)):
        s = rnd(lead, Nq, N, seed=80 + lead, scale=6.0)
        mask = None
        if masked:
            mask = torch.zeros(Nq, N)
            mask[rnd(Nq, N, seed=81) > 0.2] = float("-inf")
            mask[torch.arange(Nq), torch.arange(Nq) % N] = 0.0       # every row keeps a visible entry
        full = s if mask is None else s + mask
        p = ops.softmax_rows_(cu(s), cu(mask) if masked else None)
        within_baseline(f"softmax N={N} rows={lead}x{Nq} mask={masked}", p, torch.softmax(full.double(), -1), torch.softmax(full, -1))
        if masked:
            assert bool((p.cpu()[(mask == float("-inf")).expand_as(s)] == 0).all())
        assert_close("softmax row sums", p.sum(-1), torch.ones(lead, Nq), atol=1e-6, rtol=0)
        dp = rnd(lead, Nq, N, seed=82)
        ph = p.cpu()
        ds = ops.softmax_rows_bwd_(p, cu(dp))
        p64, d64 = ph.double(), dp.double()
        within_baseline(f"softmax bwd N={N} rows={lead}x{Nq}", ds, p64 * (d64 - (p64 * d64).sum(-1, keepdim=True)),
                        ph * (dp - (ph * dp).sum(-1, keepdim=True)))


def test_softmax_rows_refuses_more_than_1024_columns(ops):
    s = cu(rnd(2, 1025, seed=83))
    keep = s.clone()
    with pytest.raises(RuntimeError, match="mrn_softmax_rows_f32"):
        ops.softmax_rows_(s)
    with pytest.raises(RuntimeError, match="mrn_softmax_rows_bwd_f32"):
        ops.softmax_rows_bwd_(keep, s)
    torch.cuda.synchronize()
    assert torch.equal(s, keep)


@pytest.mark.parametrize("B,HW,C", [(1, 1, 4), (3, 26, 512), (2, 65, 100)])
def test_avgpool_bwd(ops, B, HW, C):
    """dx[b, p, c] = dy[b, c] / HW (the kernel multiplies by 1 / HW: measured 1.83 x the error of the fp32 division at most)"""
    dy = rnd(B, C, seed=90)
    dx = ops.avgpool_bwd(cu(dy), HW)
    assert dx.shape == (B, HW, C)
    within_baseline(f"avgpool_bwd {B}x{HW}x{C}", dx, (dy.double() / HW).unsqueeze(1).expand(B, HW, C), (dy / HW).unsqueeze(1).expand(B, HW, C))


@pytest.mark.parametrize("E", [100, 256])
@pytest.mark.parametrize("same", [False, True])
def test_embed_scatter_add(ops, E, same):
    """dtable[idx[b, s]] += demb[b, s]: indices repeated inside a sample and across samples (or all the same), idx a strided view
    (idx.stride(0) != S); the atomics reorder the sums, so 8 x the error of torch's fp32 index_add_ on the CPU (measured: 1.0 to 1.5)"""
    B, S, K = 5, 26, 41
    g = torch.Generator().manual_seed(95 + E)
    wide = torch.randint(0, 7, (B, S + 3), generator=g) * 5                    # 7 distinct rows: many repeats
    if same:
        wide.fill_(K - 1)
    wide[:, S:] = 0                                                            # (columns outside the view)
    idx = wide[:, :S]
    assert idx.stride(0) != S
    demb = rnd(B, S, E, seed=96)
    got = ops.embed_scatter_add(cu(wide)[:, :S], cu(demb), K)
    assert got.shape == (K, E)
    ref = torch.zeros(K, E, dtype=torch.float64).index_add_(0, idx.reshape(-1), demb.double().view(-1, E))
    base = torch.zeros(K, E).index_add_(0, idx.reshape(-1), demb.view(-1, E))
    within_baseline(f"embed_scatter_add E={E} same={same}", got, ref, base)
    untouched = torch.ones(K, dtype=torch.bool)
    untouched[idx.reshape(-1)] = False
    assert not bool(got.cpu()[untouched].any())


@pytest.mark.parametrize("O,I,kh,kw", [(5, 3, 3, 3), (64, 32, 2, 2), (128, 4, 1, 1)])
def test_weight_layout_kernels(ops, O, I, kh, kw):
    """pack_dgrad_weight: [O,kh,kw,I] -> [I,kh,kw,O] with both taps flipped; unpack_conv_weight: [O,kh,kw,I] -> [O,I,kh,kw], also
    accumulating onto a preloaded buffer -- exact"""
    w = rnd(O, kh, kw, I, seed=99)
    packed = ops.pack_dgrad_weight(cu(w))
    assert tuple(packed.shape) == (I, kh, kw, O)
    assert torch.equal(packed.ohwi.cpu(), w.flip(1, 2).permute(3, 1, 2, 0).contiguous())
    assert torch.equal(ops.unpack_conv_weight(cu(w)).cpu(), w.permute(0, 3, 1, 2).contiguous())
    pre = 3.0 + rnd(O, I, kh, kw, seed=100)
    buf = cu(pre)
    out = ops.unpack_conv_weight(cu(w), out=buf, accumulate=True)
    assert out is buf
    assert torch.equal(buf.cpu(), pre + w.permute(0, 3, 1, 2))
    out = ops.unpack_conv_weight(cu(w), out=buf, accumulate=False)
    assert torch.equal(buf.cpu(), w.permute(0, 3, 1, 2).contiguous())
