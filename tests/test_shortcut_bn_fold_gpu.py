"""The BatchNorm of a BasicBlock's 1x1 downsample shortcut folded into the block's closing pass (MRN_SHORTCUT_BN_FOLD, reference
modules/feature_extraction.py:171-197): the closing BatchNorm-apply kernels take the RAW downsample-conv output as their residual
plus its pending (scale, shift) and must give, bit for bit, what the separate apply pass over the branch followed by the plain closing
pass gives -- the same two fmas and the same add in the same order.  Every comparison here is on the bit patterns (NaNs included)."""
import pytest
import torch

from tests.test_kernels_gpu import cu, ops, rnd  # noqa: F401  (ops: the module-scoped fixture that loads the library)
from tests.test_width_gpu import CLASSES, build_mrn, inputs, recorded_calls

pytestmark = pytest.mark.gpu

FORMS = ("plain", "wino4", "wino2", "d16_fp16", "d16_bf16")


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def fma_f32(a, b, c):
    """fp32 fma(a, b, c) of CPU fp32 tensors, exactly: the product is exact in float64, the sum is taken in float64 with its rounding
    error (TwoSum) and rounded to odd, which makes the final rounding to fp32 that of the infinitely precise a * b + c"""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(torch.int64)
    even = (bits & 1) == 0
    away = (e > 0) == (s > 0)                                 # the exact sum lies further from zero than s
    step = torch.where(away, torch.ones_like(bits), -torch.ones_like(bits))
    bits = torch.where((e != 0) & even & (s != 0), bits + step, bits)
    return bits.view(torch.float64).float()


def closing_pass(ops, form, y, s, t, relu, **res):
    """the block's closing pass in one of its forms -> tuple of every output it writes"""
    if form == "plain":
        return ops.bn_apply_grouped(y.clone(), s, t, relu=relu, want_f32=True, want_hl=True, **res)
    if form in ("wino4", "wino2"):
        return ops.bn_apply_wino_grouped(y, s, t, int(form[-1]), relu=relu, want_f32=True, want_hl=True, dense=False, **res)
    saved = ops.REDUCED_BF16
    try:
        ops.REDUCED_BF16 = form == "d16_bf16"
        return ops.bn_apply_wino_grouped(y, s, t, 4, relu=relu, want_f32=True, want_hl=True, dense=True, **res)
    finally:
        ops.REDUCED_BF16 = saved


def operands(G, B, H, W, C, seed):
    y = cu(rnd(G, B, H, W, C, seed=seed, scale=2.0))
    y_ds = cu(rnd(G, B, H, W, C, seed=seed + 1, scale=3.0))
    s, s_ds = cu(rnd(G, C, seed=seed + 2) + 1.5), cu(rnd(G, C, seed=seed + 3) * 2.0)      # (s_ds of both signs)
    t, t_ds = cu(rnd(G, C, seed=seed + 4)), cu(rnd(G, C, seed=seed + 5))
    return y, y_ds, s, t, s_ds, t_ds


def two_pass_and_fused(ops, form, y, y_ds, s, t, s_ds, t_ds, relu):
    r, _ = ops.bn_apply_grouped(y_ds.clone(), s_ds, t_ds, relu=False, want_f32=True)
    two = closing_pass(ops, form, y, s, t, relu, residual=r)
    one = closing_pass(ops, form, y, s, t, relu, residual=y_ds, residual_affine=(s_ds, t_ds))
    torch.cuda.synchronize()
    return two, one


# ---- 1. the kernels: fused == two passes, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("G", [1, 6])
@pytest.mark.parametrize("form", FORMS)
def test_fused_residual_affine_is_the_two_pass_result(ops, form, G, C, relu):
    """W = 65: the last column group is ragged for R = 4 (one column) and R = 2 (one column); W = 64: every group full"""
    for W in (65, 64):
        B, H = 2, 4
        args = operands(G, B, H, W, C, seed=11 + W)
        two, one = two_pass_and_fused(ops, form, *args, relu)
        assert len(two) == len(one) == (2 if form == "plain" else 3)
        for k, (a, b) in enumerate(zip(two, one)):
            assert a is not None and same_bits(a, b), (form, G, C, relu, W, k)
        assert torch.isfinite(one[0]).all() and float(one[0].abs().max()) > 1.0      # (not a comparison of two empty results)


@pytest.mark.parametrize("form", FORMS)
def test_nan_and_inf_in_the_branch_propagate_as_before(ops, form):
    G, B, H, W, C = 2, 2, 4, 65, 128
    y, y_ds, s, t, s_ds, t_ds = operands(G, B, H, W, C, seed=5)
    y_ds[0, 0, 1, 3, 7] = float("nan")
    y_ds[1, 1, 2, 64, 100] = float("inf")
    y_ds[1, 0, 0, 0, 0] = float("-inf")
    for relu in (True, False):
        two, one = two_pass_and_fused(ops, form, y, y_ds, s, t, s_ds, t_ds, relu)
        for k, (a, b) in enumerate(zip(two, one)):
            assert same_bits(a, b), (form, relu, k)
        if not relu:
            assert torch.isnan(one[0][0, 0, 1, 3, 7]) and torch.isinf(one[0][1, 1, 2, 64, 100])


# ---- 2. the old entry points (null affine) ---------------------------------------------------------------------------------------
def test_old_entry_points_are_the_null_affine_path(ops):
    """mrn_bn_apply[_wino]_grouped[_d16]_f32 and their *_res_affine_* siblings with NULL affine vectors run one launcher: identical
    outputs; and the plain result still is relu(fma(y, s, t) + r), checked against an exact host evaluation (fma_f32)"""
    G, B, H, W, C = 6, 2, 4, 65, 128
    y, r, s, t, _, _ = operands(G, B, H, W, C, seed=3)
    p = ops._p
    st = ops._stream()
    rows = B * H * W

    def plain(name, *tail):
        o, hl = torch.empty_like(y), torch.empty(y.numel() * 4, device="cuda", dtype=torch.uint8)
        ops.call(name, p(y), p(r), None, p(s), p(t), p(o), p(hl), G, rows, C, 1, *tail, st)
        return o, hl

    def wino(name, R, *tail, eb=4):
        Wq = (W + R - 1) // R
        o, hl = torch.empty_like(y), torch.empty(y.numel() * 4, device="cuda", dtype=torch.uint8)
        v = torch.empty(G * B * H * Wq * (R + 2) * C * eb, device="cuda", dtype=torch.uint8)
        ops.call(name, p(y), p(r), None, p(s), p(t), p(o), p(hl), p(v), G, B, H, W, C, *tail, st)
        return o, hl, v
    pairs = [(plain("mrn_bn_apply_grouped_f32"), plain("mrn_bn_apply_grouped_res_affine_f32", None, None))]
    for R in (4, 2):
        pairs.append((wino("mrn_bn_apply_wino_grouped_f32", R, R, 1, None),
                      wino("mrn_bn_apply_wino_grouped_res_affine_f32", R, R, 1, None, None, None)))
    for bf16 in (0, 1):
        pairs.append((wino("mrn_bn_apply_wino_grouped_d16_f32", 4, 1, None, bf16, eb=2),
                      wino("mrn_bn_apply_wino_grouped_d16_res_affine_f32", 4, 1, None, bf16, None, None, eb=2)))
    torch.cuda.synchronize()
    for i, (old, new) in enumerate(pairs):
        for k, (a, b) in enumerate(zip(old, new)):
            assert same_bits(a, b), (i, k)
    yc = y.cpu()
    want = torch.relu(fma_f32(yc, s.cpu().view(G, 1, 1, 1, C).expand_as(yc), t.cpu().view(G, 1, 1, 1, C).expand_as(yc)) + r.cpu())
    for i, (old, _) in enumerate(pairs):                      # every form writes the same plain fp32 result
        assert same_bits(old[0].cpu(), want), i
    # the affine without the fp32 residual it belongs to is refused, by every entry point
    with pytest.raises(RuntimeError, match="residual affine"):
        o = torch.empty_like(y)
        ops.call("mrn_bn_apply_grouped_res_affine_f32", p(y), None, None, p(s), p(t), p(o), None, G, rows, C, 1, p(s), p(t), st)
    hl = ops.split_hl32(r)
    v = torch.empty(G * B * H * 17 * 6 * C * 4, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="residual affine"):
        ops.call("mrn_bn_apply_wino_grouped_res_affine_f32", p(y), None, p(hl), p(s), p(t), None, None, p(v), G, B, H, W, C, 4, 1, None,
                 p(s), p(t), st)
    torch.cuda.synchronize()


# ---- 3. the model: fold on == fold off ---------------------------------------------------------------------------------------------
def _expert_step(ops, net, sd, image, text_in, fold, reduced):
    from mrn_amd.modules import expert_group
    net.load_state_dict(sd, strict=True)                      # (the same running statistics before the step)
    saved = expert_group.SHORTCUT_BN_FOLD, ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS
    try:
        expert_group.SHORTCUT_BN_FOLD = fold
        if reduced:
            ops.X3_PRODUCTS = ops.TRAIN_PRODUCTS = 1          # bench.py --precision fp16: d16 closing passes, plain ones on 6-row maps
        with torch.no_grad():
            got = net.experts_prefetch(image, text_in, True)
        torch.cuda.synchronize()
    finally:
        expert_group.SHORTCUT_BN_FOLD, ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS = saved
    assert got is not None                                    # the lock-step path ran
    logits = [lg.clone() for part, _ in got["parts"] for lg in part]
    bufs = {k: v.detach().clone() for k, v in net.state_dict().items() if "running_" in k or "num_batches_tracked" in k}
    return got["feats"].clone(), logits, bufs


@pytest.mark.parametrize("imgH,imgW,mixed,reduced", [(32, 256, False, False), (32, 256, True, False), (48, 320, False, False),
                                                      (48, 320, False, True)])
def test_trba3_train_forward_with_and_without_the_fold(ops, imgH, imgW, mixed, reduced):
    """mixed: every bn2 of the downsample blocks in eval mode -- the closing pass applies a running-statistics affine to its own input
    and the batch-statistics affine of the branch to its residual"""
    B = 4
    opt, net, sd = build_mrn("trba", imgH, imgW, CLASSES["trba"], 29)
    net.train()
    if mixed:
        for e in net.model:
            cn = e.model.FeatureExtraction.ConvNet
            for name in ("layer1", "layer2", "layer3"):
                getattr(cn, name)[0].bn2.eval()
    image, tgt, _ = inputs("trba", imgH, imgW, B, CLASSES["trba"], 29)
    image, text_in = image.cuda(), tgt[:, :-1].cuda()
    f1, l1, b1 = _expert_step(ops, net, sd, image, text_in, True, reduced)
    f0, l0, b0 = _expert_step(ops, net, sd, image, text_in, False, reduced)
    assert torch.isfinite(f1).all() and same_bits(f1, f0)
    assert len(l1) == len(l0) == 3
    for a, b in zip(l1, l0):
        assert same_bits(a, b)
    ds = [k for k in b1 if ".downsample.1.running_" in k]
    assert len(ds) == 3 * 3 * 2                               # three experts x three downsample BatchNorms x (mean, var)
    for k in b1:
        assert torch.equal(b1[k], b0[k]), k
    for k in ds:
        assert not torch.equal(b1[k], sd[k].cuda())           # ... and the statistics were updated


# ---- 4. the fold is taken ------------------------------------------------------------------------------------------------------------
PLAIN = ("mrn_bn_apply_grouped_f32", "mrn_bn_apply_grouped_res_affine_f32")
WINO = ("mrn_bn_apply_wino_grouped_f32", "mrn_bn_apply_wino_grouped_res_affine_f32", "mrn_bn_apply_wino_grouped_d16_f32",
        "mrn_bn_apply_wino_grouped_d16_res_affine_f32")


@pytest.mark.parametrize("imgH,imgW,reduced", [(32, 256, False), (48, 320, False), (48, 320, True)])
def test_expert_forward_drops_three_apply_launches(ops, imgH, imgW, reduced):
    """one lock-step expert forward: three launches of the plain BatchNorm-apply kernel fewer with the fold (the downsample branches
    of layer1 / layer2 / layer3), every other entry point called as often as without.  The three closing passes that carry the pending
    affine are Winograd-form in the parity mode; in the reduced mode at imgH = 48 the 6-row map of layer3 cannot take the plain-fp16
    Winograd form, so its closing pass is the plain one -- a launch that moves from mrn_bn_apply_grouped_f32 to its *_res_affine_*
    sibling, which is why the plain kernel's launches are counted over both names"""
    from collections import Counter
    from mrn_amd.modules import expert_group
    opt, net, sd = build_mrn("trba", imgH, imgW, CLASSES["trba"], 31)
    net.train()
    image, _, _ = inputs("trba", imgH, imgW, 2, CLASSES["trba"], 31)
    group = expert_group.BackboneGroup([e.model for e in net.model])
    counts = {}
    saved = expert_group.SHORTCUT_BN_FOLD, ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS
    try:
        if reduced:
            ops.X3_PRODUCTS = ops.TRAIN_PRODUCTS = 1          # bench.py --precision fp16
        for fold in (True, False):
            expert_group.SHORTCUT_BN_FOLD = fold
            with torch.no_grad():
                group.visual_all(image.cuda())                # (weights packed, caches warm: the recorded pass is a steady-state one)
                with recorded_calls() as log:
                    group.visual_all(image.cuda())
            torch.cuda.synchronize()
            counts[fold] = Counter(n for n, _ in log)
    finally:
        expert_group.SHORTCUT_BN_FOLD, ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS = saved
    on, off = counts[True], counts[False]
    plain_on, plain_off = sum(on[n] for n in PLAIN), sum(off[n] for n in PLAIN)
    assert plain_on == plain_off - 3, (plain_on, plain_off)
    assert sum(on[n] for n in WINO) == sum(off[n] for n in WINO) > 0
    affine = [n for n in on if "res_affine" in n]
    assert sum(on[n] for n in affine) == 3 and not any("res_affine" in n for n in off)
    if not reduced:
        assert on["mrn_bn_apply_grouped_f32"] == off["mrn_bn_apply_grouped_f32"] - 3
        assert on["mrn_bn_apply_wino_grouped_res_affine_f32"] == 3
    else:
        assert on["mrn_bn_apply_grouped_res_affine_f32"] >= 1 and on["mrn_bn_apply_wino_grouped_d16_res_affine_f32"] >= 1
    rest_on = {n: c for n, c in on.items() if n not in PLAIN + WINO}
    rest_off = {n: c for n, c in off.items() if n not in PLAIN + WINO}
    assert rest_on == rest_off                                # convolutions, finalize, pooling, TPS ...: the same calls
    assert on["mrn_bn_finalize_grouped_f32"] > 0 and any(n.startswith("mrn_conv") for n in rest_on)


# ---- 5. what the deferred form refuses -----------------------------------------------------------------------------------------------
def test_defer_affine_refuses_what_it_cannot_carry(ops):
    from mrn_amd.modules import expert_group
    opt, net, sd = build_mrn("trba", 32, 128, CLASSES["trba"], 37)
    net.train()
    group = expert_group.BackboneGroup([e.model for e in net.model])
    blocks = [e.model.FeatureExtraction.ConvNet.layer1[0] for e in net.model]
    convs, bns = [b.downsample[0] for b in blocks], [b.downsample[1] for b in blocks]
    G, B, H, W, C = 3, 2, 16, 64, convs[0].in_channels
    x = expert_group.Act((G, B, H, W, C), cu(rnd(G, B, H, W, C, seed=1)), None)
    ok = dict(relu=False, want_f32=True, want_hl=False)
    bad = [dict(ok, relu=True), dict(ok, want_hl=True), dict(ok, want_f32=False), dict(ok, want_wino=4), dict(ok, height_mean=True),
           dict(ok, pool=((2, 2), (2, 2), (0, 0))), dict(ok, gelu=True), dict(ok, residual=x)]
    with recorded_calls() as log, torch.no_grad():
        for kw in bad:
            with pytest.raises(ValueError, match="defer_affine"):
                group.layer(x, convs, bns, defer_affine=True, **kw)
        with pytest.raises(ValueError, match="defer_affine"):
            group.layer(x, convs, None, defer_affine=True, **ok)
    assert log == []                                          # refused before any launch
    with torch.no_grad():
        got = group.layer(x, convs, bns, defer_affine=True, **ok)
        ref = group.layer(x, convs, bns, **ok)
    torch.cuda.synchronize()
    assert got.affine is not None and ref.affine is None and got.hl is None
    done, _ = ops.bn_apply_grouped(got.f32.clone(), got.affine[0], got.affine[1], relu=False, want_f32=True)
    # (the second call's statistics are the first's: same input, and the affine does not depend on the running buffers)
    assert same_bits(done, ref.f32)
    # a consumer that cannot take the pending affine -- conv2 behind an eval-mode BatchNorm on the plain operand is ONE launch with
    # the BatchNorm in the conv epilogue -- gets the materialised branch: same result as with the two-pass shortcut
    for b in blocks:
        b.bn2.eval()
    with torch.no_grad():
        mid = group.layer(x, [b.conv1 for b in blocks], [b.bn1 for b in blocks], want_hl=True)
        close = dict(relu=True, want_f32=True, want_hl=True)
        with recorded_calls() as log:
            a = group.layer(mid, [b.conv2 for b in blocks], [b.bn2 for b in blocks], residual=got, **close)
        b_ = group.layer(mid, [b.conv2 for b in blocks], [b.bn2 for b in blocks], residual=ref, **close)
    torch.cuda.synchronize()
    assert [n for n, _ in log if "bn_apply" in n] == ["mrn_bn_apply_grouped_f32"] and got.affine is None
    assert same_bits(got.f32, ref.f32) and same_bits(a.f32, b_.f32) and same_bits(a.hl, b_.hl)
