"""The yardsticks and the inputs of tests/test_loss_optim_gpu.py, proven without a GPU.

1. Every written-out float64 yardstick of tests/helpers.py (ce_reference, kd_reference, weight_align_reference, adam_ / sgd_ /
   adadelta_reference, ewc_reference) equals torch at the same float64 inputs: F.cross_entropy, the reference's _KD_loss expression,
   torch.optim.* after clip_grad_norm_, torch.norm.
2. The edge behaviour of torch the GPU tests rely on: cross-entropy with every row ignored, a distillation slice of one class.
3. The inputs discriminate: on every shape of the GPU lists (tests/loss_optim_cases.py) a deliberately WRONG fp32 variant of the
   yardstick misses float64 by at least 10 x the bound the GPU test applies to the kernel (helpers.baseline_bound: max(8 x the fp32
   baseline's error, 4 * 2^-24)) on at least one of the outputs that test compares.  Where a shape cannot tell a variant from the
   yardstick the test asserts exactly that, so the list of blind shapes is written down here and checked.
4. Every sample of the wide-class CTC cases is feasible."""
import pytest
import torch
import torch.nn.functional as F

from tests import loss_optim_cases as K
from tests.helpers import (baseline_bound, ce_reference, clip_reference, ewc_reference, kd_reference, rel_err, row_lse,
                           weight_align_reference)

MARGIN = 10.0


def rnd64(*shape, seed=0, scale=1.0):
    return K.rnd(*shape, seed=seed, scale=scale).double()


def close64(a, b, tol=1e-12):
    """float64 against float64: a few roundings of 2^-53, relative to max|b|"""
    return rel_err(a, b) <= tol


# ---------------------------------------------------------------------------------------------------------
# 1. the yardsticks are what torch computes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["none", "half", "all_but_one"])
@pytest.mark.parametrize("rows,C", [(1, 1), (1, 3), (255, 2), (257, 98), (31, 5374)])
def test_ce_reference_is_torch_cross_entropy(rows, C, pattern):
    c = K.ce_case(rows, C, pattern)
    x = c["logits"].double().requires_grad_(True)
    loss = F.cross_entropy(x, c["target"], ignore_index=c["ignore_index"])
    (c["upstream"] * loss).backward()
    assert close64(c["ref"][0], loss.detach()) and close64(c["ref"][1], x.grad)
    assert c["ref"][0].dtype == torch.float64 and c["base"][1].dtype == torch.float32


@pytest.mark.parametrize("c0,c1,C", K.KD_SLICES)
@pytest.mark.parametrize("T", K.KD_TEMPS)
def test_kd_reference_is_the_reference_kd_loss(c0, c1, C, T):
    rows = 50
    c = K.kd_case(c0, c1, C, rows, T)
    new, old = c["new"].double().requires_grad_(True), c["old"].double()
    pred, soft = new[:, c0:c1], old[:, c0:c1]                                   # (il_modules/lwf.py: _KD_loss on the old classes)
    loss = -1 * torch.mul(torch.softmax(soft / T, dim=1), torch.log_softmax(pred / T, dim=1)).sum() / pred.shape[0]
    (c["upstream"] * loss).backward()
    assert close64(c["ref"][0], loss.detach()) and close64(c["ref"][1], new.grad)
    assert c["ref"][1].shape == (rows, C)


@pytest.mark.parametrize("rows,n_old,C,ld", K.ALIGN_SHAPES[:5])
def test_weight_align_reference_is_torch_norm(rows, n_old, C, ld):
    w = K.align_case(rows, n_old, C, ld)["w"].double()
    gamma = torch.norm(w[:n_old], p=2, dim=1).mean() / torch.norm(w[n_old:], p=2, dim=1).mean()       # (modules/model.py weight_align)
    want = w.clone()
    want[n_old:] *= gamma
    got_gamma, got = weight_align_reference(w, n_old)
    assert close64(got_gamma, gamma) and close64(got, want)


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("name", list(K.OPTIMISERS))
def test_optimiser_references_are_torch_optim_after_clip_grad_norm(name, clipped):
    n = 1023
    c = K.opt_case(name, n, clipped)
    p = torch.nn.Parameter(c["p"].double())
    kw = K.OPTIMISERS[name]
    opt = {"adam": torch.optim.Adam, "adadelta": torch.optim.Adadelta}.get(name, torch.optim.SGD)([p], **kw)
    norms = []
    for g in c["grads"]:
        p.grad = g.double().clone()
        if clipped:
            norms.append(torch.nn.utils.clip_grad_norm_([p], c["max_norm"]))
        opt.step()
    ref, st = c["ref"], opt.state[p]
    assert close64(ref["p"], p.detach()) and close64(ref["g"], p.grad)
    if clipped:
        assert all(close64(a, b) for a, b in zip(ref["norms"], norms))
        assert all(float(k) < 1.0 for k in ref["coefs"])                         # clipping binds at every step
        assert not torch.equal(ref["g"], c["grads"][-1].double())
    else:
        assert torch.equal(ref["g"], c["grads"][-1].double())
    if name == "adam":
        assert close64(ref["m"], st["exp_avg"]) and close64(ref["v"], st["exp_avg_sq"])
    elif name == "adadelta":
        assert close64(ref["sq"], st["square_avg"]) and close64(ref["acc"], st["acc_delta"])
    elif name == "sgd_momentum":
        assert close64(ref["buf"], st["momentum_buffer"])
    else:
        assert not bool(ref["buf"].any())                                        # momentum 0: the buffer is never written
    moved = float((ref["p"] - c["p"].double()).abs().median() / c["p"].double().abs().median())
    assert 0.03 < moved < 3.0, moved                                             # three steps move p by about 0.1 |p| each


def test_clip_reference_leaves_a_small_gradient_alone():
    g = rnd64(1000, seed=1)
    norm, coef, out = clip_reference(g, 2 * float(g.norm()))
    assert float(coef) == 1.0 and torch.equal(out, g) and close64(norm, g.norm())
    p = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
    p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p], 0.3)
    assert close64(clip_reference(g, 0.3)[2], p.grad)


@pytest.mark.parametrize("binding", [True, False])
def test_ewc_reference_is_the_written_penalty_and_its_autograd(binding):
    c = K.ewc_case(10007, binding)
    g1, g2 = (g.double() for g in c["grads"])
    fisher = torch.min((g1 ** 2 + g2 ** 2) / 2, torch.tensor(c["fisher_max"], dtype=torch.float64))    # (il_modules/ewc.py)
    p = c["p"].double().requires_grad_(True)
    penalty = (fisher * (p - c["mean"].double()) ** 2).sum() / 2
    (K.EWC_COEF * penalty).backward()
    ref = c["ref"]
    assert close64(ref["fisher"], fisher) and close64(ref["penalty"], penalty.detach())
    assert close64(ref["grad"], c["grad0"].double() + p.grad)
    assert bool((fisher == c["fisher_max"]).any()) == binding
    same = ewc_reference(c["grads"], c["fisher_max"], c["p"], c["p"], K.EWC_COEF, c["grad0"], dtype=torch.float32)
    assert float(same["penalty"]) == 0.0 and torch.equal(same["grad"], c["grad0"])                    # p = mean: exactly nothing


# ---------------------------------------------------------------------------------------------------------
# 2. torch's behaviour at the edges
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("ignore_index", [1, -100])
def test_torch_cross_entropy_with_every_row_ignored(ignore_index, dtype):
    """the loss is NaN (0 / 0), the gradient all zero without a NaN in it; ce_reference has both"""
    x = K.rnd(7, 5, seed=2).to(dtype).requires_grad_(True)
    t = torch.full((7,), ignore_index)
    loss = F.cross_entropy(x, t, ignore_index=ignore_index)
    (15 * loss).backward()
    assert bool(torch.isnan(loss)) and not bool(torch.isnan(x.grad).any()) and not bool(x.grad.any())
    ref_loss, ref_d = ce_reference(x, t, ignore_index, 15.0, dtype=dtype)
    assert bool(torch.isnan(ref_loss)) and not bool(ref_d.any()) and ref_d.dtype == dtype


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_torch_kd_loss_on_a_slice_of_one_class(dtype):
    """softmax over one class is 1 and its logarithm 0: loss 0 and gradient 0, exactly"""
    new, old = K.rnd(9, 40, seed=3).to(dtype).requires_grad_(True), K.rnd(9, 40, seed=4).to(dtype)
    loss = -1 * torch.mul(torch.softmax(old[:, 5:6] / 2, dim=1), torch.log_softmax(new[:, 5:6] / 2, dim=1)).sum() / 9
    loss.backward()
    assert float(loss.detach()) == 0.0 and not bool(new.grad.any())
    ref_loss, ref_d = kd_reference(new, old, 5, 6, 2.0, dtype=dtype)
    assert float(ref_loss) == 0.0 and not bool(ref_d.any())


# ---------------------------------------------------------------------------------------------------------
# 3. the inputs discriminate
# ---------------------------------------------------------------------------------------------------------
def worst(pairs):
    """pairs of (wrong fp32 result, float64 reference, fp32 baseline) -> the largest error of the wrong result over the GPU test's
    bound for that output; a NaN or an infinity where the reference is finite counts as infinitely wrong"""
    out = 0.0
    for wrong, ref, base in pairs:
        wrong, ref, base = torch.as_tensor(wrong), torch.as_tensor(ref), torch.as_tensor(base)
        if not bool(torch.isfinite(wrong).all()):
            assert bool(torch.isfinite(ref).all())
            return float("inf")
        out = max(out, rel_err(wrong, ref) / baseline_bound(ref, base))
    return out


def untouched_past(cap, result, initial):
    """a launch that stops at the grid cap: the elements from `cap` on keep their initial values"""
    out = result.clone()
    out[cap:] = initial[cap:].to(out.dtype)
    return out


@pytest.mark.parametrize("binding", [True, False])
@pytest.mark.parametrize("n", K.EWC_SIZES)
def test_ewc_inputs_show_elements_dropped_past_the_grid_cap(n, binding):
    """cap = 2048 * 256: only n = 524 547 reaches past it; 1, 255 and 10 007 cannot tell (they fit in one pass of the grid)"""
    c = K.ewc_case(n, binding)
    ref, base, cap = c["ref"], c["base"], K.EWC_CAP
    zero = torch.zeros(n)
    d = c["p"][:cap] - c["mean"][:cap]
    wrong = [(untouched_past(cap, base["acc"], zero), ref["acc"], base["acc"]),
             (untouched_past(cap, base["fisher"], base["acc"]), ref["fisher"], base["fisher"]),
             ((base["fisher"][:cap] * d * d).sum() / 2, ref["penalty"], base["penalty"]),
             (untouched_past(cap, base["grad"], c["grad0"]), ref["grad"], base["grad"])]
    if n <= cap:
        assert all(torch.equal(torch.as_tensor(w), torch.as_tensor(b)) for w, _, b in wrong)
        return
    for one in wrong:                                        # every one of the four launches is caught on its own
        assert worst([one]) >= MARGIN, worst([one])


@pytest.mark.parametrize("rows,n_old,C,ld", K.ALIGN_SHAPES)
def test_align_inputs_show_a_partial_gamma_and_a_capped_scaling(rows, n_old, C, ld):
    """gamma from the first 256 norms only (the sums' loop not wrapping): told apart from 257 rows on -- (97, 70) and (2, 1) cannot.
    Scaling stopped at 2048 * 256 elements: only (5374, 3000, 256) has more new elements, (rows - n_old) * C = 607 744."""
    c = K.align_case(rows, n_old, C, ld)
    (g64, w64), (g32, w32) = c["ref"], c["base"]
    w = c["w"]
    norms = torch.sqrt((w * w).sum(1))
    head = norms[:256]
    gamma = (head[:n_old].sum() / n_old) / (head[n_old:].sum() / (rows - n_old))
    wrong = w.clone()
    wrong[n_old:] *= gamma
    if rows <= 256:
        assert torch.equal(gamma, g32)
    else:
        assert worst([(gamma, g64, g32)]) >= MARGIN and worst([(wrong, w64, w32)]) >= MARGIN
    cap, n_new = K.EWC_CAP, (rows - n_old) * C
    capped = w32.clone()
    capped[n_old:].view(-1)[cap:] = w[n_old:].reshape(-1)[cap:]
    if n_new <= cap:
        assert torch.equal(capped, w32)
    else:
        assert worst([(capped, w64, w32)]) >= MARGIN


@pytest.mark.parametrize("n", K.OPT_SIZES)
def test_norm_inputs_show_a_missing_tail(n):
    """the norm without the last n mod 4 elements (the scalar tail after the float4 loop): every size of the list has such a tail
    (cases.norm_input makes it 30 times larger than the other elements) and is told apart in the norm, the coefficient and the clipped gradient"""
    assert n % 4
    g, max_norm = K.norm_input(n), K.binding_max_norm(n)
    (n64, c64, g64), (n32, c32, g32) = clip_reference(g.double(), max_norm), clip_reference(g, max_norm)
    short = g.clone()
    short[n - n % 4:] = 0
    wn, wc, _ = clip_reference(short, max_norm)
    assert float(c64) < 1.0
    assert worst([(wn, n64, n32)]) >= MARGIN and worst([(wc, c64, c32)]) >= MARGIN and worst([(g * wc, g64, g32)]) >= MARGIN


def wrong_sgd(p, grads, max_norm, lr, momentum, weight_decay):
    """weight decay added after the momentum update instead of into it (fp32)"""
    p, buf = p.clone(), torch.zeros_like(p)
    for g in grads:
        g = clip_reference(g, max_norm)[2]
        d = g
        if momentum != 0:
            buf = momentum * buf + d
            d = buf
        p = p - lr * (d + weight_decay * p)
    return dict(p=p, g=g, buf=buf)


def wrong_adam(p, grads, max_norm, lr, betas=(0.9, 0.999), eps=1e-8):
    """the second moment's bias correction without its square root (fp32)"""
    p = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate(grads, 1):
        g = clip_reference(g, max_norm)[2]
        m = m + (g - m) * (1 - betas[0])
        v = v * betas[1] + (1 - betas[1]) * g * g
        p = p - lr / (1 - betas[0] ** step) * (m / (torch.sqrt(v) / (1 - betas[1] ** step) + eps))
    return dict(p=p, g=g, m=m, v=v)


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("n", K.OPT_SIZES)
@pytest.mark.parametrize("name", list(K.OPTIMISERS))
def test_update_inputs_show_the_wrong_updates(name, n, clipped):
    """elements past the cap of 4096 * 256 left as they were: only n = 1 049 347 reaches past it, the other four sizes cannot tell.
    SGD with the weight decay after the momentum update: told apart with momentum 0.9 at every size; with momentum 0 the two are
    the same formula.  Adam without the square root of the bias correction: told apart at every size."""
    c = K.opt_case(name, n, clipped)
    ref, base, cap = c["ref"], c["base"], K.UPDATE_CAP
    state = [k for k in ("m", "v", "buf", "sq", "acc") if k in ref and not (name == "sgd_plain" and k == "buf")]
    initial = dict(p=c["p"], g=c["grads"][-1], **{k: torch.zeros(n) for k in state})
    keys = ["p"] + (["g"] if clipped else []) + state
    for k in keys:                                           # every buffer shows the cap on its own
        capped = untouched_past(cap, base[k], initial[k])
        if n <= cap:
            assert torch.equal(capped, base[k])
        else:
            assert worst([(capped, ref[k], base[k])]) >= MARGIN
            assert bool((base[k][cap:] != initial[k][cap:]).all())              # (the GPU test's "has changed" check can hold)
    kw = K.OPTIMISERS[name]
    if name.startswith("sgd"):
        w = wrong_sgd(c["p"], c["grads"], c["max_norm"], **kw)
        if name == "sgd_plain":
            assert rel_err(w["p"], base["p"]) <= 2.0 ** -22                      # the same formula, rounded in another order
        else:
            assert worst([(w["p"], ref["p"], base["p"])]) >= MARGIN and worst([(w["buf"], ref["buf"], base["buf"])]) >= MARGIN
    if name == "adam":
        w = wrong_adam(c["p"], c["grads"], c["max_norm"], **kw)
        assert worst([(w["p"], ref["p"], base["p"])]) >= MARGIN


@pytest.mark.parametrize("pattern", K.CE_PATTERNS)
@pytest.mark.parametrize("rows,C", K.CE_SHAPES)
def test_ce_inputs_show_a_mean_over_all_rows(rows, C, pattern):
    """the loss and the gradient divided by the number of rows instead of the number of rows that count.  Cannot tell: nothing
    ignored ("none", and "half" / "all_but_one" at one row), and C = 1, where loss and gradient are zero whatever the divisor.
    Every row ignored: the wrong loss is 0 where the right one is NaN -- the GPU test asserts the NaN."""
    c = K.ce_case(rows, C, pattern)
    (l64, d64), (l32, d32) = c["ref"], c["base"]
    valid = rows - c["n_ignored"]
    assert c["n_ignored"] == {"none": 0, "half": rows // 2, "all_but_one": rows - 1, "all": rows}[pattern]
    if valid == 0:
        wrong_loss = torch.zeros(()) / rows                                      # the sum over no row, divided by all rows
        assert bool(torch.isnan(l64)) and not bool(torch.isnan(wrong_loss)) and not bool(d64.any())
        return
    wl, wd = l32 * (valid / rows), d32 * (valid / rows)
    if c["n_ignored"] == 0:
        assert torch.equal(wl, l32) and torch.equal(wd, d32)
    elif C == 1:
        assert not bool(l64) and not bool(d64.any()) and not bool(wl) and not bool(wd.any())
    else:
        assert worst([(wl, l64, l32)]) >= MARGIN and worst([(wd, d64, d32)]) >= MARGIN


@pytest.mark.parametrize("scale", K.CE_SWEEP_SCALES)
@pytest.mark.parametrize("C", K.CE_SWEEP_CLASSES)
def test_ce_sweep_inputs_show_a_mean_over_all_rows(C, scale):
    """the magnitude sweep's cases (312 rows, half ignored), against the bound WITH the derived term 2^-23 max|lse| the GPU test adds
    at +-30 and +-300.  The router's cases ignore nothing and cannot tell this variant."""
    c = K.ce_case(K.CE_SWEEP_ROWS, C, "half", float(scale))
    (l64, d64), (l32, d32) = c["ref"], c["base"]
    extra = 2.0 ** -23 * float(row_lse(c["logits"]).abs().max()) if scale > 4 else 0.0
    half = (c["rows"] - c["n_ignored"]) / c["rows"]
    assert rel_err(l32 * half, l64) >= MARGIN * baseline_bound(l64, l32, extra=extra / abs(float(l64)))
    assert rel_err(d32 * half, d64) >= MARGIN * baseline_bound(d64, d32, extra=extra)
    assert all(K.router_case(rows, I)["n_ignored"] == 0 for rows, I in K.ROUTER_SHAPES)


@pytest.mark.parametrize("scale", K.KD_SWEEP_SCALES)
@pytest.mark.parametrize("case", K.KD_SWEEP, ids=lambda s: "%d-%d-of-%d" % s[0])
def test_kd_sweep_inputs_show_a_missing_temperature_and_a_full_width_sum(case, scale):
    """the distillation sweep's cases against the bound with the derived term 2^-23 max(|lsa|, |lsb|) of +-30 and +-300"""
    (c0, c1, C), rows, T = case
    c = K.kd_case(c0, c1, C, rows, T, float(scale))
    (l64, d64), (l32, d32) = c["ref"], c["base"]
    extra = 0.0
    if scale > 3:
        extra = 2.0 ** -23 * max(float(row_lse(c["new"][:, c0:c1] / T).abs().max()), float(row_lse(c["old"][:, c0:c1] / T).abs().max()))
    full = kd_reference(c["new"], c["old"], 0, C, T, c["upstream"], dtype=torch.float32)[0]
    assert rel_err(full, l64) >= MARGIN * baseline_bound(l64, l32, extra=extra / abs(float(l64)))
    assert T == 2.0 and rel_err(d32 * T, d64) >= MARGIN * baseline_bound(d64, d32, extra=extra)


@pytest.mark.parametrize("T", K.KD_TEMPS)
@pytest.mark.parametrize("rows", K.KD_ROWS)
@pytest.mark.parametrize("c0,c1,C", K.KD_SLICES)
def test_kd_inputs_show_a_missing_temperature_and_a_full_width_sum(c0, c1, C, rows, T):
    """the gradient without its 1 / T: told apart at T = 2; T = 1 cannot tell, nor can the slice of one class (gradient zero).
    The loss summed over [0, C) instead of [c0, c1): every slice of the list is narrower than C and is told apart."""
    c = K.kd_case(c0, c1, C, rows, T)
    (l64, d64), (l32, d32) = c["ref"], c["base"]
    assert c1 - c0 < C
    full = kd_reference(c["new"], c["old"], 0, C, T, c["upstream"], dtype=torch.float32)[0]
    assert worst([(full, l64, l32)]) >= MARGIN
    wd = d32 * T
    if T == 1.0 or c1 - c0 == 1:
        assert torch.equal(wd, d32) or not bool(d64.any())
    else:
        assert worst([(wd, d64, d32)]) >= MARGIN
    assert not bool(d64[:, :c0].any()) and not bool(d64[:, c1:].any())
    if c1 - c0 == 1:
        assert float(l64) == 0.0 and not bool(d64.any())


# ---------------------------------------------------------------------------------------------------------
# 4. the CTC cases
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", K.CTC_WIDTHS)
@pytest.mark.parametrize("C", K.CTC_CLASSES)
def test_ctc_cases_are_feasible_and_reach_the_wide_classes(C, W):
    """length + adjacent repeats <= T for every sample (the infeasible branch belongs to test_width_gpu.py / test_cross_axes_gpu.py);
    classes >= 256 and repeats are present, also a repeat of a class >= 256; float64 F.ctc_loss is finite on every sample"""
    from mrn_amd.modules.label_length import ctc_uses_long_kernel
    c = K.ctc_case(C, W)
    assert ctc_uses_long_kernel(W) == (W == 40)
    wide_repeat = False
    for lab in c["labels"]:
        repeats = sum(a == b for a, b in zip(lab, lab[1:]))
        assert len(lab) + repeats <= K.CTC_T and len(lab) <= W and all(0 < v < C for v in lab)
        wide_repeat |= any(a == b and a >= 256 for a, b in zip(lab, lab[1:]))
    assert wide_repeat and any(max(lab) >= 256 for lab in c["labels"])
    lp = c["logits"].double().log_softmax(2).permute(1, 0, 2)
    nll = F.ctc_loss(lp, c["targets"], torch.IntTensor([K.CTC_T] * K.CTC_B), c["target_len"], blank=0, reduction="none")
    assert bool(torch.isfinite(nll).all())
