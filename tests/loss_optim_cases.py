"""Shapes and inputs shared by test_loss_optim_cpu.py (which proves that they discriminate) and test_loss_optim_gpu.py (which runs
the kernels on them).  Every input is fp32, made on the CPU from a seeded generator, and cached: the float64 references built on
them are computed once."""
import functools

import torch

from tests.helpers import (adadelta_reference, adam_reference, ce_reference, ewc_reference, kd_reference, sgd_reference,
                           weight_align_reference)

EWC_CAP = 2048 * 256               # opt_grid of optim.hip: EWC and weight alignment loop grid-stride past this many elements
UPDATE_CAP = 4096 * 256            # the block cap of the three updates; also the norm's 1024 blocks x 256 threads x 4 floats


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


# ---------------------------------------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------------------------------------
CE_CLASSES = [1, 2, 3, 16, 98, 255, 256, 257, 5374]
CE_ROWS = [1, 255, 257]
CE_BIG = (6657, 40)                # 256 * 26 + 1 rows: ce_finalize_kernel's loop wraps 26 times and one lane takes a 27th row
CE_PATTERNS = ["none", "half", "all_but_one", "all"]
CE_SHAPES = [(r, c) for c in CE_CLASSES for r in CE_ROWS] + [CE_BIG]
CE_SWEEP_ROWS, CE_SWEEP_CLASSES, CE_SWEEP_SCALES = 312, [3, 98, 5374], [4, 30, 300]
ROUTER_SHAPES = [(r, i) for i in (1, 3, 16) for r in (1, 257)]


@functools.lru_cache(maxsize=None)
def ce_case(rows, C, pattern, scale=4.0, upstream=15.0):
    """logits uniform in +-scale, targets over all classes.  The ignored rows carry ignore_index = 1 (the [PAD] class of the
    attention head) when there are at least three classes, else -100; "none" uses -100 with every target in range, the router's
    call.  "half": rows // 2 rows drawn at random, "all_but_one": every row but row rows // 3 (one row: nothing is ignored in
    either), "all": every row."""
    g = torch.Generator().manual_seed(7000 + 31 * rows + C + len(pattern))
    logits = rnd(rows, C, seed=70) * scale
    ignore_index = 1 if (C >= 3 and pattern != "none") else -100
    if ignore_index == 1:
        target = torch.randint(0, C - 1, (rows,), generator=g)
        target[target >= 1] += 1
    else:
        target = torch.randint(0, C, (rows,), generator=g)
    ignored = torch.zeros(rows, dtype=torch.bool)
    if pattern == "half":
        ignored[torch.randperm(rows, generator=g)[:rows // 2]] = True
    elif pattern == "all_but_one":
        ignored[:] = rows > 1
        ignored[rows // 3] = False
    elif pattern == "all":
        ignored[:] = True
    target[ignored] = ignore_index
    ref = ce_reference(logits, target, ignore_index, upstream)
    base = ce_reference(logits, target, ignore_index, upstream, dtype=torch.float32)
    return dict(rows=rows, C=C, pattern=pattern, logits=logits, target=target, ignore_index=ignore_index, upstream=upstream,
                n_ignored=int(ignored.sum()), ref=ref, base=base)


@functools.lru_cache(maxsize=None)
def router_case(rows, I):
    """the router's loss (il_modules/mrn.py): CrossEntropyLoss on the softmaxed expert weights in [0, 1], C = I, int64 domain labels"""
    logits = torch.softmax(rnd(rows, I, seed=71) * 3, 1)
    target = torch.randint(0, I, (rows,), generator=torch.Generator().manual_seed(7100 + rows + I))
    return dict(rows=rows, C=I, logits=logits, target=target, ignore_index=-100, upstream=1.0, n_ignored=0,
                ref=ce_reference(logits, target), base=ce_reference(logits, target, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------
# CTC at wide class counts: B = 3, T = 12; every sample is feasible (length + repeats <= T)
# ---------------------------------------------------------------------------------------------------------
CTC_B, CTC_T = 3, 12
CTC_CLASSES = [300, 600]
CTC_WIDTHS = [5, 40]               # the 64-state kernel; the long kernel with two states per lane


@functools.lru_cache(maxsize=None)
def ctc_case(C, W):
    logits = rnd(CTC_B, CTC_T, C, seed=72) * 3
    if W == 5:
        labels = [[C - 1, C - 1, 7, 256, 299], [2, 260, 2], [255, 256, 256, 3]]
    else:
        labels = [[C - 1, 258, 258, 9, 300 % C + 2, 4, 4, 270, 5], [C - 2, 6, 257, 257], [2, 3, 256, 280, 280, C - 1]]
    targets = torch.ones(CTC_B, W, dtype=torch.int64)
    for b, lab in enumerate(labels):
        targets[b, :len(lab)] = torch.tensor(lab)
    tl = torch.tensor([len(lab) for lab in labels], dtype=torch.int32)
    return dict(C=C, W=W, logits=logits, labels=labels, targets=targets, target_len=tl)


# ---------------------------------------------------------------------------------------------------------
# knowledge distillation
# ---------------------------------------------------------------------------------------------------------
KD_SLICES = [(0, 70, 97), (1, 70, 97), (1, 97, 97), (5, 6, 40), (0, 700, 1000), (300, 999, 1001)]
KD_ROWS = [1, 50, 257, 1000]
KD_TEMPS = [1.0, 2.0]
KD_SWEEP = [((1, 70, 97), 50, 2.0), ((300, 999, 1001), 50, 2.0)]
KD_SWEEP_SCALES = [3, 30, 300]


@functools.lru_cache(maxsize=None)
def kd_case(c0, c1, C, rows, T, scale=3.0, upstream=3.0):
    new, old = rnd(rows, C, seed=73) * scale, rnd(rows, C, seed=74) * scale
    return dict(c0=c0, c1=c1, C=C, rows=rows, T=T, new=new, old=old, upstream=upstream,
                ref=kd_reference(new, old, c0, c1, T, upstream), base=kd_reference(new, old, c0, c1, T, upstream, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------
# EWC
# ---------------------------------------------------------------------------------------------------------
EWC_SIZES = [1, 255, 10007, EWC_CAP + 256 + 3]
EWC_COEF = 1000.0


@functools.lru_cache(maxsize=None)
def ewc_case(n, binding):
    """two gradients of about 0.02 (their squares: 4e-4 at most), fisher_max 1e-4 (binding for about half of the elements) or 1.0"""
    g1, g2 = rnd(n, seed=75) * 0.02, rnd(n, seed=76) * 0.02
    p, mean, grad0 = rnd(n, seed=77), rnd(n, seed=78), rnd(n, seed=79) * 0.05
    fisher_max = 1e-4 if binding else 1.0
    ref = ewc_reference([g1, g2], fisher_max, p, mean, EWC_COEF, grad0)
    base = ewc_reference([g1, g2], fisher_max, p, mean, EWC_COEF, grad0, dtype=torch.float32)
    return dict(n=n, grads=[g1, g2], p=p, mean=mean, grad0=grad0, fisher_max=fisher_max, ref=ref, base=base)


# ---------------------------------------------------------------------------------------------------------
# weight alignment: (rows, n_old, C, ld)
# ---------------------------------------------------------------------------------------------------------
ALIGN_SHAPES = [(97, 70, 256, 256), (2, 1, 4, 4), (300, 299, 100, 100), (300, 1, 100, 128), (513, 256, 64, 64), (5374, 3000, 256, 256)]


@functools.lru_cache(maxsize=None)
def align_case(rows, n_old, C, ld):
    """the new rows are about three times as long as the old ones, and every row has its own length (factor 0.5 to 1.5)"""
    w = rnd(rows, C, seed=80) * (1.0 + 0.5 * rnd(rows, 1, seed=81))
    w[n_old:] *= 3.0
    return dict(rows=rows, n_old=n_old, C=C, ld=ld, w=w, ref=weight_align_reference(w, n_old),
                base=weight_align_reference(w, n_old, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------
# gradient norm and the three updates
# ---------------------------------------------------------------------------------------------------------
OPT_SIZES = [1, 3, 1023, 100003, UPDATE_CAP + 768 + 3]
OPT_STEPS = 3
OPTIMISERS = {                     # learning rates that move a parameter by about 0.1 |p| per step
    "adam": dict(lr=0.1),
    "sgd_momentum": dict(lr=0.1, momentum=0.9, weight_decay=1e-3),
    "sgd_plain": dict(lr=0.1, momentum=0.0, weight_decay=1e-3),
    "adadelta": dict(lr=30.0),
}


@functools.lru_cache(maxsize=None)
def opt_inputs(n):
    """p uniform in +-1 and one gradient per step uniform in +-1 (times 1, 2, 3), none of them near zero"""
    p = rnd(n, seed=82)
    p[p.abs() < 0.05] = 0.5
    grads = []
    for k in range(OPT_STEPS):
        g = rnd(n, seed=83 + k) * (k + 1)
        g[g.abs() < 0.05 * (k + 1)] = 0.25 * (k + 1)
        grads.append(g)
    return p, grads


@functools.lru_cache(maxsize=None)
def norm_input(n):
    """the gradient of the norm tests: the first step's, with the last n mod 4 elements -- the ones only the norm kernel's scalar tail
    reads -- 30 times larger where the float4 loop has anything to read at all, so that a norm without them is visibly short.  (The
    update tests keep the plain gradients: three outliers would set the scale every error is measured against.)"""
    g = opt_inputs(n)[1][0].clone()
    if n > 4 and n % 4:
        g[n - n % 4:] *= 30.0
    return g


def opt_reference(name, p, grads, max_norm, dtype=torch.float64):
    kw = OPTIMISERS[name]
    fn = {"adam": adam_reference, "adadelta": adadelta_reference}.get(name, sgd_reference)
    return fn(p, grads, max_norm, dtype=dtype, **kw)


def binding_max_norm(n):
    """0.7 x the first gradient's norm: clipping binds at every step (the later gradients are larger)"""
    return 0.7 * float(opt_inputs(n)[1][0].double().norm())


@functools.lru_cache(maxsize=2)
def opt_case(name, n, clipped):
    p, grads = opt_inputs(n)
    max_norm = binding_max_norm(n) if clipped else None
    return dict(name=name, n=n, p=p, grads=grads, max_norm=max_norm, ref=opt_reference(name, p, grads, max_norm),
                base=opt_reference(name, p, grads, max_norm, dtype=torch.float32))


FLAT_ADAM_NUMELS = [5, 130, UPDATE_CAP + 1]       # views padded to 8, 132: the third one starts at 140 and crosses the cap
