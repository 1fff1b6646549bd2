"""Shapes and inputs shared by test_router_kernels_cpu.py (which proves the yardsticks and that the inputs discriminate) and
test_router_kernels_gpu.py (which runs rowops.hip, router.hip and DMRouterFn on them).  Every input is fp32, made on the CPU from a
seeded generator, and cached with its float64 reference and fp32 baseline (tests/helpers.py): both are computed once."""
import functools

import torch

from tests.helpers import (colnorm_reference, dm_router_reference, fanin_reference, gate_tail_reference, gelu_grad_reference,
                           gelu_reference, layernorm_reference)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def both(fn, *a, **k):
    """(float64 reference, fp32 baseline) of a yardstick"""
    return fn(*a, **k, dtype=torch.float64), fn(*a, **k, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------
# LayerNorm over the last dim: one wave per row, lane l holds float4 l, l + 64, l + 128, l + 192 of the row
# ---------------------------------------------------------------------------------------------------------
LN_C = [4, 252, 256, 260, 512, 1024]          # most lanes idle; one short of / exactly / one past one float4 per lane; two trips; all four
LN_ROWS = [1, 3, 5, 65]
LN_BIG_ROWS = 65537                           # backward: 1024 blocks of 65 rows, blocks 1009 .. 1023 own no row
LN_BIG_C = [4, 256]
LN_KINDS = ["unit", "offset", "const"]
LN_EPS = [1e-5, 1e-6]
LN_HL_C = [32, 256, 1024]
LN_SHAPES = [(r, c) for c in LN_C for r in LN_ROWS] + [(LN_BIG_ROWS, c) for c in LN_BIG_C]


@functools.lru_cache(maxsize=None)
def ln_case(rows, C, kind="unit", eps=1e-5):
    """x uniform in +-1; "offset": every row moved by 1000 (a one-pass variance E[x^2] - mean^2 loses everything there); "const": row
    rows // 2 is 0.75 throughout (variance exactly 0: rstd = 1 / sqrt(eps), dx finite)"""
    x = rnd(rows, C, seed=100 + len(kind))
    if kind == "offset":
        x = x + 1000.0
    elif kind == "const":
        x[rows // 2] = 0.75
    gamma, beta, dy = rnd(C, seed=101) * 0.5 + 1.2, rnd(C, seed=102), rnd(rows, C, seed=103)
    ref, base = both(layernorm_reference, x, gamma, beta, eps, dy)
    return dict(rows=rows, C=C, kind=kind, eps=eps, x=x, gamma=gamma, beta=beta, dy=dy, ref=ref, base=base)


# ---------------------------------------------------------------------------------------------------------
# column norm: one thread per (b, w) column, 256 columns per block
# ---------------------------------------------------------------------------------------------------------
COLNORM_SHAPES = [(1, 256, 3), (2, 4, 1), (31, 255, 3), (65, 257, 1), (2, 257, 3), (129, 4096, 3)]       # (P, Wd, B)


@functools.lru_cache(maxsize=None)
def colnorm_case(P, Wd, B, eps=1e-5):
    x, dy, dx0 = rnd(B, P, Wd, seed=110), rnd(B, P, Wd, seed=111), rnd(B, P, Wd, seed=112)
    gamma, beta = rnd(P, seed=113) * 0.5 + 1.2, rnd(P, seed=114)
    ref, base = both(colnorm_reference, x, gamma, beta, eps, dy)
    return dict(P=P, Wd=Wd, B=B, eps=eps, x=x, dy=dy, dx0=dx0, gamma=gamma, beta=beta, ref=ref, base=base)


# ---------------------------------------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------------------------------------
EW_SHAPES = [(1, 4), (5, 252), (300, 512)]
EW_GRID = [1.0, -1.0, 6.0, -6.0, 0.0, -0.0, 1e-30, -1e-30, 1e-3, -1e-3, 40.0, -40.0]
EW_SPECIALS = [float("inf"), float("-inf"), float("nan"), 1.0]


@functools.lru_cache(maxsize=None)
def ew_case(rows, C):
    """a: the grid first (as much of it as the shape holds), then uniform in +-3; b uniform in +-1; d: one DropPath scale per group of
    rows (groups of 1 row at rows <= 5, of 100 rows otherwise)"""
    n = rows * C
    a = (rnd(n, seed=120) * 3)
    k = min(n, len(EW_GRID))
    a[:k] = torch.tensor(EW_GRID[:k])
    a, b = a.view(rows, C), rnd(rows, C, seed=121)
    per = 1 if rows <= 5 else 100
    d = (rnd(rows // per, seed=122) > 0).float() / 0.9
    return dict(rows=rows, C=C, a=a, b=b, d=d, rows_per_d=per)


def ew_reference(op, a, b=None, d=None, rows_per_d=1, dtype=torch.float64):
    """op: "gelu", "gelu_bwd" (b * gelu'(a)), "mul", "add", "residual" (a + b * d[row // rows_per_d])"""
    a = a.detach().to(dtype)
    b = None if b is None else b.detach().to(dtype)
    if op == "gelu":
        return gelu_reference(a, dtype)
    if op == "gelu_bwd":
        return b * gelu_grad_reference(a, dtype)
    if op == "mul":
        return a * b
    if op == "add":
        return a + b
    assert op == "residual"
    return a + b * d.detach().to(dtype).repeat_interleave(rows_per_d).view(-1, 1)


# ---------------------------------------------------------------------------------------------------------
# token permutation / spatial projection
# ---------------------------------------------------------------------------------------------------------
PERM_SHAPES = [(31, 1), (31, 3), (33, 2), (65, 8)]        # (P, I): N = 31 (identity), 93 (ldw 96), 66 (ldw 68), 520
SPATIAL_B, SPATIAL_C = [1, 3], [128, 256]


def token_perm(P, I):
    """perm[p * I + d] = d * P + p (functional.token_permutation) and its inverse, int32, on the CPU"""
    idx = torch.arange(P * I, dtype=torch.int32)
    perm = (idx % I) * P + idx // I
    inv = torch.empty_like(perm)
    inv[perm.long()] = idx
    return perm, inv


@functools.lru_cache(maxsize=None)
def spatial_case(P, I, B, C):
    """vp[b] = Wsp' vn[b] + bsp'[:, None] and dvn[b] = Wsp'^T dvp[b], Wsp' = Wsp[perm][:, perm] (what DMRouterFn issues to gemm_raw)"""
    N = P * I
    wsp, bsp = rnd(N, N, seed=130) / N ** 0.5, rnd(N, seed=131)
    vn, dvp = rnd(B, N, C, seed=132), rnd(B, N, C, seed=133)
    perm, _ = token_perm(P, I)
    pl = perm.long()

    def fwd(dtype):
        w = wsp.to(dtype)[pl][:, pl]
        return torch.einsum("nm,bmc->bnc", w, vn.to(dtype)) + bsp.to(dtype)[pl].view(1, N, 1)

    def bwd(dtype):
        return torch.einsum("nm,bnc->bmc", wsp.to(dtype)[pl][:, pl], dvp.to(dtype))
    return dict(P=P, I=I, B=B, C=C, N=N, wsp=wsp, bsp=bsp, vn=vn, dvp=dvp, perm=perm, ref=(fwd(torch.float64), bwd(torch.float64)),
                base=(fwd(torch.float32), bwd(torch.float32)))


# ---------------------------------------------------------------------------------------------------------
# gate tail
# ---------------------------------------------------------------------------------------------------------
GATE_I, GATE_B, GATE_P, GATE_BETA = [1, 2, 8], [1, 63, 64, 65], [1, 31, 129], [1.0, 5.0]
GATE_SHAPES = [(i, b, p, beta) for i in GATE_I for b in GATE_B for p in GATE_P for beta in GATE_BETA]
GATE_SATURATED = (8, 65, 31, 5.0)             # with r scaled so that |beta * s| reaches about 200


@functools.lru_cache(maxsize=None)
def gate_case(I, B, P, beta, r_scale=1.0):
    r = rnd(B, P, I, seed=140) * r_scale
    Wr, br, dw = rnd(P, seed=141) * 0.3, rnd(1, seed=142), rnd(B, I, seed=143)
    ref, base = both(gate_tail_reference, r, Wr, br, beta, dw)
    w_free = rnd(B, I, seed=144) * 0.5 + 0.6          # weights in 0.1 .. 1.1 that are no softmax: sum(ds) is not zero, dbr a real number
    free_ref, free_base = both(gate_tail_reference, r, Wr, br, beta, dw, w=w_free)
    return dict(I=I, B=B, P=P, beta=beta, r=r, Wr=Wr, br=br, dw=dw, ref=ref, base=base, w_free=w_free, free_ref=free_ref,
                free_base=free_base)


def saturated_gate_case():
    """r in +-18: s is a sum of 31 terms of standard deviation 0.173 * 10.4, its largest of 520 about 3 sigma = 40, so beta * s reaches
    about 200 (the CPU test checks the range) and exp(beta * (s - max)) underflows to zero for more than a quarter of the weights"""
    I, B, P, beta = GATE_SATURATED
    return gate_case(I, B, P, beta, r_scale=18.0)


@functools.lru_cache(maxsize=None)
def tie_case(I, B, P):
    """hard routing on exact ties: in sample b the columns i0 = b % (I - 1) and i1 = i0 + 1 + (b % (I - 1 - i0)) are the same numbers, so
    their scores are the same bits in any precision, and they are the maximum: Wr[p] * col[p] = |Wr[p]| * (2 + |r|) >= 2 |Wr[p]|, where
    every other column has |Wr[p] r| <= |Wr[p]|.  Expected index: i0, in EVERY sample."""
    assert I >= 2
    r = rnd(B, P, I, seed=150)
    Wr, br = rnd(P, seed=151) * 0.3, rnd(1, seed=152)
    want = torch.empty(B, dtype=torch.int64)
    for b in range(B):
        i0 = b % (I - 1)
        i1 = i0 + 1 + (b % (I - 1 - i0))
        col = torch.sign(Wr) * (2.0 + r[b, :, i0].abs())
        r[b, :, i0] = col
        r[b, :, i1] = col
        want[b] = i0
    return dict(I=I, B=B, P=P, r=r, Wr=Wr, br=br, want=want)


# ---------------------------------------------------------------------------------------------------------
# fan-in / select-expert
# ---------------------------------------------------------------------------------------------------------
FANIN_I = [1, 3, 8]
FANIN_NEWEST = [5, 1023, 1024, 1025, 5374]
FANIN_BT = [(1, 1), (5, 26)]
FANIN_SHAPES = [(i, c, b, t) for i in FANIN_I for c in FANIN_NEWEST for b, t in FANIN_BT]
FANIN_BIG = (2, (3, 5), 256, 256)             # 65536 rows: one more than a launch may have in grid.y


def fanin_classes(I, C):
    """ragged class counts growing to C; every older one is no multiple of 4"""
    out = []
    for i in range(I - 1):
        c = max(1, C * (i + 1) // I)
        out.append(c - 1 if c % 4 == 0 else c)
    return tuple(out) + (C,)


@functools.lru_cache(maxsize=None)
def fanin_case(I, classes, B, T):
    C = classes[-1]
    logits = [rnd(B, T, c, seed=160 + i) * 3 for i, c in enumerate(classes)]
    w = torch.softmax(rnd(B, I, seed=170) * 2, 1)
    dout = rnd(B, T, C, seed=171)
    index = (torch.arange(B) * 5 + 1) % I
    ref, base = both(fanin_reference, logits, w, dout)
    return dict(I=I, classes=classes, B=B, T=T, C=C, logits=logits, w=w, dout=dout, index=index, ref=ref, base=base)


def select_reference(logits, index):
    """hard routing: sample b takes expert index[b]'s logits, padded to the newest class count with ones; an index outside 0 .. I - 1
    gives the row of ones"""
    C = logits[-1].shape[-1]
    B, T = logits[0].shape[:2]
    out = torch.ones(B, T, C)
    for b, i in enumerate(index.tolist()):
        if 0 <= i < len(logits):
            out[b, :, :logits[i].shape[-1]] = logits[i][b]
    return out


# ---------------------------------------------------------------------------------------------------------
# argmax
# ---------------------------------------------------------------------------------------------------------
ARGMAX_C = [1, 63, 64, 65, 5374]
ARGMAX_ROWS = [1, 5]
ARGMAX_VARIANTS = ["plain", "tie", "nan", "ninf"]


@functools.lru_cache(maxsize=None)
def argmax_case(rows, C, variant):
    """x uniform in +-4.  "tie": the maximum + 1 stands at two columns of different lanes (c and c + 1 + row, first wins);
    "nan": one NaN per row (torch.max answers its index); "ninf": row rows // 2 is -inf throughout (index 0), the others plain"""
    x = rnd(rows, C, seed=180) * 4
    for r in range(rows):
        c0 = (7 * r + C // 3) % C
        if variant == "tie" and C >= 2:
            c1 = (c0 + 1 + r) % C
            if c1 == c0:
                c1 = (c0 + 1) % C
            x[r, c0] = x[r, c1] = 5.0
        elif variant == "nan":
            x[r, c0] = float("nan")
    if variant == "ninf":
        x[rows // 2] = float("-inf")
    idx = torch.max(x.double(), 1).indices
    prob = torch.softmax(x.double(), 1).max(1).values
    prob32 = torch.softmax(x, 1).max(1).values
    return dict(rows=rows, C=C, variant=variant, x=x, idx=idx, prob=prob, prob32=prob32)


# ---------------------------------------------------------------------------------------------------------
# DMRouterFn end to end
# ---------------------------------------------------------------------------------------------------------
DM_SHAPES = [(1, 31, 1, 128), (1, 33, 2, 256), (3, 31, 3, 256), (2, 65, 8, 512)]        # (B, P, I, C)


@functools.lru_cache(maxsize=None)
def dm_inputs(B, P, I, C):
    """x, the 16 parameters (DMRouterFn's order: Linear weights uniform in +-1 / sqrt(fan-in), norm weights about 1.2, biases +-0.3)
    and the upstream gradient"""
    N = P * I

    def lin(n, k, seed):
        return rnd(n, k, seed=seed) / k ** 0.5, rnd(n, seed=seed + 1) * 0.3

    def norm(n, seed):
        return rnd(n, seed=seed) * 0.5 + 1.2, rnd(n, seed=seed + 1) * 0.3
    w1, b1 = lin(2 * C, C, 200)
    wsp, bsp = lin(N, N, 202)
    w2, b2 = lin(C, C, 204)
    wch, bch = lin(I * C, I * C, 206)
    w3, b3 = lin(C, C, 208)
    n_w, n_b = norm(C, 210)
    sn_w, sn_b = norm(C, 212)
    cn_w, cn_b = norm(P, 214)
    bch = bch + 1.0                                                               # (the gate multiplies: keep it away from zero)
    x, dout = rnd(B, P, I, C, seed=216), rnd(B, P, I, C, seed=217)
    return x, (n_w, n_b, w1, b1, sn_w, sn_b, wsp, bsp, w2, b2, cn_w, cn_b, wch, bch, w3, b3), dout


@functools.lru_cache(maxsize=None)
def dm_case(B, P, I, C):
    x, params, dout = dm_inputs(B, P, I, C)
    ref, base = both(dm_router_reference, x, params, dout)
    return dict(B=B, P=P, I=I, C=C, x=x, params=params, dout=dout, ref=ref, base=base)
