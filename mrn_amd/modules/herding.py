"""Herding exemplar selection for the rehearsal memory (iCaRL, Rebuffi et al. 2017, algorithm 4), per task: the algorithm, stated once.
Pure Python / numpy, imports without a GPU.  csrc/herding.hip (include/mrn_herding.h, ops.herding_features / ops.herding_select) is the
device form; the functions here are its float64 restatement and what CPU tensors take.

Features.  A sample's feature is the time mean of its contextual feature [T, D], divided by (its Euclidean norm + 1e-8): a unit vector,
or all zeros for an all-zero sample.

Selection of m out of the N rows of F [N, D].  mu = the column mean of F, r_1 = mu.  At step k = 1 ... m the pick is the row i, among
the rows not yet picked, that minimises

    d_i = ||f_i||^2 - 2 f_i . r_k

which is ||k mu - S_{k-1} - f_i||^2 up to the term ||r_k||^2 common to all i (S = the sum of the rows picked so far, r_k = k mu - S_{k-1}):
the row that keeps the running mean of the picks closest to the mean of the task.  A tie goes to the lower row index.  Then
r_{k+1} = r_k + mu - f_i.  The result is picks [m] IN PICK ORDER and dist [m], the minimised d of every step.  A prefix of the picks is
the selection for the smaller budget, which is what BaseLearner.reduce_samplers relies on when it cuts a list back.

Left out on purpose: per-character or per-class herding (the memory here is per task), fp16 tables, sharding over ranks.
"""
import numpy as np

FEATURE_EPS = 1e-8
MAX_ROWS = 1 << 24          # csrc/herding.hip: HERD_MAX_N
MIN_DIM, MAX_DIM = 4, 8192  # HERD_MIN_D, HERD_MAX_D; D % 4 == 0 (16-byte loads of a row)


def select_supported(N, D, m):
    """the limits of mrn_herding_select_f32"""
    return 1 <= m <= N <= MAX_ROWS and MIN_DIM <= D <= MAX_DIM and D % 4 == 0


def check_request(N, D, m):
    """the errors both paths raise before anything is computed or launched"""
    if N < 1 or D < 1:
        raise ValueError(f"herding: an empty feature table [{N}, {D}]")
    if isinstance(m, bool) or int(m) != m:
        raise ValueError(f"herding: m must be an integer, got {m!r}")
    if m < 1 or m > N:
        raise ValueError(f"herding: m = {m} outside 1 ... N = {N}")
    return int(m)


def features_host(feat):
    """feat [B, T, D] (anything numpy converts) -> float64 [B, D]: the time mean divided by (its norm + 1e-8)"""
    feat = np.asarray(feat, dtype=np.float64)
    if feat.ndim != 3 or feat.shape[1] < 1:
        raise ValueError(f"herding features need [B, T >= 1, D], got {feat.shape}")
    mean = feat.mean(axis=1)
    return mean / (np.sqrt((mean * mean).sum(axis=1, keepdims=True)) + FEATURE_EPS)


def herding_host(F, m):
    """F [N, D], m -> (picks int64 [m] in pick order, dist float64 [m]): the selection of the module docstring in float64"""
    F = np.asarray(F, dtype=np.float64)
    if F.ndim != 2:
        raise ValueError(f"herding: the feature table must be [N, D], got {F.shape}")
    N, D = F.shape
    m = check_request(N, D, m)
    if not np.isfinite(F).all():
        raise ValueError("herding: the feature table has non-finite entries")
    mu = F.mean(axis=0)
    norms = (F * F).sum(axis=1)
    r = mu.copy()
    free = np.ones(N, dtype=bool)
    picks = np.empty(m, dtype=np.int64)
    dist = np.empty(m, dtype=np.float64)
    for k in range(m):
        d = np.where(free, norms - 2.0 * (F @ r), np.inf)
        i = int(np.argmin(d))                      # the first minimum: a tie goes to the lower index
        picks[k], dist[k] = i, d[i]
        free[i] = False
        r = r + mu - F[i]
    return picks, dist
