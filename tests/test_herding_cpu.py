"""Herding exemplar selection (mrn_amd/modules/herding.py, include/mrn_herding.h, csrc/herding.hip): what can be checked without a GPU.
The header and the exported symbols, the float64 host form herding_host against an independent restatement in exact rational
arithmetic, its properties (distinct picks, prefixes, permutations, the tie rule, the errors), the claim the GPU tests rest on -- that
small-integer tables make every quantity exact in fp32 under any summation order --, and the learners' bookkeeping with a fake loader
and a stubbed feature hook."""
import contextlib
import ctypes
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.helpers import DetLoader
from tests.test_learners_cpu import learner_opt

HERDING = ("mrn_herding_features_f32", "mrn_herding_select_work_bytes", "mrn_herding_select_f32")
U32 = 2.0 ** -24


# ---- tables and yardsticks shared with tests/test_herding_gpu.py -------------------------------------------------------------------
def integer_table(seed, N, D):
    """integers -2 ... 2 as float32: with N a power of two every mean, residual, product and sum below is a multiple of 1 / N of
    modest size, exact in fp32 and in float64 whatever the order of the additions"""
    return np.random.default_rng(seed).integers(-2, 3, (N, D)).astype(np.float32)


def duplicated_table(seed, N, D):
    """N / 2 rows, each twice, the copies N / 2 apart: every step but the last of a pair is a tie between two rows"""
    half = integer_table(seed, N // 2, D)
    return np.concatenate([half, half], 0)


def unit_table(seed, N, D, offset=1.0):
    """unit rows with a common offset: normal rows shifted along one direction, normalised (fp32)"""
    rng = np.random.default_rng(seed)
    direction = rng.standard_normal(D)
    direction /= np.linalg.norm(direction)
    x = rng.standard_normal((N, D)) / np.sqrt(D) + offset * direction
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def replay(F, picks):
    """the picks replayed in float64 on the table F: -> (excess [m], tau [m], objective [m]).  objective_k = the picked row's
    ||f||^2 - 2 f . r_k, excess_k = that minus the minimum over the rows not yet picked, given the previous picks; tau_k =
    4 (D + 4) 2^-24 (max ||f||^2 + max ||f|| ||r_k||), the worst case of one fp32 dot product, of the fp32 norms and of the rounding
    of r (twice: the picked row and the best one).  Raises when a pick is out of range or repeated"""
    F = np.asarray(F, dtype=np.float64)
    N, D = F.shape
    norms = (F * F).sum(1)
    mu = F.mean(0)
    r = mu.copy()
    free = np.ones(N, dtype=bool)
    excess, tau, objective = np.empty(len(picks)), np.empty(len(picks)), np.empty(len(picks))
    for k, i in enumerate(int(p) for p in picks):
        assert 0 <= i < N and free[i], (k, i)
        d = norms - 2.0 * (F @ r)
        objective[k] = d[i]
        excess[k] = d[i] - d[free].min()
        tau[k] = 4 * (D + 4) * U32 * (norms.max() + np.sqrt(norms.max()) * np.linalg.norm(r))
        free[i] = False
        r = r + mu - F[i]
    return excess, tau, objective


def herding_by_definition(F, m):
    """iCaRL's own statement in exact rational arithmetic: at step k the unpicked row i that minimises ||mu - (S + f_i) / k||, the
    lowest index among equals; S the sum of the rows picked so far"""
    N, D = F.shape
    rows = [[Fraction(int(v)) for v in row] for row in F]
    mu = [sum(rows[i][j] for i in range(N)) / N for j in range(D)]
    S = [Fraction(0)] * D
    picks, free = [], [True] * N
    for k in range(1, m + 1):
        best, arg = None, -1
        for i in range(N):
            if free[i]:
                dist2 = sum((mu[j] - (S[j] + rows[i][j]) / k) ** 2 for j in range(D))
                if best is None or dist2 < best:
                    best, arg = dist2, i
        picks.append(arg)
        free[arg] = False
        S = [S[j] + rows[arg][j] for j in range(D)]
    return picks


def herding_fp32_permuted(F, m, seed):
    """the selection as a device would form it: fp32 norms and products summed in a random column order one term at a time, mu and r
    in float64, r rounded to fp32 once per step"""
    F = np.asarray(F, dtype=np.float32)
    N, D = F.shape
    order = np.random.default_rng(seed).permutation(D)

    def dots(v):
        acc = np.zeros(N, dtype=np.float32)
        for j in order:
            acc = (acc + F[:, j] * v[j]).astype(np.float32)
        return acc
    norms = np.zeros(N, dtype=np.float32)
    for j in order:
        norms = (norms + F[:, j] * F[:, j]).astype(np.float32)
    mu = F.astype(np.float64)[np.random.default_rng(seed + 1).permutation(N)].sum(0) / N
    r = mu.copy()
    free = np.ones(N, dtype=bool)
    picks, dist = [], []
    for _ in range(m):
        d = (norms - np.float32(2) * dots(r.astype(np.float32))).astype(np.float32)
        d = np.where(free, d, np.float32(np.inf))
        i = int(np.argmin(d))
        picks.append(i)
        dist.append(float(d[i]))
        free[i] = False
        r = r + mu - F[i].astype(np.float64)
    return np.array(picks), np.array(dist)


# ---- the header --------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    from mrn_amd.modules import herding as H
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.HERDING_HEADER_PATH)
    assert tuple(protos) == HERDING
    others = [_lib.parse_header(), _lib.parse_header(_lib.DECODE_HEADER_PATH), _lib.parse_header(_lib.ATTN_BEAM_HEADER_PATH),
              _lib.parse_header(_lib.LEXICON_HEADER_PATH), _lib.parse_header(_lib.ATTN_LEXICON_HEADER_PATH),
              _lib.parse_header(_lib.ATTN_SCORE_HEADER_PATH), _lib.parse_header(_lib.SHORTLIST_HEADER_PATH)]
    assert not any(set(protos) & set(o) for o in others)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    loaded = _lib.LIB.load()
    for name in HERDING:
        assert hasattr(dll, name) and name in _lib.LIB._protos
        assert len(getattr(loaded, name).argtypes) == len(protos[name][2])
    ret, argtypes, argnames = protos["mrn_herding_select_f32"]
    assert ret == "int" and argnames == ["F", "N", "D", "m", "picks", "dist", "work", "work_bytes", "stream"]
    assert argtypes[0] == "const float*" and argtypes[4] == "int32_t*" and argtypes[5] == "float*"
    ret, argtypes, argnames = protos["mrn_herding_features_f32"]
    assert argnames == ["feat", "B", "T", "D", "batch_stride", "time_stride", "F", "N", "row0", "stream"]
    assert argtypes[4] == "int64_t" and argtypes[5] == "int64_t"
    assert protos["mrn_herding_select_work_bytes"][0] == "int64_t" and loaded.mrn_herding_select_work_bytes.restype is ctypes.c_int64
    # the workspace rule is host-side (no launch): positive within the limits, -1 outside, and it grows with the table
    work = loaded.mrn_herding_select_work_bytes
    assert work(1, 4) > 0 and work(H.MAX_ROWS, H.MAX_DIM) > work(1000, 256) >= 1000 * 5 + 256 * 24
    for N, D in ((0, 4), (H.MAX_ROWS + 1, 4), (10, 0), (10, 6), (10, H.MAX_DIM + 4), (10, 2)):
        assert work(N, D) == -1 and not H.select_supported(N, D, 1)
    assert H.select_supported(1, 4, 1) and H.select_supported(H.MAX_ROWS, H.MAX_DIM, H.MAX_ROWS) and not H.select_supported(5, 8, 6)


def test_limits_match_the_kernel_source():
    import os
    import re
    from mrn_amd.modules import herding as H
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrn_amd", "csrc", "herding.hip")).read()
    const = {m.group(1): m.group(2) for m in re.finditer(r"constexpr (?:int|float) (HERD_\w+) = ([^;]+);", src)}
    assert const["HERD_MAX_N"] == "1 << 24" and H.MAX_ROWS == 1 << 24
    assert int(const["HERD_MIN_D"]) == H.MIN_DIM and int(const["HERD_MAX_D"]) == H.MAX_DIM
    assert float(const["HERD_EPS"].rstrip("f")) == H.FEATURE_EPS


# ---- the host form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,N,D", [(0, 16, 3), (1, 32, 6), (2, 8, 1), (3, 64, 4)])
def test_host_form_is_the_definition(seed, N, D):
    from mrn_amd.modules.herding import herding_host
    F = integer_table(seed, N, D)
    picks, dist = herding_host(F, N)
    assert picks.dtype == np.int64 and dist.dtype == np.float64 and picks.shape == dist.shape == (N,)
    assert picks.tolist() == herding_by_definition(F, N)
    excess, _, objective = replay(F, picks)
    assert (excess == 0).all() and np.array_equal(objective, dist)
    # dist is the minimised ||f||^2 - 2 f . r_k: add ||r_k||^2 and it is the squared distance the definition minimises, times k^2
    F64, mu, S = F.astype(np.float64), F.astype(np.float64).mean(0), np.zeros(D)
    for k, i in enumerate(picks, 1):
        r = k * mu - S
        assert dist[k - 1] + r @ r == pytest.approx(((r - F64[i]) ** 2).sum(), abs=1e-9)
        S += F64[i]


def test_host_form_properties():
    from mrn_amd.modules.herding import herding_host
    F = unit_table(4, 90, 12)
    full, full_d = herding_host(F, 90)
    assert sorted(full.tolist()) == list(range(90))                       # m == N: a permutation of all the rows
    for j in range(1, 91):
        picks, dist = herding_host(F, j)
        assert len(set(picks.tolist())) == j
        assert np.array_equal(picks, full[:j]) and np.array_equal(dist, full_d[:j])
    # a table whose rows each occur twice: the copy with the lower index goes first, whichever way the copies are laid out
    for table in (duplicated_table(5, 64, 6), np.repeat(integer_table(6, 32, 5), 2, 0)):
        picks = herding_host(table, len(table)).__getitem__(0).tolist()
        rows = {}
        for at, i in enumerate(picks):
            rows.setdefault(table[i].tobytes(), []).append((i, at))
        for copies in rows.values():
            by_index = sorted(copies)
            assert [at for _, at in by_index] == sorted(at for _, at in by_index), copies


def test_host_form_errors():
    from mrn_amd import ops
    from mrn_amd.modules.herding import features_host, herding_host
    F = unit_table(7, 10, 8)
    for bad_m in (0, -1, 11, 2.5, True):
        with pytest.raises(ValueError, match="herding"):
            herding_host(F, bad_m)
        with pytest.raises(ValueError, match="herding"):
            ops.herding_select(torch.from_numpy(F), bad_m)
    for empty in (np.zeros((0, 8), np.float32), np.zeros((5, 0), np.float32)):
        with pytest.raises(ValueError, match="empty"):
            herding_host(empty, 1)
        with pytest.raises(ValueError, match="empty"):
            ops.herding_select(torch.from_numpy(empty), 1)
    for poison in (np.nan, np.inf, -np.inf):
        G = F.copy()
        G[3, 2] = poison
        with pytest.raises(ValueError, match="non-finite"):
            herding_host(G, 2)
        with pytest.raises(ValueError, match="non-finite"):
            ops.herding_select(torch.from_numpy(G), 2)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        herding_host(F[0], 1)
    with pytest.raises(ValueError, match="T >= 1"):
        features_host(np.zeros((2, 0, 4)))


def test_features_host():
    from mrn_amd.modules.herding import features_host
    rng = np.random.default_rng(8)
    feat = rng.standard_normal((5, 7, 12)).astype(np.float32)
    feat[2] = 0
    out = features_host(feat)
    assert out.dtype == np.float64 and out.shape == (5, 12)
    for b in range(5):
        mean = feat[b].astype(np.float64).sum(0) / 7
        assert np.allclose(out[b], mean / (np.sqrt(mean @ mean) + 1e-8), rtol=1e-15, atol=0)
    assert (out[2] == 0).all() and np.allclose(np.linalg.norm(out[[0, 1, 3, 4]], axis=1), 1, atol=1e-7)


@pytest.mark.parametrize("case", ["256x16", "512x132", "dup256x8"])
def test_integer_tables_are_exact_in_fp32_under_any_summation_order(case):
    """what the exact GPU cases rest on: an fp32 evaluation with the terms of every sum in a random order returns herding_host's picks
    and its dist, to the last bit"""
    from mrn_amd.modules.herding import herding_host
    F, m = {"256x16": (integer_table(10, 256, 16), 256), "512x132": (integer_table(11, 512, 132), 100),
            "dup256x8": (duplicated_table(12, 256, 8), 256)}[case]
    picks, dist = herding_host(F, m)
    for seed in (0, 1):
        p32, d32 = herding_fp32_permuted(F, m, seed)
        assert np.array_equal(p32, picks) and np.array_equal(d32, dist)


def test_cpu_tensors_take_the_host_forms():
    from mrn_amd import ops
    from mrn_amd.modules.herding import features_host, herding_host
    rng = np.random.default_rng(13)
    feat = torch.from_numpy(rng.standard_normal((6, 5, 8)).astype(np.float32))
    table = torch.full((10, 8), 7.0)
    out = ops.herding_features(feat[::2], out=table, row0=4)
    assert out is table and (table[:4] == 7).all() and (table[7:] == 7).all()
    assert np.array_equal(table[4:7].numpy(), features_host(feat[::2].numpy()).astype(np.float32))
    fresh = ops.herding_features(feat)
    assert fresh.shape == (6, 8) and fresh.dtype == torch.float32
    picks, dist = ops.herding_select(fresh, 4)
    ref = herding_host(fresh.numpy(), 4)
    assert picks.dtype == torch.int64 and dist.dtype == torch.float32 and not picks.is_cuda
    assert np.array_equal(picks.numpy(), ref[0]) and np.array_equal(dist.numpy(), ref[1].astype(np.float32))
    with pytest.raises(ValueError, match="out must be"):
        ops.herding_features(feat, out=table, row0=5)
    with pytest.raises(ValueError, match="float32"):
        ops.herding_select(fresh.double(), 2)


# ---- the learners' bookkeeping -----------------------------------------------------------------------------------------------------
class OrderedLoader(DetLoader):
    """the fake loader with an ordered pass over the previous task's data: `sizes[taski - 1]` samples in batches of 7, the "image" of
    a sample being its contextual feature [T, D] itself (the stubbed hook returns it)"""

    def __init__(self, sizes, T=3, D=8):
        super().__init__(2, "herding", 1)
        rng = np.random.default_rng(21)
        self.data = [torch.from_numpy(rng.standard_normal((n, T, D)).astype(np.float32) + 0.3) for n in sizes]

    def rehearsal_prev_model(self, taski):
        self.calls.append(("rehearsal_prev_model", (taski,)))
        data = self.data[taski - 1]
        return [(data[i:i + 7], ["x"] * len(data[i:i + 7])) for i in range(0, len(data), 7)], len(data)


@pytest.mark.parametrize("name", ["base", "mrn"])
def test_herding_memory_bookkeeping(name):
    from mrn_amd.il_modules.base import BaseLearner
    from mrn_amd.il_modules.mrn import MRN
    from mrn_amd.modules.herding import features_host, herding_host
    opt = learner_opt(memory="herding", memory_num=24)
    sizes = (40, 33, 50)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = (BaseLearner if name == "base" else MRN)(opt)
        loader = OrderedLoader(sizes)
        seen = []

        def hook(image, taski):
            assert not torch.is_grad_enabled() and not any(mod.training for mod in learner.model.modules())
            seen.append(taski)
            return image
        learner.herding_feature = hook
        learner.model.train()
        frozen = list(learner.model.modules())[-1]                  # (a leaf) a module a learner keeps in eval mode stays there
        frozen.eval()
        orders = [herding_host(features_host(d.numpy()).astype(np.float32), n)[0] for d, n in zip(loader.data, sizes)]
        np.random.seed(99)
        state = np.random.get_state()
        for taski in range(1, 4):
            learner.build_rehearsal_memory(loader, taski)
            num = 24 // taski
            assert len(learner.memory_index) == taski
            for i, idx in enumerate(learner.memory_index):          # the newest list in herding order, the older ones cut to prefixes
                assert isinstance(idx, np.ndarray) and idx.dtype.kind == "i"
                assert np.array_equal(idx, orders[i][:num]), (taski, i)
            assert learner.model.training and not frozen.training
            assert all(mod.training for mod in learner.model.modules() if mod is not frozen)
        after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]       # no numpy random draw
    assert seen == [1] * 6 + [2] * 5 + [3] * 8
    calls = [c for c in loader.calls if c[0] == "get_dataset"]
    assert [c[1][:2] for c in calls] == [(1, "herding"), (2, "herding"), (3, "herding")]
    for taski, c in enumerate(calls, 1):                            # get_dataset received the lists as they stood
        assert [i.tolist() for i in c[1][2]] == [o[:24 // taski].tolist() for o in orders[:taski]]


def test_random_memory_is_untouched_by_the_new_option():
    """memory="random" still draws np.random.choice at the same place of the stream (the golden lists of test_learners_cpu.py pin the
    values; here: the draw is the first one after the seed) and never calls the feature hook"""
    from mrn_amd.il_modules.base import BaseLearner
    with contextlib.redirect_stdout(io.StringIO()):
        learner = BaseLearner(learner_opt(memory="random", memory_num=24))
        learner.herding_feature = None
        loader = OrderedLoader((40,))
        np.random.seed(5)
        learner.build_rehearsal_memory(loader, 1)
    assert np.array_equal(learner.memory_index[0], np.random.RandomState(5).choice(range(40), 24, replace=False))
