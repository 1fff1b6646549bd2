"""Inputs of the lexicon-decoding tests, generated once and shared: tests/test_lexicon_cpu.py holds the float64 host form
(mrn_amd/modules/decoding.py::ctc_lexicon_host) to the independent reference on exactly the inputs tests/test_lexicon_gpu.py gives
mrn_ctc_lexicon_decode_f32 (mrn_amd/csrc/ctc_lexicon.hip).

The independent reference is torch.nn.functional.ctc_loss on the CPU in float64, reduction="none", negated: one (sample, word) pair
per loss entry (a sample's words go through one call as its batch).  It is never the code under test.

A case is a dict: x float32 [B][T][C] (read-only), tokens int32 [N][Lmax], lens int32 [N], cand int32 [B][K] or None, n."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

ATOL, RTOL = 1e-5, 1e-5      # score_all against the float64 reference on live pairs: the band tests/test_long_labels_gpu.py holds the
#                              CTC loss kernels to against torch; -inf pairs agree exactly


def pack(words):
    """list of class lists -> (tokens int32 [N][Lmax >= 1], lens int32 [N])"""
    lens = np.array([len(w) for w in words], dtype=np.int32)
    tokens = np.zeros((len(words), max(int(lens.max()), 1)), dtype=np.int32)
    for i, w in enumerate(words):
        tokens[i, :len(w)] = w
    return tokens, lens


def unpack(tokens, lens):
    return [[int(c) for c in tokens[i, :lens[i]]] for i in range(len(lens))]


def needs(word):
    """frames a word needs: its length plus one blank per pair of equal neighbours"""
    return len(word) + sum(a == b for a, b in zip(word, word[1:]))


def _case(x, words, n, cand=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    tokens, lens = pack(words)
    return dict(x=x, tokens=tokens, lens=lens, cand=None if cand is None else np.asarray(cand, dtype=np.int32), n=n)


def _random_words(rng, N, C, lo, hi, repeat=0.3):
    """N words of lo..hi classes out of 1..C-1; with probability `repeat` a class repeats its left neighbour"""
    words = []
    for _ in range(N):
        w = []
        for _ in range(int(rng.integers(lo, hi + 1))):
            w.append(w[-1] if w and rng.random() < repeat else int(rng.integers(1, C)))
        words.append(w)
    return words


@functools.lru_cache(maxsize=None)
def all_pairs():
    """B = 3, T = 12, C = 7, N = 40: words of 0..6 classes with repeats.  No word of at most 6 classes is infeasible in 12 frames (it
    needs 11 at the most), so the infeasible ones are three longer words: 7 and 8 equal classes (13, 15 frames) and 9 classes with four
    repeats (13 frames)"""
    rng = np.random.default_rng(4101)
    words = [[]] + [[int(c) for c in rng.integers(1, 7, size=L)] for L in range(1, 7)] + [[3] * 6, [1, 1, 2, 2, 3, 3], [5, 5]]
    words += [[2] * 7, [4] * 8, [1, 1, 2, 2, 3, 3, 4, 4, 5]]
    words += _random_words(rng, 40 - len(words), 7, 0, 6, repeat=0.4)
    return _case(2.0 * rng.standard_normal((3, 12, 7)), words, 4)


STATE_EDGE = [(L, T) for L in (0, 1, 30, 31) for T in ("tight", 63, 64, 65)]


@functools.lru_cache(maxsize=None)
def state_edge(L, T):
    """C = 40, B = 2: a word of L distinct-neighbour classes, one with r = min(3, L - 1) repeats, one of L equal classes, and the
    shorter words around L.  T = "tight" is L + r frames: the second word has exactly one alignment, the third is infeasible when it
    needs more"""
    rng = np.random.default_rng(4200 + L)
    r = max(min(3, L - 1), 0)
    plain = [int(c) for c in (np.arange(L) * 7 + 3) % 39 + 1]
    assert all(a != b for a, b in zip(plain, plain[1:]))
    rep = list(plain)
    for i in range(r):
        rep[2 * i + 1] = rep[2 * i]
    words = [plain, rep, [17] * L, plain[:max(L - 1, 0)], plain[:1], []]
    frames = max(L + r, 1) if T == "tight" else T
    return _case(2.0 * rng.standard_normal((2, frames, 40)), words, 4)


@functools.lru_cache(maxsize=None)
def frames(T):
    """T in {1, 2, 512} at B = 2, N = 9, C = 5"""
    rng = np.random.default_rng(4300 + T)
    words = [[], [1], [4], [2, 2], [1, 3], [3, 3, 3], [4, 1, 2], [2], [1, 1]]
    return _case(2.0 * rng.standard_normal((2, T, 5)), words, 4)


@functools.lru_cache(maxsize=None)
def classes(C):
    """C = 2: words of class 1 only, every neighbour a repeat (B = 2, T = 8).  C = 65535: B = 1, T = 4, classes 1 and 65534"""
    rng = np.random.default_rng(4400 + C)
    if C == 2:
        return _case(2.0 * rng.standard_normal((2, 8, 2)), [[1] * L for L in (0, 1, 2, 3, 4, 5)], 4)
    hi = C - 1
    words = [[], [1], [hi], [1, hi], [hi, 1], [hi, hi], [1, hi, 1], [hi, hi, hi]]
    return _case(2.0 * rng.standard_normal((1, 4, C)), words, 4)


TAILS = [(N, B) for N in (1, 5, 257) for B in (1, 17)]


@functools.lru_cache(maxsize=None)
def tails(N, B):
    """N in {1, 5, 257} x B in {1, 17}: word counts around the four words of a block, batches around nothing in particular"""
    rng = np.random.default_rng(4500 + 31 * N + B)
    return _case(2.0 * rng.standard_normal((B, 9, 11)), _random_words(rng, N, 11, 0, 6), 4)


@functools.lru_cache(maxsize=None)
def candidates():
    """K = 6 candidate slots per sample out of N = 20 words: -1 slots in front, between and behind, a word named twice in a row, a
    row of one word, a row of nothing"""
    rng = np.random.default_rng(4600)
    cand = [[3, -1, 7, 7, 19, 0], [-1, -1, 5, 2, -1, 5], [11, 11, 11, 11, 11, 11], [-1, -1, -1, -1, -1, -1], [0, 1, 2, 3, 4, 5]]
    return _case(2.0 * rng.standard_normal((5, 10, 9)), _random_words(rng, 20, 9, 0, 6), 4, cand)


@functools.lru_cache(maxsize=None)
def ties():
    """duplicate words (bit-equal scores, the lower position first), two infeasible words, n = 8 above the six live ones"""
    rng = np.random.default_rng(4700)
    words = [[1, 2], [3], [1, 2], [3], [4, 4, 4, 4], [1, 2], [2, 2, 2, 2], []]
    return _case(2.0 * rng.standard_normal((3, 6, 6)), words, 8)


@functools.lru_cache(maxsize=None)
def all_dead():
    """every word infeasible in T = 4: no sample has a live word"""
    rng = np.random.default_rng(4800)
    return _case(2.0 * rng.standard_normal((2, 4, 6)), [[1, 1, 1], [2, 3, 4, 5, 1], [5, 5, 2, 2]], 2)


@functools.lru_cache(maxsize=None)
def non_finite():
    """sample 0 clean; sample 1 a NaN in one frame; sample 2 class 3 at -inf in every frame (its words die, the others live);
    sample 3 a +inf logit; sample 4 one frame of -inf only"""
    rng = np.random.default_rng(4900)
    x = 2.0 * rng.standard_normal((5, 7, 6))
    x[1, 4, 2] = np.nan
    x[2, :, 3] = -np.inf
    x[3, 0, 5] = np.inf
    x[4, 6, :] = -np.inf
    return _case(x, [[1], [3], [1, 3], [2, 2], [], [3, 3], [5, 4, 1]], 4)


@functools.lru_cache(maxsize=None)
def agreement():
    """B = 32, T = 63, C = 97, N = 1000 words of 1..25 classes.  Sample b carries word 31 b of the lexicon: its frame path stretched
    over the 63 frames, 6 above noise of sigma 2, so that the ranking has something to find; the other words are random"""
    rng = np.random.default_rng(5000)
    words = [w for w in _random_words(rng, 4000, 97, 1, 25, repeat=0.15) if needs(w) <= 40][:1000]
    assert len(words) == 1000 and {len(w) for w in words} >= {1, 25}
    x = 2.0 * rng.standard_normal((32, 63, 97))
    for b in range(32):
        w = words[31 * b]
        row = []
        for c in w:
            row += ([0] if row and row[-1] == c else []) + [c]
        at = np.sort(rng.choice(63, size=len(row), replace=False))
        for t, c in zip(at, row):
            x[b, t, c] += 6.0
        blank = np.setdiff1d(np.arange(63), at)
        x[b, blank, 0] += 6.0
    return _case(x, words, 4)


def reference_scores(case):
    """float64 [B][Nc]: -ctc_loss(log_softmax(x[b]), word) per (sample, position), -inf for an unused slot.  NaN where torch gives NaN
    (non-finite logits): the ranking rules of such samples are the tests' to state, not this function's"""
    x, tokens, lens, cand = case["x"], case["tokens"], case["lens"], case["cand"]
    B, T, C = x.shape
    lp = torch.log_softmax(torch.from_numpy(np.array(x)).double(), dim=2)
    Nc = len(lens) if cand is None else cand.shape[1]
    out = np.full((B, Nc), -np.inf)
    for b in range(B):
        words = np.arange(len(lens)) if cand is None else cand[b]
        used = np.flatnonzero(words >= 0)
        if not used.size:
            continue
        tg = torch.from_numpy(tokens[words[used]].astype(np.int64))
        ln = torch.from_numpy(lens[words[used]].astype(np.int64))
        loss = F.ctc_loss(lp[b].unsqueeze(1).expand(T, used.size, C), tg, torch.full((used.size,), T, dtype=torch.long), ln, blank=0,
                          reduction="none", zero_infinity=False)
        out[b, used] = -loss.numpy()
    return out


_REFERENCE = {}


def reference(name, maker, *args):
    """reference_scores of maker(*args), computed once per process and left unchanged"""
    key = (name,) + args
    if key not in _REFERENCE:
        ref = reference_scores(maker(*args))
        ref.setflags(write=False)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


def rank(score_row, n):
    """positions of the n best live entries of one sample's scores: descending score, a tie to the lower position"""
    return [int(q) for q in sorted(range(len(score_row)), key=lambda q: (-score_row[q], q))[:n] if score_row[q] > -np.inf]
