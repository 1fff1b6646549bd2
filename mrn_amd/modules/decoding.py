"""How validation() decodes a CTC head, and the host form of the beam decoder (pure Python: importable without a GPU).

validation() (mrn_amd/test.py, reference test.py:211-219) decodes by best path: the arg-max of every frame, collapsed.  That is the
single most likely ALIGNMENT.  With opt.ctc_decode = "beam" the CTC heads are decoded by prefix beam search instead, which sums over
alignments and returns the most likely LABEL with its (pruned) probability.  The attention head has no alignments to sum over and
ignores the option.

The algorithm, which mrn_ctc_beam_decode_f32 (mrn_amd/csrc/ctc_beam.hip) runs in float32 and ctc_beam_host below in float64.  Per
sample x[T][C], class 0 the blank, beam width W, cut-off K.  An entry is (prefix, pb, pnb): the log-probability of the prefix ending
in blank / in non-blank; total = logaddexp(pb, pnb).  Start: ((), 0, -inf).  Per frame t:

  1. lp = x[t] - logsumexp(x[t]);
  2. S = the k = min(K, C - 1) non-blank classes of largest raw logit, a tie to the lower class, kept in that order;
  3. entry i with last class l stays:       pb' = total_i + lp[0],  pnb' = pnb_i + lp[l] if l in S else -inf;
  4. entry i extended by c in S (rank r):   pb' = -inf,  pnb' = (pb_i if c == l else total_i) + lp[c];
  5. an extension that spells a live entry j is added (logaddexp) into j's stay pnb' and dropped;
  6. of the candidates with a finite total the W largest are kept, ties in candidate order (i, slot), slot 0 = stay, 1 + r = rank r.

Outputs per sample, entries in descending total: tokens [W][T] (0 behind the prefix), length [W] (-1 = dead slot), score [W]; and for
the best entry the pair that goes wherever argmax_prob_lastdim's goes: path [T] = its classes with one blank between equal
neighbours, blanks behind (the greedy collapse gives the prefix back) and prob [T] = [exp(score), 1, 1, ...] (the cumulative product
is exp(score): multiplying by 1.0 is exact).
"""
import numpy as np

CTC_DECODERS = ("greedy", "beam")
DEFAULT_BEAM_WIDTH = 8
DEFAULT_BEAM_TOP_N = 15

BEAM_MAX_T = 512             # frames mrn_ctc_beam_decode_f32 takes (the scorer's SCORE_MAX_T; two [W][T] token buffers in LDS)
BEAM_MAX_CLASSES = 65535     # classes are 16-bit tokens there
BEAM_MAX_WIDTH = 16          # entries live in lanes, candidates four per lane: W * (K + 1) <= 256
BEAM_MAX_TOP_N = 15


def _positive_int(opt, name, default):
    v = getattr(opt, name, default)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return int(v)


def decode_options(opt):
    """(ctc_decode, beam_width, beam_top_n) of an options object; absent keys are "greedy", 8, 15"""
    mode = getattr(opt, "ctc_decode", "greedy")
    if mode not in CTC_DECODERS:
        raise ValueError(f"ctc_decode must be one of {CTC_DECODERS}, got {mode!r}")
    return mode, _positive_int(opt, "beam_width", DEFAULT_BEAM_WIDTH), _positive_int(opt, "beam_top_n", DEFAULT_BEAM_TOP_N)


def beam_supported(prediction, T, C, W, K):
    """does mrn_ctc_beam_decode_f32 decode T frames of C classes of a `prediction` head with beam width W and cut-off K"""
    return ("CTC" in prediction and 1 <= T <= BEAM_MAX_T and 2 <= C <= BEAM_MAX_CLASSES and 1 <= W <= BEAM_MAX_WIDTH
            and 1 <= K <= BEAM_MAX_TOP_N)


def _cut_off(row, k):
    """the k non-blank classes of largest raw logit, a tie to the lower class, in that order (linear in C: no full sort)"""
    x = row[1:]
    if k >= x.size:
        chosen = np.arange(x.size)
    else:
        kth = np.partition(x, x.size - k)[x.size - k]
        above = np.flatnonzero(x > kth)
        chosen = np.concatenate([above, np.flatnonzero(x == kth)[:k - above.size]])
    return chosen[np.lexsort((chosen, -x[chosen]))] + 1


def _beam_one(x, W, K):
    """one sample [T][C] -> [(prefix tuple, total)] in descending total"""
    T, C = x.shape
    k = min(K, C - 1)
    x64 = x.astype(np.float64)
    peak = x64.max(axis=1, keepdims=True)
    lp_all = x64 - (peak + np.log(np.exp(x64 - peak).sum(axis=1, keepdims=True)))
    prefix, pb, pnb = [()], np.zeros(1), np.full(1, -np.inf)
    for t in range(T):
        lp = lp_all[t]
        S = _cut_off(x[t], k)
        rank = {int(c): r for r, c in enumerate(S)}
        n = len(prefix)
        total = np.logaddexp(pb, pnb)
        last = np.array([p[-1] if p else -1 for p in prefix], dtype=np.int64)
        in_S = np.array([int(c) in rank for c in last], dtype=bool)
        stay_pb = total + lp[0]
        stay_pnb = np.where(in_S, pnb + lp[np.maximum(last, 0)], -np.inf)
        ext = np.where(S[None, :] == last[:, None], pb[:, None], total[:, None]) + lp[S][None, :]        # [n][k]
        where = {p: i for i, p in enumerate(prefix)}
        dropped = np.zeros((n, k), dtype=bool)
        for j, p in enumerate(prefix):          # the one extension that spells entry j: from the entry that is p without its last class
            if p and p[-1] in rank and p[:-1] in where:
                i, r = where[p[:-1]], rank[p[-1]]
                stay_pnb[j] = np.logaddexp(stay_pnb[j], ext[i, r])
                dropped[i, r] = True
        cand_pb = np.concatenate([stay_pb[:, None], np.full((n, k), -np.inf)], axis=1).reshape(-1)      # candidate order (i, slot)
        cand_pnb = np.concatenate([stay_pnb[:, None], np.where(dropped, -np.inf, ext)], axis=1).reshape(-1)
        cand_total = np.logaddexp(cand_pb, cand_pnb)
        cand_total[~np.isfinite(cand_total)] = -np.inf
        keep = [q for q in np.argsort(-cand_total, kind="stable")[:W] if cand_total[q] > -np.inf]
        prefix = [prefix[q // (k + 1)] + ((int(S[q % (k + 1) - 1]),) if q % (k + 1) else ()) for q in keep]
        pb, pnb = cand_pb[keep], cand_pnb[keep]
    return list(zip(prefix, np.logaddexp(pb, pnb)))


def frame_path(prefix, T):
    """a prefix as a row of T frames: one blank between equal neighbours, blanks behind"""
    row = []
    for c in prefix:
        if row and row[-1] == c:
            row.append(0)
        row.append(c)
    if len(row) > T:
        raise ValueError(f"a prefix of {len(prefix)} classes needs {len(row)} frames, more than {T}")
    return row + [0] * (T - len(row))


def ctc_beam_host(logits, W, K):
    """float64 prefix beam search of logits [B][T][C] (numpy) -> (tokens int32 [B][W][T], length int32 [B][W], score float64 [B][W],
    path int64 [B][T], prob float32 [B][T]): the outputs of ops.ctc_beam_decode, for CPU tensors and for batches outside the
    kernel's limits.  Any W >= 1 and K >= 1"""
    logits = np.asarray(logits)
    if logits.ndim != 3 or logits.shape[1] < 1 or logits.shape[2] < 2 or W < 1 or K < 1:
        raise ValueError(f"ctc_beam_host needs logits [B][T >= 1][C >= 2], W >= 1 and K >= 1, got {logits.shape}, {W}, {K}")
    B, T, _ = logits.shape
    tokens = np.zeros((B, W, T), dtype=np.int32)
    length = np.full((B, W), -1, dtype=np.int32)
    score = np.full((B, W), -np.inf, dtype=np.float64)
    path = np.zeros((B, T), dtype=np.int64)
    prob = np.ones((B, T), dtype=np.float32)
    for b in range(B):
        entries = _beam_one(logits[b], W, K)
        for w, (p, s) in enumerate(entries):
            tokens[b, w, :len(p)] = p
            length[b, w] = len(p)
            score[b, w] = s
        if entries:
            path[b] = frame_path(entries[0][0], T)
        prob[b, 0] = np.float32(np.exp(score[b, 0]))
    return tokens, length, score, path, prob
