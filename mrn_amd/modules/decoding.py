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

Language-model fusion (opt-in: lm = a modules/char_lm.py CharLM, lm_weight alpha >= 0, lm_bonus beta finite; mrn_ctc_beam_lm_decode_f32
runs it in float32).  An entry additionally carries lm, the sum of LM.logp(prev, last, c) over its classes c, accumulated left to right
(prev, last = the two classes in front of c, 0 where the prefix is shorter: begin of text).  lm is a function of the prefix alone, so
two routes to one prefix carry the same bits and step 5's merge stays exact and needs no LM term.  The steps above with step 6 ranked
by a key instead of the total:

  6'. key = total + alpha * lm' + beta * len' (evaluated left to right); a stay has lm' = lm_i, len' = len_i, an extension by c has
      lm' = lm_i + LM.logp(prev_i, last_i, c), len' = len_i + 1.  Of the candidates with a finite (acoustic) total the W largest KEYS
      are kept, ties in candidate order as before; a candidate whose total is not finite never survives, whatever the model says;
  7'. after the last frame the live entries are ordered once more, by fused = total + alpha * (lm + LM.logp(prev, last, 0)) + beta * len
      (0 = end of text), descending, a tie to the earlier slot.

score stays the acoustic log-probability of the label (prob[0] = exp(score) stays a probability for the scorer); one more output,
fused [W], holds the key the entries are ordered by (-inf for a dead slot).  With alpha = beta = 0 the key is the total and tokens,
length, score, path and prob are today's, bit for bit.

The attention head (reference modules/prediction.py:70-86 feeds the arg-max back: one hypothesis) is decoded by beam search with
opt.attn_decode = "beam"; the width is opt.beam_width.  mrn_attn_beam_decode_* (mrn_amd/csrc/attn_decode.hip attn_beam_kernel) runs it in
float32, all steps of all experts in one launch, attn_beam_host below in float64.  Per sample: width W, S = batch_max_length + 1 steps,
start token sos, end token eos.  An entry is (tokens, score, finished, h, c).  Start: one live entry (no tokens, score 0, h = c = 0, fed
sos); the other W - 1 slots are dead (score -inf).  Per step:

  1. every live unfinished entry i runs the attention cell of modules/prediction.py on its last token (a token >= num_class or < 0
     counts as 0, as in greedy) and lp = log_softmax(generator(h)) over the num_class real classes;
  2. entry i gives the candidates (i, c) with score_i + lp[c]; a finished entry (its last token is eos) gives the single candidate
     (i, eos) with its score unchanged, and keeps its tokens;
  3. the W candidates of largest score survive, ties in candidate order (i, then c); a NaN score counts as -inf, and a candidate of
     score -inf never survives (its slot is dead);
  4. a survivor takes its parent's new (h, c); it is finished if c == eos.

There is no length normalisation.  Decoding may stop once every live entry is finished: further steps change nothing.  Outputs per
sample, entries in descending score: tokens int32 [W][S] (eos behind the first eos), length [W] (the tokens up to and including eos, S
for an entry that never finished, -1 = dead slot), score [W] (-inf for a dead slot), logp [W][S] (the log-probability of each chosen
token, 0 behind the first eos); and for the best entry path int64 [S] and prob [S] = exp(logp), 1.0 behind the first eos: the pair
argmax_prob_lastdim hands the scorer.  With W = 1 this is greedy decoding.

Language-model fusion on the attention head (opt-in: lm = a modules/char_lm.py CharLM over the head's classes, lm_weight alpha >= 0,
lm_bonus beta finite, top_n; mrn_attn_beam_lm_decode_* runs it in float32 (attn_beam_lm_kernel), attn_beam_host(lm=) in float64).  An
AttnLabelConverter's class 0 is [UNK], which no text contains (char_lm.encode_texts bans it), so 0 doubles as begin / end of text in
the model exactly as the blank does on a CTC head; [PAD], [SOS] and [EOS] never occur in a text and sit at the unigram floor.  The
beam search above with these differences:

  state: an entry also carries the last two LM symbols (a, b), (0, 0) at the start = begin of text, its LM sum lm and its length len
     in characters; acoustic = the score above;
  LM symbol of a class: eos -> 0, the end of text; every other class -> itself;
  LM term of a proposed class k behind (a, b): LM.logp(a, b, 0) for k = eos; unk_logp, flat, for k = 0; LM.logp(a, b, k) otherwise
     (classes >= C_lm included).  After the step the context is (b, symbol(k)): a PREDICTED class 0 ([UNK]) therefore reads as begin
     of text to its successors;
  2'. a live unfinished entry proposes its N = min(16, max(W, top_n)) classes of largest LOGIT only (larger logit first, a tie to the
     lower class, a NaN logit counts as -inf); a proposal has acoustic' = acoustic + lp[k] and
     key = acoustic' + alpha * (lm + term) + beta * len' (evaluated left to right), len' = len + 1, len for eos.  A finished entry
     proposes itself alone with its key unchanged: it already holds the end-of-text term;
  3'. the W x N proposals of a sample are ranked by key, ties in (entry, class) order; rank < W with a key above -inf (a NaN key
     counts as -inf) survives.

score and logp stay acoustic, so prob stays a probability; one more output, fused [W], holds the key, and the entries come in
descending fused (-inf for a dead slot).  With alpha = beta = 0 the key is the acoustic score and, because N >= W, the six outputs are
the plain search's bit for bit -- up to one kind of rounding tie: if acoustic + lp of a proposal behind an entry's W-th rounds to the
very float of one in front of it and its class is lower, the (entry, class) tie rule takes it where the plain search never saw it.  The margin then also covers the pruning boundary: for every live unfinished entry the gap between
its N-th and (N + 1)-th logit, against one token's band.
"""
import numpy as np

CTC_DECODERS = ("greedy", "beam")
DEFAULT_BEAM_WIDTH = 8
DEFAULT_BEAM_TOP_N = 15

BEAM_MAX_T = 512             # frames mrn_ctc_beam_decode_f32 takes (the scorer's SCORE_MAX_T; two [W][T] token buffers in LDS)
BEAM_MAX_CLASSES = 65535     # classes are 16-bit tokens there
BEAM_MAX_WIDTH = 16          # entries live in lanes, candidates four per lane: W * (K + 1) <= 256
BEAM_MAX_TOP_N = 15

ATTN_DECODERS = ("greedy", "beam")
ATTN_BEAM_MAX_WIDTH = 16     # the 16 MFMA rows of a workgroup are 16 / W samples x W entries
ATTN_BEAM_MAX_STEPS = 512
ATTN_EOS = 3                 # AttnLabelConverter (tools/utils.py): [UNK]=0 [PAD]=1 [SOS]=2 [EOS]=3 -- the end token of the evaluation forwards


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


def attn_decode_options(opt):
    """(attn_decode, width) of an options object; absent keys are "greedy", 8.  The width is beam_width, the key the CTC decoder reads"""
    mode = getattr(opt, "attn_decode", "greedy")
    if mode not in ATTN_DECODERS:
        raise ValueError(f"attn_decode must be one of {ATTN_DECODERS}, got {mode!r}")
    return mode, _positive_int(opt, "beam_width", DEFAULT_BEAM_WIDTH)


def attn_beam_request(attn_beam, prediction, is_train):
    """the width an evaluation forward decodes by beam search with, or None: attn_beam is set, the head is an attention head, the call is
    an evaluation under no_grad"""
    import torch
    if attn_beam is None or "Attn" not in prediction or is_train or torch.is_grad_enabled():
        return None
    if isinstance(attn_beam, bool) or not isinstance(attn_beam, (int, np.integer)) or attn_beam < 1:
        raise ValueError(f"attn_beam must be an integer >= 1, got {attn_beam!r}")
    return int(attn_beam)


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


def _beam_one(x, W, K, lm=None, alpha=0.0, beta=0.0, dtype=np.float64):
    """one sample [T][C] -> [(prefix tuple, total)] in descending total; with a language model [(prefix tuple, total, fused)] in
    descending fused key.  All arithmetic in `dtype`"""
    T, C = x.shape
    k = min(K, C - 1)
    f = dtype
    ninf = f(-np.inf)
    x64 = x.astype(f)
    peak = x64.max(axis=1, keepdims=True)
    lp_all = x64 - (peak + np.log(np.exp(x64 - peak).sum(axis=1, keepdims=True)))
    prefix, pb, pnb = [()], np.zeros(1, dtype=f), np.full(1, ninf, dtype=f)
    e_lm = np.zeros(1, dtype=f)
    alpha, beta = f(alpha), f(beta)
    for t in range(T):
        lp = lp_all[t]
        S = _cut_off(x[t], k)
        rank = {int(c): r for r, c in enumerate(S)}
        n = len(prefix)
        total = np.logaddexp(pb, pnb)
        last = np.array([p[-1] if p else -1 for p in prefix], dtype=np.int64)
        in_S = np.array([int(c) in rank for c in last], dtype=bool)
        stay_pb = total + lp[0]
        stay_pnb = np.where(in_S, pnb + lp[np.maximum(last, 0)], ninf)
        ext = np.where(S[None, :] == last[:, None], pb[:, None], total[:, None]) + lp[S][None, :]        # [n][k]
        where = {p: i for i, p in enumerate(prefix)}
        dropped = np.zeros((n, k), dtype=bool)
        for j, p in enumerate(prefix):          # the one extension that spells entry j: from the entry that is p without its last class
            if p and p[-1] in rank and p[:-1] in where:
                i, r = where[p[:-1]], rank[p[-1]]
                stay_pnb[j] = np.logaddexp(stay_pnb[j], ext[i, r])
                dropped[i, r] = True
        cand_pb = np.concatenate([stay_pb[:, None], np.full((n, k), ninf, dtype=f)], axis=1).reshape(-1)      # candidate order (i, slot)
        cand_pnb = np.concatenate([stay_pnb[:, None], np.where(dropped, ninf, ext)], axis=1).reshape(-1)
        cand_total = np.logaddexp(cand_pb, cand_pnb)
        cand_total[~np.isfinite(cand_total)] = -np.inf
        key = cand_total
        if lm is not None:
            cand_lm = np.repeat(e_lm[:, None], k + 1, axis=1)                                              # a stay keeps lm_i
            cand_len = np.array([len(p) for p in prefix], dtype=f)[:, None] + np.array([0] + [1] * k, dtype=f)[None, :]
            for i, p in enumerate(prefix):
                a, b = p[-2] if len(p) > 1 else 0, p[-1] if p else 0
                for r, c in enumerate(S):
                    cand_lm[i, 1 + r] = e_lm[i] + lm.logp(a, b, int(c), f)
            cand_lm = cand_lm.reshape(-1)
            key = cand_total + alpha * cand_lm + beta * cand_len.reshape(-1)
            key[cand_total == -np.inf] = -np.inf
        keep = [q for q in np.argsort(-key, kind="stable")[:W] if key[q] > -np.inf]
        prefix = [prefix[q // (k + 1)] + ((int(S[q % (k + 1) - 1]),) if q % (k + 1) else ()) for q in keep]
        pb, pnb = cand_pb[keep], cand_pnb[keep]
        if lm is not None:
            e_lm = cand_lm[keep]
    total = np.logaddexp(pb, pnb)
    assert total.dtype == f
    if lm is None:
        return list(zip(prefix, total))
    eos = np.array([lm.logp(p[-2] if len(p) > 1 else 0, p[-1] if p else 0, 0, f) for p in prefix], dtype=f)
    fused = total + alpha * (e_lm + eos) + beta * np.array([len(p) for p in prefix], dtype=f)
    assert fused.dtype == f
    return [(prefix[i], total[i], fused[i]) for i in np.argsort(-fused, kind="stable")]


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


def ctc_beam_host(logits, W, K, lm=None, lm_weight=0.0, lm_bonus=0.0, dtype=np.float64):
    """float64 prefix beam search of logits [B][T][C] (numpy) -> (tokens int32 [B][W][T], length int32 [B][W], score float64 [B][W],
    path int64 [B][T], prob float32 [B][T]): the outputs of ops.ctc_beam_decode, for CPU tensors and for batches outside the
    kernel's limits.  Any W >= 1 and K >= 1.  With lm (a char_lm.CharLM), lm_weight >= 0 and a finite lm_bonus the search is the
    fused one of the module docstring and fused float64 [B][W] is a sixth output.  dtype = np.float32 runs all arithmetic, the
    model's included, in float32 (what float32 costs the kernel is measured on this form)"""
    logits = np.asarray(logits)
    if logits.ndim != 3 or logits.shape[1] < 1 or logits.shape[2] < 2 or W < 1 or K < 1:
        raise ValueError(f"ctc_beam_host needs logits [B][T >= 1][C >= 2], W >= 1 and K >= 1, got {logits.shape}, {W}, {K}")
    if dtype not in (np.float32, np.float64):
        raise ValueError(f"ctc_beam_host: dtype must be np.float32 or np.float64, got {dtype!r}")
    if lm is not None:
        lm_weight, lm_bonus = check_lm_weights(lm_weight, lm_bonus)
    B, T, _ = logits.shape
    tokens = np.zeros((B, W, T), dtype=np.int32)
    length = np.full((B, W), -1, dtype=np.int32)
    score = np.full((B, W), -np.inf, dtype=np.float64)
    fused = np.full((B, W), -np.inf, dtype=np.float64)
    path = np.zeros((B, T), dtype=np.int64)
    prob = np.ones((B, T), dtype=np.float32)
    for b in range(B):
        if lm is None and dtype is np.float64:
            entries = _beam_one(logits[b], W, K)
        else:
            entries = _beam_one(logits[b], W, K, lm, lm_weight, lm_bonus, dtype)
        for w, e in enumerate(entries):
            p = e[0]
            tokens[b, w, :len(p)] = p
            length[b, w] = len(p)
            score[b, w] = e[1]
            if lm is not None:
                fused[b, w] = e[2]
        if entries:
            path[b] = frame_path(entries[0][0], T)
        prob[b, 0] = np.float32(np.exp(score[b, 0]))
    return (tokens, length, score, path, prob) if lm is None else (tokens, length, score, path, prob, fused)


DEFAULT_LM_WEIGHT = 0.5
DEFAULT_LM_BONUS = 0.0
BEAM_LM_MAX_CLASSES = 65535      # C_lm: classes are 16-bit fields of a table key
BEAM_LM_MAX_SLOTS = 1 << 26


def check_lm_weights(lm_weight, lm_bonus):
    """(alpha, beta) as floats: alpha >= 0 and finite, beta finite; anything else is a ValueError"""
    for name, v in (("lm_weight", lm_weight), ("lm_bonus", lm_bonus)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if lm_weight < 0:
        raise ValueError(f"lm_weight must be >= 0, got {lm_weight!r}")
    return float(lm_weight), float(lm_bonus)


def lm_options(opt, attn):
    """(lm or None, lm_weight, lm_bonus) of an options object: opt.ctc_lm is absent / None (off) or a char_lm.CharLM, opt.lm_weight
    (default 0.5) and opt.lm_bonus (default 0) its weights.  The model fuses into the CTC beam search, so on a CTC head ctc_lm without
    ctc_decode='beam', or together with lexicon or candidates, is a ValueError; the attention head ignores the option"""
    from .char_lm import CharLM
    lm = getattr(opt, "ctc_lm", None)
    if lm is None or attn:
        return None, DEFAULT_LM_WEIGHT, DEFAULT_LM_BONUS
    if not isinstance(lm, CharLM):
        raise ValueError(f"ctc_lm must be a CharLM (modules/char_lm.py build_char_lm), got {type(lm).__name__}")
    if getattr(opt, "ctc_decode", "greedy") != "beam":
        raise ValueError("ctc_lm fuses into the prefix beam search: set ctc_decode='beam'")
    for key in ("lexicon", "candidates"):
        if getattr(opt, key, None) is not None:
            raise ValueError(f"ctc_lm and {key}: a closed-vocabulary decoder has no use for a language model, set one of them")
    return (lm,) + check_lm_weights(getattr(opt, "lm_weight", DEFAULT_LM_WEIGHT), getattr(opt, "lm_bonus", DEFAULT_LM_BONUS))


def beam_lm_supported(lm):
    """does mrn_ctc_beam_lm_decode_f32 take this model (beam_supported answers for the batch)"""
    return 1 <= lm.order <= 3 and lm.C_lm <= BEAM_LM_MAX_CLASSES and len(lm.keys) <= BEAM_LM_MAX_SLOTS


def _f64(v):
    return np.asarray(v.detach().cpu() if hasattr(v, "detach") else v).astype(np.float64)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


ATTN_LM_MAX_PROPOSALS = 16       # N: the candidate planes of attn_beam_lm_kernel are [16][16]


def attn_beam_host(sd, batch_H, sos, eos, width, batch_max_length, want_margin=False, lm=None, lm_weight=0.0, lm_bonus=0.0,
                   top_n=DEFAULT_BEAM_TOP_N):
    """float64 beam search on the attention head: sd = a state dict of modules/prediction.py Attention (tensors or arrays), batch_H
    [B][T][D] -> (tokens int32 [B][W][S], length int32 [B][W], score float64 [B][W], logp float64 [B][W][S], path int64 [B][S], prob
    float32 [B][S]): the outputs of ops.attn_beam_decode, for CPU tensors and as the kernel's yardstick.  Any width >= 1.
    want_margin adds margin float64 [B]: the smallest gap, over the steps, between neighbouring kept candidates and between the last
    kept and the best dropped one, divided by the step's token count (a score of n tokens is known to n times a token's band).
    With lm (a char_lm.CharLM), lm_weight >= 0, a finite lm_bonus and top_n >= 1 the search is the fused one of the module docstring:
    fused float64 [B][W] is a seventh output (in front of the margin), the entries come in descending fused, and the margin also
    covers the pruning boundary (the gap between a live unfinished entry's N-th and (N + 1)-th logit, against one token's band)"""
    if lm is None:
        return _attn_search_host("attn_beam_host", sd, batch_H, sos, eos, width, batch_max_length, None, want_margin)
    return _attn_fusion_host(sd, batch_H, sos, eos, width, batch_max_length, want_margin, lm, lm_weight, lm_bonus, top_n)


def attn_lm_proposals(width, top_n):
    """N, the classes an unfinished entry proposes: min(16, max(W, top_n)), and never fewer than W (the host form takes any width)"""
    if isinstance(top_n, bool) or not isinstance(top_n, (int, np.integer)) or top_n < 1:
        raise ValueError(f"top_n must be an integer >= 1, got {top_n!r}")
    return max(int(width), min(ATTN_LM_MAX_PROPOSALS, max(int(width), int(top_n))))


def _attn_fusion_host(sd, batch_H, sos, eos, width, batch_max_length, want_margin, lm, lm_weight, lm_bonus, top_n):
    """attn_beam_host with a language model: the fused search of the module docstring, sample by sample"""
    W, S = int(width), int(batch_max_length) + 1
    alpha, beta = check_lm_weights(lm_weight, lm_bonus)
    w = {k: _f64(v) for k, v in sd.items()}
    Hb = _f64(batch_H)
    if Hb.ndim != 3 or W < 1 or S < 1:
        raise ValueError(f"attn_beam_host needs batch_H [B][T][D], width >= 1 and batch_max_length >= 0, got {Hb.shape}, {W}, {S - 1}")
    N = attn_lm_proposals(W, top_n)
    B, T, D = Hb.shape
    C, Hd = w["generator.weight"].shape
    if not 0 <= eos < C:
        raise ValueError(f"eos={eos} outside the {C} classes")
    Hproj = Hb @ w["attention_cell.i2h.weight"].T
    h, c = np.zeros((B, W, Hd)), np.zeros((B, W, Hd))
    last = np.full((B, W), int(sos), dtype=np.int64)
    score = np.full((B, W), -np.inf)
    score[:, 0] = 0.0
    key = score.copy()
    ctx = np.zeros((B, W, 2), dtype=np.int64)
    lms = np.zeros((B, W))
    count = np.zeros((B, W), dtype=np.int64)
    finished = np.zeros((B, W), dtype=bool)
    tokens = np.full((B, W, S), eos, dtype=np.int32)
    logp = np.zeros((B, W, S))
    margin = np.full(B, np.inf)
    classes = np.arange(C)
    for s in range(S):
        if not ((score > -np.inf) & ~finished).any():
            break
        tok = np.where((last >= C) | (last < 0), 0, last)
        h2, c2, lp, x = _attn_cell_host(w, Hb, Hproj, h, c, tok, want_logits=True)
        nxt = [np.empty_like(a) for a in (h, c, last, score, key, ctx, lms, count, finished, tokens, logp)]
        for b in range(B):
            props = []                  # (key, entry, class, acoustic, lp of the class, lm sum, context, length)
            for i in range(W):
                if not score[b, i] > -np.inf:
                    continue
                if finished[b, i]:
                    props.append((key[b, i], i, eos, score[b, i], 0.0, lms[b, i], tuple(ctx[b, i]), count[b, i]))
                    continue
                ranked = np.lexsort((classes, -x[b, i]))[:N + 1]
                if len(ranked) > N:
                    with np.errstate(invalid="ignore"):
                        gap = x[b, i, ranked[N - 1]] - x[b, i, ranked[N]]
                    margin[b] = min(margin[b], gap if gap == gap else np.inf)
                pa, pb = int(ctx[b, i, 0]), int(ctx[b, i, 1])
                for k in map(int, ranked[:N]):
                    term = lm.logp(pa, pb, 0) if k == eos else lm.unk_logp if k == 0 else lm.logp(pa, pb, k)
                    acoustic = score[b, i] + lp[b, i, k]
                    acoustic = acoustic if acoustic == acoustic else -np.inf
                    total, n_chars = lms[b, i] + term, count[b, i] + (0 if k == eos else 1)
                    with np.errstate(invalid="ignore"):
                        kv = acoustic + alpha * total + beta * n_chars
                    props.append((kv if kv == kv else -np.inf, i, k, acoustic, lp[b, i, k], total, (pb, 0 if k == eos else k), n_chars))
            props.sort(key=lambda p: (-p[0], p[1], p[2]))
            top = np.array([p[0] for p in props[:W + 1]] + [-np.inf] * (W + 1 - min(len(props), W + 1)))
            with np.errstate(invalid="ignore"):
                gaps = np.where(top[:W] > -np.inf, top[:W] - top[1:], np.inf)
            margin[b] = min(margin[b], gaps.min() / (s + 1))
            for q in range(W):
                nh, nc, nlast, nscore, nkey, nctx, nlms, ncount, nfin, ntok, nlp = (a[b] for a in nxt)
                if q < len(props) and props[q][0] > -np.inf:
                    kv, i, k, acoustic, lpk, total, context, n_chars = props[q]
                    nh[q], nc[q], nlast[q], nscore[q], nkey[q] = h2[b, i], c2[b, i], k, acoustic, kv
                    nctx[q], nlms[q], ncount[q], nfin[q] = context, total, n_chars, k == eos
                    ntok[q], nlp[q] = tokens[b, i], logp[b, i]
                    ntok[q, s], nlp[q, s] = k, 0.0 if finished[b, i] else lpk
                else:
                    nh[q], nc[q], nlast[q], nscore[q], nkey[q] = 0.0, 0.0, eos, -np.inf, -np.inf
                    nctx[q], nlms[q], ncount[q], nfin[q], ntok[q], nlp[q] = 0, 0.0, 0, False, eos, 0.0
        h, c, last, score, key, ctx, lms, count, finished, tokens, logp = nxt
    alive = score > -np.inf
    is_eos = tokens == eos
    length = np.where(is_eos.any(axis=2), is_eos.argmax(axis=2) + 1, S).astype(np.int32)
    length[~alive] = -1
    out = (tokens, length, score, logp, tokens[:, 0].astype(np.int64), np.exp(logp[:, 0]).astype(np.float32), key)
    return out + (margin,) if want_margin else out


def _attn_search_host(who, sd, batch_H, sos, eos, width, batch_max_length, trie, want_margin):
    """attn_beam_host (trie None) and attn_lexicon_host (a Trie: the candidates of an unfinished entry are those its node admits, a node
    id is carried per entry, and `word` is one more output in front of the margin)"""
    W, S = int(width), int(batch_max_length) + 1
    w = {k: _f64(v) for k, v in sd.items()}
    Hb = _f64(batch_H)
    if Hb.ndim != 3 or W < 1 or S < 1:
        raise ValueError(f"{who} needs batch_H [B][T][D], width >= 1 and batch_max_length >= 0, got {Hb.shape}, {W}, {S - 1}")
    B, T, D = Hb.shape
    C, Hd = w["generator.weight"].shape
    if not 0 <= eos < C:
        raise ValueError(f"eos={eos} outside the {C} classes")
    Hproj = Hb @ w["attention_cell.i2h.weight"].T                         # [B][T][H]
    h, c = np.zeros((B, W, Hd)), np.zeros((B, W, Hd))
    last = np.full((B, W), int(sos), dtype=np.int64)
    score = np.full((B, W), -np.inf)
    score[:, 0] = 0.0
    finished = np.zeros((B, W), dtype=bool)
    tokens = np.full((B, W, S), eos, dtype=np.int32)
    logp = np.zeros((B, W, S))
    margin = np.full(B, np.inf)
    rows = np.arange(B)[:, None]
    node = np.zeros((B, W), dtype=np.int64)
    for s in range(S):
        if not ((score > -np.inf) & ~finished).any():
            break
        tok = np.where((last >= C) | (last < 0), 0, last)
        h2, c2, lp = _attn_cell_host(w, Hb, Hproj, h, c, tok)            # lp [B][W][C]
        with np.errstate(invalid="ignore", divide="ignore"):
            cand = score[:, :, None] + lp
        done = np.full((B, W, C), -np.inf)
        done[:, :, eos] = score
        if trie is not None:
            admitted, step_to = _admitted(trie, node, C, eos)
            cand = np.where(admitted, cand, -np.inf)
        cand = np.where(finished[:, :, None], done, cand)
        cand[np.isnan(cand)] = -np.inf
        flat = cand.reshape(B, W * C)                                     # candidate order (i, c)
        order = np.argsort(-flat, axis=1, kind="stable")[:, :W + 1]
        top = np.take_along_axis(flat, order, axis=1)
        if top.shape[1] < W + 1:
            top = np.concatenate([top, np.full((B, W + 1 - top.shape[1]), -np.inf)], axis=1)
        with np.errstate(invalid="ignore"):
            gaps = np.where(top[:, :W] > -np.inf, top[:, :W] - top[:, 1:W + 1], np.inf)
        margin = np.minimum(margin, gaps.min(axis=1) / (s + 1))
        keep = order[:, :W]
        if keep.shape[1] < W:
            keep = np.concatenate([keep, np.zeros((B, W - keep.shape[1]), dtype=keep.dtype)], axis=1)
        new_score = top[:, :W]
        par, cls = keep // C, keep % C
        alive = new_score > -np.inf
        was_done = finished[rows, par]
        tokens, logp = tokens[rows, par], logp[rows, par]
        tokens[:, :, s] = np.where(alive, cls, eos)
        logp[:, :, s] = np.where(alive & ~was_done, lp[rows, par, cls], 0.0)
        tokens[~alive], logp[~alive] = eos, 0.0
        h, c = h2[rows, par], c2[rows, par]
        if trie is not None:                                              # a finished or dead entry keeps its node
            node = np.where(alive & ~was_done, step_to[rows, par, cls], node[rows, par])
        last = np.where(alive, cls, eos)
        finished = alive & (cls == eos)
        score = new_score
    alive = score > -np.inf
    is_eos = tokens == eos
    length = np.where(is_eos.any(axis=2), is_eos.argmax(axis=2) + 1, S).astype(np.int32)
    length[~alive] = -1
    out = (tokens, length, score, logp, tokens[:, 0].astype(np.int64), np.exp(logp[:, 0]).astype(np.float32))
    if trie is not None:
        out += (np.where(alive, trie.word_of[node], -1).astype(np.int32),)
    return out + (margin,) if want_margin else out


# ---- lexicon-constrained decoding on the CTC heads ---------------------------------------------------------------------------------
# With opt.lexicon (a sequence of words) a CTC head is decoded to the lexicon word of largest log p(word | image).  The algorithm, which
# mrn_ctc_lexicon_decode_f32 (mrn_amd/csrc/ctc_lexicon.hip) runs in float32 and ctc_lexicon_host below in float64.  Per sample x[T][C],
# class 0 the blank, and word w = (c_1 .. c_L), 1 <= c_i <= C - 1, L >= 0:
#
#   lse[t] = m + log sum_k exp(x[t][k] - m), m the row maximum;  lp[t][k] = x[t][k] - lse[t];
#   states z_0 .. z_2L = blank, c_1, blank, ..., c_L, blank;
#   alpha_0(0) = lp[0][0], alpha_0(1) = lp[0][c_1] if L >= 1, every other alpha_0(s) = -inf;
#   alpha_t(s) = lp[t][z_s] + logaddexp(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if z_s != blank and z_s != z_{s-2}]);
#   score = logaddexp(alpha_{T-1}(2L), alpha_{T-1}(2L-1)), alpha_{T-1}(0) for L = 0;  logaddexp of all -inf is -inf, never NaN.
#
# That is -ctc_loss(log_softmax(x), w, blank=0); a word with L + repeats > T scores -inf.  Per sample the positions (the word index, or
# the slot of the sample's candidate row) are ranked by descending score, a tie to the lower position.  A position of score -inf is
# dead (an infeasible word, an unused candidate slot), and so is every position of a sample whose lse is NaN in any frame (a NaN or
# +inf logit, a frame of -inf).  Dead slots come last, with index -1 and score -inf.  Outputs: index int32 [B][n] (WORD indices:
# cand[b][slot] with candidate lists), score [B][n], score_all [B][Nc] (Nc = K with candidate lists, else N), and for the best entry the
# pair that goes wherever argmax_prob_lastdim's goes: path [B][T] = frame_path(word, T), prob [B][T] = [exp(score), 1, 1, ...]; a sample
# without a live word has an all-blank path and prob[0] = 0.
LEXICON_MAX_T = 512           # frames mrn_ctc_lexicon_decode_f32 takes (the scorer's SCORE_MAX_T)
LEXICON_MAX_CLASSES = 65535
LEXICON_MAX_LENGTH = 31       # state s of a word lives in lane s: 2 L + 1 <= 64, the limit of the 64-state CTC loss kernel
LEXICON_MAX_WORDS = 1 << 20
LEXICON_MAX_TOP_N = 16
DEFAULT_LEXICON_TOP_N = 1


def lexicon_options(opt):
    """(words or None, n) of an options object: opt.lexicon is absent / None (off) or a sequence of str, opt.lexicon_top_n (default 1)
    the entries returned per sample"""
    n = _positive_int(opt, "lexicon_top_n", DEFAULT_LEXICON_TOP_N)
    words = getattr(opt, "lexicon", None)
    if words is None:
        return None, n
    if isinstance(words, (str, bytes)) or not hasattr(words, "__iter__"):
        raise ValueError(f"lexicon must be a sequence of words (str), got {type(words).__name__}")
    words = list(words)
    for w in words:
        if not isinstance(w, str):
            raise ValueError(f"lexicon must be a sequence of words (str), got an entry {w!r}")
    return words, n


def lexicon_supported(prediction, T, C, Lmax, N, n):
    """does mrn_ctc_lexicon_decode_f32 score N words of at most Lmax classes against T frames of C classes of a `prediction` head and
    return n entries per sample"""
    return ("CTC" in prediction and 1 <= T <= LEXICON_MAX_T and 2 <= C <= LEXICON_MAX_CLASSES and 0 <= Lmax <= LEXICON_MAX_LENGTH
            and 1 <= N <= LEXICON_MAX_WORDS and 1 <= n <= LEXICON_MAX_TOP_N)


def encode_lexicon(converter, words):
    """words -> (tokens int32 [N][Lmax] (0 behind a word), lengths int32 [N], kept_words): the words a CTC converter can spell, in
    their order, duplicates kept.  A word with a character outside converter.dict, or one of the [UNK] / [CTCblank] class, is dropped;
    ValueError if nothing is left"""
    table = converter.dict
    banned = {0, table.get("[UNK]")}
    rows, kept = [], []
    for w in words:
        row = [table.get(ch) for ch in w]
        if any(c is None or c in banned for c in row):
            continue
        rows.append(row)
        kept.append(w)
    if not kept:
        raise ValueError(f"lexicon: none of the {len(list(words))} words can be spelled with the converter's characters")
    lengths = np.fromiter((len(r) for r in rows), dtype=np.int32, count=len(rows))
    tokens = np.zeros((len(rows), max(int(lengths.max()), 1)), dtype=np.int32)
    for i, r in enumerate(rows):
        tokens[i, :len(r)] = r
    return tokens, lengths, kept


def _lexicon_scores(lp, tokens, lengths):
    """log p(word | frames) of M words against lp [T][C] (float64 log-probabilities) -> float64 [M], vectorised over the words"""
    T = lp.shape[0]
    M, Lm = tokens.shape
    S = 2 * Lm + 1
    z = np.zeros((M, S), dtype=np.int64)
    z[:, 1::2] = tokens
    valid = np.arange(S)[None, :] < (2 * lengths + 1)[:, None]
    z[~valid] = 0
    skip = np.zeros((M, S), dtype=bool)
    skip[:, 3::2] = tokens[:, 1:] != tokens[:, :-1]
    skip &= valid
    neg = np.full((M, 2), -np.inf)
    alpha = np.full((M, S), -np.inf)
    alpha[:, 0] = lp[0, 0]
    if Lm:
        alpha[:, 1] = np.where(lengths >= 1, lp[0, z[:, 1]], -np.inf)
    for t in range(1, T):
        a1 = np.concatenate([neg[:, :1], alpha[:, :-1]], axis=1)
        a2 = np.where(skip, np.concatenate([neg, alpha[:, :-2]], axis=1)[:, :S], -np.inf)
        m = np.maximum(np.maximum(alpha, a1), a2)
        m0 = np.where(m > -np.inf, m, 0.0)
        with np.errstate(divide="ignore"):
            acc = m0 + np.log(np.exp(alpha - m0) + np.exp(a1 - m0) + np.exp(a2 - m0))      # all -inf: 0 + log(0) = -inf
        alpha = np.where(valid, acc + lp[t][z], -np.inf)
    rows = np.arange(M)
    e1 = alpha[rows, 2 * lengths]
    e2 = np.where(lengths >= 1, alpha[rows, np.maximum(2 * lengths - 1, 0)], -np.inf)
    m = np.maximum(e1, e2)
    m0 = np.where(m > -np.inf, m, 0.0)
    with np.errstate(divide="ignore"):
        return m0 + np.log(np.exp(e1 - m0) + np.exp(e2 - m0))


def ctc_lexicon_host(logits, lex_tokens, lex_len, n, cand=None):
    """float64 lexicon decoding of logits [B][T][C] (numpy) against the words lex_tokens int [N][Lmax] / lex_len int [N], or per sample
    against the words cand int [B][K] names (-1 = unused slot) -> (index int32 [B][n], score float64 [B][n], score_all float64
    [B][Nc], path int64 [B][T], prob float32 [B][T]): the outputs of ops.ctc_lexicon_decode, for CPU tensors and for batches outside
    the kernel's limits.  Any word length, any N >= 1 and n >= 1"""
    logits = np.asarray(logits)
    tokens = np.asarray(lex_tokens).astype(np.int64)
    lengths = np.asarray(lex_len).astype(np.int64)
    if logits.ndim != 3 or logits.shape[1] < 1 or logits.shape[2] < 2 or n < 1:
        raise ValueError(f"ctc_lexicon_host needs logits [B][T >= 1][C >= 2] and n >= 1, got {logits.shape}, {n}")
    B, T, C = logits.shape
    if tokens.ndim != 2 or lengths.shape != tokens.shape[:1] or len(lengths) < 1:
        raise ValueError(f"ctc_lexicon_host needs tokens [N >= 1][Lmax] and lengths [N], got {tokens.shape}, {lengths.shape}")
    N, Lmax = tokens.shape
    if lengths.min() < 0 or lengths.max() > Lmax:
        raise ValueError(f"ctc_lexicon_host: word lengths outside 0..{Lmax}")
    tokens = np.where(np.arange(Lmax)[None, :] < lengths[:, None], tokens, 0)
    used = tokens[np.arange(Lmax)[None, :] < lengths[:, None]]
    if used.size and (used.min() < 1 or used.max() > C - 1):
        raise ValueError(f"ctc_lexicon_host: word tokens outside 1..{C - 1}")
    if cand is not None:
        cand = np.asarray(cand).astype(np.int64)
        if cand.ndim != 2 or cand.shape[0] != B or cand.shape[1] < 1 or (cand.size and (cand.min() < -1 or cand.max() > N - 1)):
            raise ValueError(f"ctc_lexicon_host needs cand [B][K >= 1] with entries in -1..{N - 1}, got {cand.shape}")
    Nc = N if cand is None else cand.shape[1]
    index = np.full((B, n), -1, dtype=np.int32)
    score = np.full((B, n), -np.inf, dtype=np.float64)
    score_all = np.full((B, Nc), -np.inf, dtype=np.float64)
    path = np.zeros((B, T), dtype=np.int64)
    prob = np.ones((B, T), dtype=np.float32)
    x64 = logits.astype(np.float64)
    for b in range(B):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            peak = x64[b].max(axis=1, keepdims=True)
            lse = peak + np.log(np.exp(x64[b] - peak).sum(axis=1, keepdims=True))
        words = np.arange(N) if cand is None else cand[b]
        if not np.isnan(lse).any():
            used = np.flatnonzero(words >= 0)
            if used.size:
                with np.errstate(invalid="ignore"):
                    lp = x64[b] - lse
                s = _lexicon_scores(lp, tokens[words[used]], lengths[words[used]])
                score_all[b, used] = np.where(np.isnan(s), -np.inf, s)
        order = [q for q in np.argsort(-score_all[b], kind="stable")[:n] if score_all[b, q] > -np.inf]
        for r, q in enumerate(order):
            index[b, r] = words[q]
            score[b, r] = score_all[b, q]
        if order:
            w = int(words[order[0]])
            path[b] = frame_path([int(c) for c in tokens[w, :lengths[w]]], T)
            prob[b, 0] = np.float32(np.exp(score[b, 0]))
        else:
            prob[b, 0] = 0.0
    return index, score, score_all, path, prob


# ---- lexicon-constrained decoding on the attention head ------------------------------------------------------------------------------
# With opt.attn_lexicon (a sequence of words) an attention head is decoded by the beam search above walked along a trie of the lexicon:
# mrn_attn_lexicon_decode_* (mrn_amd/csrc/attn_decode.hip attn_lexicon_kernel) runs it in float32, all steps of all experts in one launch,
# attn_lexicon_host below in float64.  (Scoring every (sample, word) pair, as the CTC lexicon decoder does, would give every pair a
# recurrent roll-out of its own.)  The trie: node 0 is the root, nodes are numbered breadth-first with a node's children in ascending
# class order, so the numbering does not depend on the order of the words and a child's index is above its parent's; the children of
# node n are the edges child_off[n] ... child_off[n + 1] - 1 with class child_tok[e] and node child_node[e]; word_of[n] is the lowest
# lexicon index of a word that ends at n, else -1.  Every entry carries a node, the start entry the root.  The search is the beam
# search with step 2 replaced:
#
#   2. a live unfinished entry i at node n gives the candidates (i, child_tok[e]) with score_i + lp[child_tok[e]] for the children e
#      of n whose class is below num_class, and (i, eos) with score_i + lp[eos] if a word ends at n (word_of[n] >= 0); lp is still the
#      log-softmax over all num_class classes: nothing is renormalised, so a finished entry's score is log p(word, eos | image) of the
#      model.  A finished entry gives (i, eos) with its score unchanged, as before.  An entry without a candidate contributes nothing.
#   4. a survivor takes its parent's new (h, c) and the chosen child's node; a finished or dead entry keeps its node.
#
# With W >= the number of distinct words nothing is pruned and entry 0 is the exact arg-max over the lexicon.  The longest word must
# fit: trie.depth <= batch_max_length, and then every live entry ends in eos within the S steps.  A sample may end without a live
# entry (an expert whose classes stop below every word's first class): path all eos, prob all 1, every length -1, every score -inf.
# Outputs: the beam's six and word int32 [W] = word_of of the entry's node, -1 for a dead slot.
from collections import namedtuple

Trie = namedtuple("Trie", "child_off child_tok child_node word_of depth words")      # words: the size of the lexicon word_of indexes
ATTN_SPECIALS = ("[UNK]", "[PAD]", "[SOS]", "[EOS]")


def attn_lexicon_options(opt):
    """(words or None, width) of an options object: opt.attn_lexicon is absent / None (off) or a sequence of str, the width is
    opt.beam_width (default 8) whatever attn_decode says: a lexicon makes the search a constrained beam search"""
    width = _positive_int(opt, "beam_width", DEFAULT_BEAM_WIDTH)
    words = getattr(opt, "attn_lexicon", None)
    if words is None:
        return None, width
    if isinstance(words, (str, bytes)) or not hasattr(words, "__iter__"):
        raise ValueError(f"attn_lexicon must be a sequence of words (str), got {type(words).__name__}")
    words = list(words)
    for w in words:
        if not isinstance(w, str):
            raise ValueError(f"attn_lexicon must be a sequence of words (str), got an entry {w!r}")
    return words, width


def encode_attn_lexicon(converter, words, batch_max_length):
    """words -> (tokens int32 [N][Lmax] (0 behind a word), lengths int32 [N], kept_words): the words an AttnLabelConverter can spell, in
    their order, duplicates kept, the empty word too.  A word with a character outside converter.dict, or one of the [UNK] / [PAD] /
    [SOS] / [EOS] classes, or longer than batch_max_length (its [EOS] would not fit the S = batch_max_length + 1 steps) is dropped;
    ValueError if nothing is left.  Case-sensitive, like encode_lexicon"""
    table = converter.dict
    banned = {table[s] for s in ATTN_SPECIALS if s in table}
    words = list(words)
    rows, kept = [], []
    for w in words:
        row = [table.get(ch) for ch in w]
        if len(row) > batch_max_length or any(c is None or c in banned for c in row):
            continue
        rows.append(row)
        kept.append(w)
    if not kept:
        raise ValueError(f"attn_lexicon: none of the {len(words)} words can be spelled with the converter's characters within "
                         f"{batch_max_length} of them")
    lengths = np.fromiter((len(r) for r in rows), dtype=np.int32, count=len(rows))
    tokens = np.zeros((len(rows), max(int(lengths.max()), 1)), dtype=np.int32)
    for i, r in enumerate(rows):
        tokens[i, :len(r)] = r
    return tokens, lengths, kept


def build_trie(tokens, lengths):
    """tokens int [N][Lmax], lengths int [N] (N >= 1, classes >= 0) -> Trie of int32 arrays: child_off [M + 1], child_tok [M - 1],
    child_node [M - 1] in CSR form, word_of [M] (the lowest index of a word ending at the node, else -1), depth = the longest word,
    words = N.  Nodes are numbered breadth-first, children in ascending class order; level by level over the sorted words, no
    per-node work"""
    tokens = np.asarray(tokens).astype(np.int64)
    lengths = np.asarray(lengths).astype(np.int64)
    if tokens.ndim != 2 or lengths.shape != tokens.shape[:1] or len(lengths) < 1:
        raise ValueError(f"build_trie needs tokens [N >= 1][Lmax] and lengths [N], got {tokens.shape}, {lengths.shape}")
    N, Lmax = tokens.shape
    if lengths.min() < 0 or lengths.max() > Lmax:
        raise ValueError(f"build_trie: word lengths outside 0..{Lmax}")
    used = np.arange(Lmax)[None, :] < lengths[:, None]
    if (tokens[used] < 0).any():
        raise ValueError("build_trie: negative class in a word")
    padded = np.where(used, tokens, -1)
    depth = int(lengths.max())
    order = np.lexsort(padded.T[::-1]) if Lmax else np.arange(N)        # the words in lexicographic order, a prefix before its extensions
    at = np.zeros(N, dtype=np.int64)               # node of every word's prefix of the current length; a word that has ended keeps its node
    parents, toks = [], []
    M = 1
    for d in range(depth):
        act = order[lengths[order] > d]            # in sorted order (node of the prefix, next class) is non-decreasing: one run per child
        par, tk = at[act], padded[act, d]
        new = np.ones(len(act), dtype=bool)
        new[1:] = (par[1:] != par[:-1]) | (tk[1:] != tk[:-1])
        at[act] = M + np.cumsum(new) - 1
        parents.append(par[new])
        toks.append(tk[new])
        M += int(new.sum())
    word_of = np.full(M, N, dtype=np.int64)
    np.minimum.at(word_of, at, np.arange(N))
    word_of[word_of == N] = -1
    parents = np.concatenate(parents) if parents else np.zeros(0, dtype=np.int64)
    child_tok = np.concatenate(toks) if toks else np.zeros(0, dtype=np.int64)
    child_off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(np.bincount(parents, minlength=M), out=child_off[1:])
    return Trie(child_off.astype(np.int32), child_tok.astype(np.int32), np.arange(1, M, dtype=np.int32), word_of.astype(np.int32),
                depth, N)


def check_trie(trie):
    """the host check every trie passes once before it is uploaded (ops.upload_trie): the kernel trusts the arrays, so whatever could
    send a read outside them is a ValueError here -- int32, one-dimensional and contiguous; offsets monotone from 0 to E = M - 1;
    parent < child_node[e] < M; classes >= 0; -1 <= word_of < words; no path from the root longer than depth.  -> (M, E)"""
    arrays = {k: getattr(trie, k) for k in ("child_off", "child_tok", "child_node", "word_of")}
    for k, a in arrays.items():
        if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"trie: {k} must be a contiguous one-dimensional int32 array")
    off, tok, child, word_of = arrays.values()
    M, E = len(word_of), len(tok)
    depth, words = trie.depth, trie.words
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (depth, words)) or depth < 0 or words < 1:
        raise ValueError(f"trie: depth={depth!r} and words={words!r} must be integers >= 0 and >= 1")
    if M < 1 or len(off) != M + 1 or len(child) != E or E != M - 1:
        raise ValueError(f"trie: {M} nodes need {M + 1} offsets and {M - 1} edges, got {len(off)}, {E} classes and {len(child)} children")
    if off[0] != 0 or off[-1] != E or (np.diff(off) < 0).any():
        raise ValueError(f"trie: child_off must rise from 0 to {E}")
    parent = np.repeat(np.arange(M), np.diff(off))
    if E and ((child <= parent).any() or (child >= M).any()):
        raise ValueError(f"trie: child_node must lie between its parent and {M}")
    if E and tok.min() < 0:
        raise ValueError("trie: negative class in child_tok")
    if word_of.min() < -1 or word_of.max() >= words:
        raise ValueError(f"trie: word_of outside -1..{words - 1}")
    level = np.zeros(M, dtype=np.int64)             # longest path from the root: a child is above its parent, so depth + 1 sweeps settle it
    for _ in range(int(depth) + 1):
        deeper = level.copy()
        np.maximum.at(deeper, child, level[parent] + 1)
        if np.array_equal(deeper, level):
            break
        level = deeper
    else:
        raise ValueError(f"trie: a path from the root is longer than depth={depth}")
    return M, E


def _admitted(trie, node, C, eos):
    """node int [B][W] -> (admitted bool [B][W][C], step_to int64 [B][W][C]): the classes the entries' nodes admit and the node each
    leads to, a ragged expand of the CSR rows; eos is admitted where a word ends and leads nowhere"""
    B, W = node.shape
    flat = node.reshape(-1)
    lo = trie.child_off[flat].astype(np.int64)
    count = trie.child_off[flat + 1] - lo
    row = np.repeat(np.arange(B * W), count)
    edge = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count) + np.repeat(lo, count)
    cls = trie.child_tok[edge].astype(np.int64)
    ok = cls < C
    admitted = np.zeros((B * W, C), dtype=bool)
    step_to = np.repeat(flat[:, None], C, axis=1)
    admitted[row[ok], cls[ok]] = True
    step_to[row[ok], cls[ok]] = trie.child_node[edge[ok]]
    ends = trie.word_of[flat] >= 0
    admitted[ends, eos] = True
    step_to[ends, eos] = flat[ends]
    return admitted.reshape(B, W, C), step_to.reshape(B, W, C)


def attn_lexicon_host(sd, batch_H, sos, eos, width, batch_max_length, trie, want_margin=False):
    """float64 lexicon-constrained beam search on the attention head: the operands of attn_beam_host and a Trie (build_trie) ->
    attn_beam_host's six outputs and word int32 [B][W] (word_of of the entry's node, -1 for a dead slot): the outputs of
    ops.attn_lexicon_decode, for CPU tensors and as the kernel's yardstick.  want_margin adds margin float64 [B] as attn_beam_host
    does, the gaps taken over admissible candidates only"""
    check_trie(trie)
    if trie.depth > int(batch_max_length):
        raise ValueError(f"attn_lexicon_host: the longest word has {trie.depth} classes, more than batch_max_length={batch_max_length}")
    return _attn_search_host("attn_lexicon_host", sd, batch_H, sos, eos, width, batch_max_length, trie, want_margin)


def attn_lexicon_request(attn_lexicon, width):
    """the trie handle an evaluation forward constrains its beam search with, or None; without a beam width the handle is an error"""
    if attn_lexicon is not None and width is None:
        raise ValueError("attn_lexicon constrains the beam search of attn_beam=<width>: pass both (evaluation under no_grad, attention head)")
    return attn_lexicon


# ---- exact scoring of per-sample candidate words on the attention head -----------------------------------------------------------------
# With opt.candidates every image is decoded against a word list of its own (the protocol of IIIT5K-50, SVT-50, IC03-50).  A CTC head
# takes ctc_lexicon_host / mrn_ctc_lexicon_decode_f32 with a candidate table.  On the attention head B x K roll-outs are affordable
# where N x B were not: mrn_attn_score_candidates_* (mrn_amd/csrc/attn_decode.hip attn_score_kernel) scores every (sample, slot) pair
# by a teacher-forced roll-out in float32, all steps of all experts in one launch, attn_candidates_host below in float64.  For sample
# b and slot k, word w = cand[b][k] with classes c_1 .. c_L (L >= 0):
#
#   the inputs of steps 0 .. L are sos, c_1, .., c_L (a start token >= num_class or < 0 counts as 0, as in greedy);
#   the targets are c_1, .., c_L, eos;
#   lp_s = log_softmax(generator(h_s)) over the num_class classes, a NaN logit counting as -inf;
#   score = sum_s lp_s[target_s] = log p(word, eos | image) of the model, exactly: no beam, nothing pruned, nothing renormalised.
#
# A slot is dead, with index -1 and score -inf, when it is unused (-1), when a class of its word is not below num_class, or when its
# score is -inf or NaN.  Per sample the slots are ranked as ctc_lexicon_host ranks them: descending score, a tie to the lower slot,
# dead slots last.  Outputs, in ops.ctc_lexicon_decode's order: index int32 [B][n] (WORD indices), score [B][n], score_all [B][K], and
# for the best entry path int64 [B][S] (its classes, then eos) and prob float32 [B][S] (its per-token probabilities, 1 behind the
# first eos) -- the form attn_beam_decode gives its best entry; a sample without a live slot gets path all eos and prob all 0 (the
# empty prediction with confidence 0).  Optional: logp [B][K][S], the per-token log-probabilities, 0 behind a word's eos and in a
# dead slot.
CANDIDATES_MAX_STEPS = 512
CANDIDATES_MAX_CLASSES = 65535
CANDIDATES_MAX_WORDS = 1 << 20
CANDIDATES_MAX_TOP_N = 16


def candidates_options(opt):
    """(candidates or None, n) of an options object: opt.candidates is absent / None (off), a callable (the batch's list of label
    strings -> one sequence of words per sample) or a dict label -> words; n = opt.lexicon_top_n (default 1).  The option replaces the
    decoding of either head, so together with lexicon, attn_lexicon, ctc_decode='beam' or attn_decode='beam' it is a ValueError"""
    n = _positive_int(opt, "lexicon_top_n", DEFAULT_LEXICON_TOP_N)
    cands = getattr(opt, "candidates", None)
    if cands is None:
        return None, n
    if not callable(cands) and not isinstance(cands, dict):
        raise ValueError(f"candidates must be a callable (labels -> word lists) or a dict label -> words, got {type(cands).__name__}")
    for key, on in (("lexicon", getattr(opt, "lexicon", None) is not None), ("attn_lexicon", getattr(opt, "attn_lexicon", None) is not None),
                    ("ctc_decode='beam'", getattr(opt, "ctc_decode", "greedy") == "beam"),
                    ("attn_decode='beam'", getattr(opt, "attn_decode", "greedy") == "beam")):
        if on:
            raise ValueError(f"candidates and {key} both replace the head's decoding: set one of them")
    return cands, n


def candidate_lists(candidates, labels):
    """the word lists of a batch: one list of str per label.  A dict without a label, a callable that returns another number of lists
    than labels, and an entry that is no word are ValueErrors"""
    labels = list(labels)
    if isinstance(candidates, dict):
        missing = [gt for gt in labels if gt not in candidates]
        if missing:
            raise ValueError(f"candidates: no word list for the label {missing[0]!r}")
        lists = [candidates[gt] for gt in labels]
    else:
        lists = list(candidates(labels))
        if len(lists) != len(labels):
            raise ValueError(f"candidates: {len(lists)} word lists for {len(labels)} labels")
    out = []
    for words in lists:
        if isinstance(words, (str, bytes)) or not hasattr(words, "__iter__"):
            raise ValueError(f"candidates: a sample's words must be a sequence of str, got {type(words).__name__}")
        words = list(words)
        for w in words:
            if not isinstance(w, str):
                raise ValueError(f"candidates: a sample's words must be a sequence of str, got an entry {w!r}")
        out.append(words)
    return out


class CandidateTable:
    """the word table of one validation() call: the union of the candidate lists, encoded once by the head's lexicon encoder
    (encode_lexicon / encode_attn_lexicon: words the converter cannot spell are dropped); rows() gives a batch's cand int32 [B][K]"""

    def __init__(self, converter, lists, attn, batch_max_length):
        union = list(dict.fromkeys(w for words in lists for w in words))
        if attn:
            self.tokens, self.lengths, self.words = encode_attn_lexicon(converter, union, batch_max_length)
        else:
            self.tokens, self.lengths, self.words = encode_lexicon(converter, union)
        self.index = {w: i for i, w in enumerate(self.words)}

    def rows(self, lists):
        """cand int32 [B][K] of a batch: the table indices of every sample's words in their order (a dropped or unknown word leaves no
        slot), -1 behind; K >= 1"""
        rows = [[self.index[w] for w in words if w in self.index] for words in lists]
        K = max([len(r) for r in rows] + [1])
        cand = np.full((len(rows), K), -1, dtype=np.int32)
        for b, r in enumerate(rows):
            cand[b, :len(r)] = r
        return cand


def check_word_table(lex_tokens, lex_len, cand, B, S):
    """the host check of a word table and a candidate table (numpy) before any launch: int tokens [N >= 1][Lmax] with classes >= 0,
    lengths [N] in 0 .. min(Lmax, S - 1), cand [B][K >= 1] in -1 .. N - 1 -> (N, Lmax, K); anything else is a ValueError"""
    tokens, lengths, cand = np.asarray(lex_tokens), np.asarray(lex_len), np.asarray(cand)
    if tokens.ndim != 2 or lengths.shape != tokens.shape[:1] or len(lengths) < 1 or len(lengths) > CANDIDATES_MAX_WORDS:
        raise ValueError(f"candidates: a word table needs tokens [1 <= N <= 2^20][Lmax] and lengths [N], got {tokens.shape}, {lengths.shape}")
    N, Lmax = tokens.shape
    if lengths.min() < 0 or lengths.max() > min(Lmax, S - 1):
        raise ValueError(f"candidates: word lengths outside 0..{min(Lmax, S - 1)} (the longest word and its end token take S = {S} steps)")
    if (tokens[np.arange(Lmax)[None, :] < lengths[:, None]] < 0).any():
        raise ValueError("candidates: negative class in a word")
    if cand.ndim != 2 or cand.shape[0] != B or cand.shape[1] < 1:
        raise ValueError(f"candidates: a candidate table needs cand [B = {B}][K >= 1], got {cand.shape}")
    if cand.size and (cand.min() < -1 or cand.max() > N - 1):
        raise ValueError(f"candidates: a candidate index outside -1..{N - 1}")
    return N, Lmax, cand.shape[1]


def _attn_cell_host(w, Hb, Hproj, h, c, tok, want_logits=False):
    """one step of the attention cell of modules/prediction.py in float64 on rows [B][R]: h, c [B][R][H], tok int [B][R] -> (h, c,
    log-softmax of the generator [B][R][C] with a NaN logit counting as -inf) -- _attn_search_host's arithmetic in its order.
    want_logits: the logits (NaN as -inf) are a fourth output"""
    a = "attention_cell."
    hp = h @ w[a + "h2h.weight"].T + w[a + "h2h.bias"]
    e = np.tanh(Hproj[:, None] + hp[:, :, None, :]) @ w[a + "score.weight"][0]
    e = np.exp(e - e.max(axis=2, keepdims=True))
    alpha = e / e.sum(axis=2, keepdims=True)
    ctx = np.einsum("bwt,btd->bwd", alpha, Hb)
    g = (np.concatenate([ctx, w["char_embeddings.weight"][tok]], axis=2) @ w[a + "rnn.weight_ih"].T + w[a + "rnn.bias_ih"]
         + h @ w[a + "rnn.weight_hh"].T + w[a + "rnn.bias_hh"])
    gi, gf, gg, go = np.split(g, 4, axis=2)
    c2 = _sigmoid(gf) * c + _sigmoid(gi) * np.tanh(gg)
    h2 = _sigmoid(go) * np.tanh(c2)
    x = h2 @ w["generator.weight"].T + w["generator.bias"]
    x = np.where(np.isnan(x), -np.inf, x)
    peak = x.max(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        lp = x - (peak + np.log(np.exp(x - peak).sum(axis=2, keepdims=True)))
    return (h2, c2, lp, x) if want_logits else (h2, c2, lp)


def rank_candidates(score_all, cand, n):
    """score_all float [B][K] (-inf = dead), cand int [B][K] -> (index int32 [B][n], score [B][n], best slot int64 [B], -1 without a live
    slot): descending score, a tie to the lower slot, dead slots last with index -1 and score -inf"""
    B, K = score_all.shape
    index = np.full((B, n), -1, dtype=np.int32)
    score = np.full((B, n), -np.inf, dtype=score_all.dtype)
    best = np.full(B, -1, dtype=np.int64)
    order = np.argsort(-score_all, axis=1, kind="stable")[:, :n]
    for b in range(B):
        live = [q for q in order[b] if score_all[b, q] > -np.inf]
        index[b, :len(live)] = cand[b, live]
        score[b, :len(live)] = score_all[b, live]
        if live:
            best[b] = live[0]
    return index, score, best


def attn_candidates_host(sd, batch_H, sos, eos, lex_tokens, lex_len, cand, n, batch_max_length, want_logp=False):
    """float64 exact scoring of per-sample candidate words on the attention head: sd = a state dict of modules/prediction.py Attention,
    batch_H [B][T][D], the word table lex_tokens int [N][Lmax] / lex_len int [N], cand int [B][K] (-1 = unused slot), n entries per
    sample -> (index int32 [B][n], score float64 [B][n], score_all float64 [B][K], path int64 [B][S], prob float32 [B][S]) and, with
    want_logp, logp float64 [B][K][S]: the outputs of ops.attn_score_candidates, for CPU tensors and as the kernel's yardstick.  Any
    K >= 1 and n >= 1"""
    S, n = int(batch_max_length) + 1, int(n)
    w = {k: _f64(v) for k, v in sd.items()}
    Hb = _f64(batch_H)
    if Hb.ndim != 3 or S < 1 or n < 1:
        raise ValueError(f"attn_candidates_host needs batch_H [B][T][D], n >= 1 and batch_max_length >= 0, got {Hb.shape}, {n}, {S - 1}")
    B, T, D = Hb.shape
    C, Hd = w["generator.weight"].shape
    if not 0 <= eos < C:
        raise ValueError(f"eos={eos} outside the {C} classes")
    tokens, lengths, cand = np.asarray(lex_tokens).astype(np.int64), np.asarray(lex_len).astype(np.int64), np.asarray(cand).astype(np.int64)
    N, Lmax, K = check_word_table(tokens, lengths, cand, B, S)
    tokens = np.where(np.arange(Lmax)[None, :] < lengths[:, None], tokens, 0)
    spelled = (tokens < C).all(axis=1)                                     # a class this head does not have: the word is dead here
    word = np.maximum(cand, 0)
    live = (cand >= 0) & spelled[word]                                     # [B][K]
    L = np.where(live, lengths[word], -1)
    text = np.full((B, K, S), eos, dtype=np.int64)                         # the targets: the word's classes, then eos
    text[:, :, :Lmax] = np.where(np.arange(Lmax)[None, None, :] < L[:, :, None], tokens[word], eos)[:, :, :S]
    text[~live] = eos
    first = int(sos)
    first = 0 if first >= C or first < 0 else first
    Hproj = Hb @ w["attention_cell.i2h.weight"].T
    h, c = np.zeros((B, K, Hd)), np.zeros((B, K, Hd))
    logp = np.zeros((B, K, S))
    rows, slots = np.arange(B)[:, None], np.arange(K)[None, :]
    for s in range(int(L.max()) + 1):
        tok = np.full((B, K), first, dtype=np.int64) if s == 0 else text[:, :, s - 1]
        h, c, lp = _attn_cell_host(w, Hb, Hproj, h, c, tok)
        logp[:, :, s] = np.where(s <= L, lp[rows, slots, text[:, :, s]], 0.0)
    with np.errstate(invalid="ignore"):
        score_all = logp.sum(axis=2)
    dead = ~live | np.isnan(score_all) | (score_all == -np.inf)
    score_all[dead] = -np.inf
    logp[dead] = 0.0
    index, score, best = rank_candidates(score_all, cand, n)
    path = np.full((B, S), eos, dtype=np.int64)
    prob = np.zeros((B, S), dtype=np.float32)
    has = best >= 0
    path[has] = text[has, best[has]]
    prob[has] = np.exp(logp[has, best[has]]).astype(np.float32)
    out = (index, score, score_all, path, prob)
    return out + (logp,) if want_logp else out


def attn_candidates_request(attn_candidates, prediction, is_train, attn_beam=None):
    """the candidate handle an evaluation forward scores its batch against, or None: attn_candidates is set, the head is an attention
    head, the call is an evaluation under no_grad.  Together with a beam width the handle is an error: both replace greedy decoding"""
    import torch
    if attn_candidates is None:
        return None
    if attn_beam is not None:
        raise ValueError("attn_candidates and attn_beam both replace the greedy pair of an evaluation forward: pass one of them")
    if "Attn" not in prediction or is_train or torch.is_grad_enabled():
        return None
    return attn_candidates


# ---- lexicon shortlists by edit distance ---------------------------------------------------------------------------------------------
# With opt.lexicon_shortlist = K a large shared lexicon (opt.lexicon on a CTC head, opt.attn_lexicon on the attention head) is decoded
# by the lexicon protocol of the CRNN paper (Shi et al., section 3.3): take the lexicon-free transcription, keep the K words nearest
# to it by edit distance, choose among those by the model's probability.  The first step is the greedy decode the forward already
# runs, the last the exact candidate scoring above (ctc_lexicon_host / attn_candidates_host and their kernels on a table cand [B][K]);
# the middle one is mrn_lexicon_shortlist_i32 (mrn_amd/csrc/lexicon_shortlist.hip), restated in numpy by lexicon_shortlist_host
# below.  For sample b with the hypothesis hyp[b][:n_b], n_b = hyp_len[b] clipped to 0 .. Hmax, and word w with the classes
# lex_tokens[w][:lex_len[w]]:
#
#   d(b, w) = the Levenshtein distance with unit costs over class tokens (mrn_amd/test.py edit_distance on the two token rows);
#   the words with max_dist None or d <= max_dist are ranked by (d, w) ascending: a tie goes to the lower word index;
#   the first K go to cand[b] (word indices) and dist[b] (their distances), in that order; unused slots are -1 in both, the value
#   ctc_lexicon_host(cand=) and CandidateHandle.with_cand take for an unused slot.
#
# Duplicate words are distinct indices and are all kept, as the encoders keep them.  Everything is integer arithmetic: the kernel's
# result is the host form's, element for element.  The kernel holds a hypothesis as one 64-bit word of Myers' bit-vector algorithm: a
# sample with more than 64 tokens is flagged and finished by the host form (ops.lexicon_shortlist merges the rows).  The shortlist only
# orders the candidates: with K >= N and no cut-off nothing is lost and the best word is the exact arg-max over the lexicon.  A sample
# whose shortlist is empty (every word beyond max_dist) has no live slot and gets the empty prediction with confidence 0.
SHORTLIST_MAX_K = 256
SHORTLIST_MAX_WORDS = 1 << 20
SHORTLIST_MAX_LENGTH = 255        # a distance is at most max(64, 255) and is kept as a byte between the two launches
SHORTLIST_MAX_HYPOTHESIS = 64
SHORTLIST_MAX_CLASS = 65534


def shortlist_options(opt):
    """(K or None, max_dist or None) of an options object: opt.lexicon_shortlist is absent / None (off) or an integer >= 1, the words
    kept per sample; opt.lexicon_max_distance is absent / None (no cut-off) or an integer >= 0"""
    K = getattr(opt, "lexicon_shortlist", None)
    if K is not None:
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError(f"lexicon_shortlist must be an integer >= 1 (or None), got {K!r}")
        K = int(K)
    max_dist = getattr(opt, "lexicon_max_distance", None)
    if max_dist is not None:
        if isinstance(max_dist, bool) or not isinstance(max_dist, (int, np.integer)) or max_dist < 0:
            raise ValueError(f"lexicon_max_distance must be an integer >= 0 (or None), got {max_dist!r}")
        max_dist = int(max_dist)
    return K, max_dist


def shortlist_request(opt, attn):
    """(K, max_dist) of validation() on an attention (attn) or CTC head, or None with the option off.  The shortlist is taken from the
    head's own lexicon option (attn_lexicon / lexicon; the other head's is ignored, as without a shortlist): without it the option is a
    ValueError, and so it is together with candidates, which names every sample's words itself"""
    K, max_dist = shortlist_options(opt)
    if K is None:
        return None
    if getattr(opt, "candidates", None) is not None:
        raise ValueError("lexicon_shortlist and candidates both choose the words a sample is scored against: set one of them")
    key = "attn_lexicon" if attn else "lexicon"
    if getattr(opt, key, None) is None:
        raise ValueError(f"lexicon_shortlist={K} shortlists the words of {key}, which is not set "
                         f"(a{'n attention' if attn else ' CTC'} head reads {key})")
    return K, max_dist


def shortlist_supported(Lmax, N, K, max_class):
    """does mrn_lexicon_shortlist_i32 take a table of N words of at most Lmax classes, the largest of them max_class, and K slots"""
    return (1 <= K <= SHORTLIST_MAX_K and 1 <= N <= SHORTLIST_MAX_WORDS and 1 <= Lmax <= SHORTLIST_MAX_LENGTH
            and 0 <= max_class <= SHORTLIST_MAX_CLASS)


def lexicon_shortlist_host(hyp, hyp_len, lex_tokens, lex_len, K, max_dist=None):
    """the K nearest words of every sample in numpy: hyp int [B][Hmax], hyp_len int [B] (clipped to 0 .. Hmax), the word table
    lex_tokens int [N][Lmax] / lex_len int [N] -> (cand int32 [B][K], dist int32 [B][K]), -1 in unused slots: the outputs of
    ops.lexicon_shortlist, for CPU tensors, for tables outside the kernel's limits and for the samples it flags.  Any hypothesis
    length, any K >= 1.  One Levenshtein row per hypothesis token over all words at once: the row's left-to-right minimum is a
    running minimum of (value - column)"""
    hyp, hyp_len = np.asarray(hyp).astype(np.int64), np.asarray(hyp_len).astype(np.int64)
    tokens, lengths = np.asarray(lex_tokens).astype(np.int64), np.asarray(lex_len).astype(np.int64)
    K = int(K)
    if hyp.ndim != 2 or hyp_len.shape != hyp.shape[:1] or K < 1:
        raise ValueError(f"lexicon_shortlist_host needs hyp [B][Hmax], hyp_len [B] and K >= 1, got {hyp.shape}, {hyp_len.shape}, {K}")
    if tokens.ndim != 2 or lengths.shape != tokens.shape[:1] or len(lengths) < 1:
        raise ValueError(f"lexicon_shortlist_host needs tokens [N >= 1][Lmax] and lengths [N], got {tokens.shape}, {lengths.shape}")
    if max_dist is not None and max_dist < 0:
        raise ValueError(f"lexicon_shortlist_host: max_dist={max_dist} must be >= 0 or None")
    B, Hmax = hyp.shape
    N, Lmax = tokens.shape
    if lengths.min() < 0 or lengths.max() > Lmax:
        raise ValueError(f"lexicon_shortlist_host: word lengths outside 0..{Lmax}")
    cols = np.arange(Lmax + 1)
    words = np.arange(N)
    cand = np.full((B, K), -1, dtype=np.int32)
    dist = np.full((B, K), -1, dtype=np.int32)
    for b in range(B):
        row = np.broadcast_to(cols, (N, Lmax + 1))                       # D[0][j] = j
        for i in range(int(min(max(hyp_len[b], 0), Hmax))):
            new = np.empty((N, Lmax + 1), dtype=np.int64)
            new[:, 0] = i + 1
            new[:, 1:] = np.minimum(row[:, 1:] + 1, row[:, :-1] + (tokens != hyp[b, i]))
            row = np.minimum.accumulate(new - cols, axis=1) + cols        # D[i][j] = min over k <= j of new[k] + (j - k)
        d = row[words, lengths]
        kept = words if max_dist is None else np.flatnonzero(d <= max_dist)
        order = kept[np.argsort(d[kept], kind="stable")][:K]
        cand[b, :len(order)] = order
        dist[b, :len(order)] = d[order]
    return cand, dist


def hypothesis_of_path(path, eos):
    """attention head: the greedy tokens path int [B][S] -> (hyp int32 [B][S], hyp_len int32 [B]): the tokens before the first eos
    (all S where there is none); numpy"""
    path = np.asarray(path)
    is_eos = path == eos
    n = np.where(is_eos.any(axis=1), is_eos.argmax(axis=1), path.shape[1])
    return path.astype(np.int32), n.astype(np.int32)


def hypothesis_of_frames(index):
    """CTC head: the per-frame arg-max index int [B][T] -> (hyp int32 [B][T], hyp_len int32 [B]): the best path collapsed (repeats of
    the raw index merged, blanks dropped), front-packed, 0 behind; numpy"""
    index = np.asarray(index)
    B, T = index.shape
    keep = index != 0
    keep[:, 1:] &= index[:, 1:] != index[:, :-1]
    hyp = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        row = index[b, keep[b]]
        hyp[b, :len(row)] = row
    return hyp, keep.sum(axis=1).astype(np.int32)


def attn_shortlist_request(attn_shortlist, prediction, is_train, attn_beam=None, attn_candidates=None):
    """the (handle, K, max_dist) an evaluation forward shortlists and scores its batch with, or None: attn_shortlist is set, the head is
    an attention head, the call is an evaluation under no_grad.  Together with a beam width or a candidate handle it is an error: all
    three replace greedy decoding"""
    import torch
    if attn_shortlist is None:
        return None
    if attn_beam is not None or attn_candidates is not None:
        raise ValueError("attn_shortlist replaces the greedy pair of an evaluation forward as attn_beam and attn_candidates do: pass one "
                         "of them")
    if not isinstance(attn_shortlist, tuple) or len(attn_shortlist) != 3:
        raise ValueError(f"attn_shortlist must be (handle of ops.upload_words, K, max_dist or None), got {attn_shortlist!r}")
    from types import SimpleNamespace
    K, max_dist = shortlist_options(SimpleNamespace(lexicon_shortlist=attn_shortlist[1], lexicon_max_distance=attn_shortlist[2]))
    if K is None:
        raise ValueError("attn_shortlist: K must be an integer >= 1")
    if "Attn" not in prediction or is_train or torch.is_grad_enabled():
        return None
    return attn_shortlist[0], K, max_dist


def attn_lm_options(opt, attn):
    """(lm or None, lm_weight, lm_bonus, top_n) of an options object: opt.attn_lm is absent / None (off) or a char_lm.CharLM over the
    attention head's classes, opt.lm_weight (default 0.5), opt.lm_bonus (default 0) and opt.beam_top_n (default 15) the keys opt.ctc_lm
    reads.  The model fuses into the attention head's beam search, so on an attention head attn_lm without attn_decode='beam', or
    together with attn_lexicon, candidates or lexicon_shortlist, is a ValueError; CTC heads ignore the option"""
    from .char_lm import CharLM
    lm = getattr(opt, "attn_lm", None)
    if lm is None or not attn:
        return None, DEFAULT_LM_WEIGHT, DEFAULT_LM_BONUS, DEFAULT_BEAM_TOP_N
    if not isinstance(lm, CharLM):
        raise ValueError(f"attn_lm must be a CharLM (modules/char_lm.py build_char_lm), got {type(lm).__name__}")
    if getattr(opt, "attn_decode", "greedy") != "beam":
        raise ValueError("attn_lm fuses into the attention head's beam search: set attn_decode='beam'")
    for key in ("attn_lexicon", "candidates", "lexicon_shortlist"):
        if getattr(opt, key, None) is not None:
            raise ValueError(f"attn_lm and {key}: a closed-vocabulary decoder has no use for a language model, set one of them")
    weights = check_lm_weights(getattr(opt, "lm_weight", DEFAULT_LM_WEIGHT), getattr(opt, "lm_bonus", DEFAULT_LM_BONUS))
    return (lm,) + weights + (_positive_int(opt, "beam_top_n", DEFAULT_BEAM_TOP_N),)


def attn_lm_request(attn_lm, attn_beam, attn_lexicon=None, attn_candidates=None, attn_shortlist=None):
    """the (handle, weight, bonus, top_n) an evaluation forward fuses into its beam search, or None: attn_lm is set.  It stands beside
    attn_beam: without a width, or together with a lexicon, candidate or shortlist search, it is an error"""
    if attn_lm is None:
        return None
    if attn_beam is None:
        raise ValueError("attn_lm fuses a language model into the beam search: pass attn_beam=<width> with it")
    if attn_lexicon is not None or attn_candidates is not None or attn_shortlist is not None:
        raise ValueError("attn_lm: a closed-vocabulary search (attn_lexicon, attn_candidates, attn_shortlist) has no use for a language model")
    if not isinstance(attn_lm, tuple) or len(attn_lm) != 4:
        raise ValueError(f"attn_lm must be (handle of ops.upload_char_lm, lm_weight, lm_bonus, top_n), got {attn_lm!r}")
    handle, weight, bonus, top_n = attn_lm
    if not hasattr(handle, "lm") or not hasattr(handle, "keys"):
        raise ValueError(f"attn_lm: the first member must be the handle of ops.upload_char_lm, got {type(handle).__name__}")
    attn_lm_proposals(1, top_n)
    return (handle,) + check_lm_weights(weight, bonus) + (int(top_n),)


# ---- one request record for the attention head's second decode -----------------------------------------------------------------------
# The evaluation forwards of Model, DERNet and MRNNet resolve their keywords (attn_beam, attn_lexicon, attn_candidates, attn_shortlist,
# attn_lm) once, with attn_search_request; everything below them takes the record.
ATTN_SEARCHES = ("beam", "lexicon", "candidates", "shortlist")
# where (path, prob, word) stand in the output tuple of a kind's search: Attention.beam_search / lexicon_search / score_candidates and
# the grouped ops of the same names; shortlist_search returns score_candidates' outputs in front of its table
_BEST_AT = {"beam": (4, 5, None), "lexicon": (4, 5, 6), **dict.fromkeys(("candidates", "shortlist"), (3, 4, 0))}


class AttnSearch(namedtuple("AttnSearch", "kind width trie cands words K max_dist", defaults=(None,) * 6)):
    """the second decode of an evaluation forward: kind is one of ATTN_SEARCHES; width and trie (an ops.TrieHandle; "lexicon" only) of a
    beam search, cands (an ops.CandidateHandle after with_cand) of "candidates", words (the handle of ops.upload_words), K and max_dist
    of "shortlist".  Members a kind does not use are None.  lm: None here; the language model of an AttnFusedSearch"""
    __slots__ = ()
    lm = None

    @property
    def has_word(self):          # does the search name a word of a table (the forward's beam_word)
        return self.kind != "beam"

    def scoring(self, cand, S):
        """a shortlist request and the table cand int32 [B,K] computed for it -> the "candidates" request that scores the table"""
        return AttnSearch("candidates", cands=self.words.with_cand(cand, S))


class AttnFusedSearch(AttnSearch):
    """the "beam" request of a beam search fused with a language model: lm = (ops.CharLMHandle, lm_weight, lm_bonus, top_n) beside
    the record's width.  Everything that takes an AttnSearch takes it; two requests are equal when record and model are.  A subclass
    and not an eighth member of the record: tests/test_attn_search_cpu.py pins AttnSearch to its seven members.  _replace keeps the
    model; _asdict and the hash are the record's (equal requests hash alike)"""

    def __new__(cls, width, lm):
        self = super().__new__(cls, "beam", width=width)
        self.lm = lm
        return self

    def _replace(self, **kw):
        lm = kw.pop("lm", self.lm)
        new = AttnSearch._replace(self, **kw)
        new.lm = lm
        return new

    def __eq__(self, other):
        return tuple.__eq__(self, other) and getattr(other, "lm", None) == self.lm

    def __ne__(self, other):
        return not self == other

    __hash__ = AttnSearch.__hash__


def attn_search_request(prediction, is_train, attn_beam=None, attn_lexicon=None, attn_candidates=None, attn_shortlist=None, attn_lm=None):
    """the keywords of an evaluation forward -> AttnSearch, or None where nothing is decoded a second time (no keyword set, a CTC
    head, training, grad enabled).  Every check is one of the *_request functions above, attn_lm's first, then the four in this order:
    attn_lexicon (or attn_lm) without attn_beam is an error whatever the head"""
    fusion = attn_lm_request(attn_lm, attn_beam, attn_lexicon, attn_candidates, attn_shortlist)
    width = attn_beam_request(attn_beam, prediction, is_train)
    trie = attn_lexicon_request(attn_lexicon, attn_beam)
    cands = attn_candidates_request(attn_candidates, prediction, is_train, attn_beam)
    short = attn_shortlist_request(attn_shortlist, prediction, is_train, attn_beam, attn_candidates)
    if short is not None:
        return AttnSearch("shortlist", words=short[0], K=short[1], max_dist=short[2])
    if cands is not None:
        return AttnSearch("candidates", cands=cands)
    if width is None:
        return None
    if fusion is not None:
        return AttnFusedSearch(width, fusion)
    return AttnSearch("beam" if trie is None else "lexicon", width=width, trie=trie)


def best_of(kind, res):
    """the output tuple of a kind's search -> (path, prob, word or None) of every sample's best entry, whatever the leading dimensions
    ([B, ...] of one head, [G, B, ...] of a heads group)"""
    path, prob, word = _BEST_AT[kind]
    return res[path], res[prob], None if word is None else res[word][..., 0]

