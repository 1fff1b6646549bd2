"""Prediction stage operator: attention decoder on the HIP path (reference modules/prediction.py:8-118).

Same constructor (`Attention(input_size, hidden_size, num_class, fc, num_char_embeddings=256)`), forward signature
and state_dict keys (attention_cell.{i2h,h2h,score,rnn}.*, generator.* aliasing fc, char_embeddings.weight).
Teacher-forced mode is one persistent kernel for all 26 steps with i2h(H) and the embedding half of the LSTMCell
input projection hoisted into GEMMs; greedy mode is one persistent kernel too (ops.attn_greedy_decode: generator and argmax inside
the step, the token fed back in LDS), with the step-by-step form kept behind MRN_GREEDY_DECODE=stepwise.
"""
import torch
import torch.nn as nn

from .. import ops
from ._nn import require_no_grad
from .hidden_size import check_hidden


def _host_result(res):
    """the arrays of a host form of modules/decoding.py as the tensors its kernel returns: float64 becomes float32"""
    return tuple(torch.from_numpy(r).to(torch.float32) if r.dtype == "float64" else torch.from_numpy(r) for r in res)


class AttentionCell(nn.Module):
    def __init__(self, input_size, hidden_size, num_embeddings):
        super().__init__()
        self.i2h = nn.Linear(input_size, hidden_size, bias=False)
        self.h2h = nn.Linear(hidden_size, hidden_size)
        self.score = nn.Linear(hidden_size, 1, bias=False)
        self.rnn = nn.LSTMCell(input_size + num_embeddings, hidden_size)
        self.hidden_size = hidden_size
        self.input_size = input_size


class Attention(nn.Module):
    def __init__(self, input_size, hidden_size, num_class, fc, num_char_embeddings=256):
        super().__init__()
        self.attention_cell = AttentionCell(input_size, hidden_size, num_char_embeddings)
        self.hidden_size = hidden_size
        self.num_class = num_class
        self.generator = fc
        self.num_char_embeddings = num_char_embeddings
        self.char_embeddings = nn.Embedding(num_class, num_char_embeddings)

    def cut_unknown(self, index):
        return torch.where(index >= self.num_class, 0, index)

    def _packed(self):
        """fragment-major copies of the three recurrent weight streams (rebuilt when a parameter changes)"""
        cell = self.attention_cell
        ps = (cell.h2h.weight, cell.rnn.weight_ih, cell.rnn.weight_hh)
        key = tuple((p.data_ptr(), p._version) for p in ps)
        cache = getattr(self, "_mrn_packed", None)
        if cache is None or cache[0] != key:
            with torch.no_grad():
                D = cell.input_size
                packed = (ops.pack_fragment_major(ps[0]), ops.pack_fragment_major(ps[1][:, :D]),
                          ops.pack_fragment_major(ps[2]))
            cache = (key, packed)
            self._mrn_packed = cache
        return cache[1]

    def _packed_x3(self):
        """the same three streams as fp16 hi / lo fragment-major splits + their inverse prescales (ops.pack_decoder_x3), cached"""
        cell = self.attention_cell
        ps = (cell.h2h.weight, cell.rnn.weight_ih, cell.rnn.weight_hh)
        key = tuple((p.data_ptr(), p._version) for p in ps)
        cache = getattr(self, "_mrn_packed_x3", None)
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key, ops.pack_decoder_x3(ps[0], ps[1], ps[2], cell.input_size))
            self._mrn_packed_x3 = cache
        return cache[1]

    def x3_ok(self):
        return ops.DECODER_X3 and self.attention_cell.input_size % 32 == 0 and self.hidden_size == 256

    def _greedy_operands(self):
        """what the fused greedy decoder reads besides the recurrent streams, cached per parameter version:
        (etab [C,4H] = char_embeddings.weight . W_ih[:, D:]^T + b_ih, generator stream (ops.pack_generator), w_inv float[4] or None)"""
        cell = self.attention_cell
        x3 = self.x3_ok()
        ps = (self.char_embeddings.weight, cell.rnn.weight_ih, cell.rnn.bias_ih, self.generator.weight, cell.h2h.weight, cell.rnn.weight_hh)
        key = tuple((p.data_ptr(), p._version) for p in ps) + (x3,)
        cache = getattr(self, "_mrn_greedy", None)
        if cache is None or cache[0] != key:
            with torch.no_grad():
                etab = ops.linear(self.char_embeddings.weight, cell.rnn.weight_ih[:, cell.input_size:], cell.rnn.bias_ih)
                w_gen, g_inv = ops.pack_generator(self.generator.weight, x3)
                w_inv = torch.cat([self._packed_x3()[3], g_inv]).contiguous() if x3 else None
            cache = (key, (etab, w_gen, w_inv))
            self._mrn_greedy = cache
        return cache[1]

    def greedy_args(self):
        """(etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, w_inv) of ops.attn_greedy_decode[_grouped]"""
        cell = self.attention_cell
        etab, w_gen, w_inv = self._greedy_operands()
        w_h2h, w_ih_ctx, w_hh = self._packed_x3()[:3] if w_inv is not None else self._packed()
        return (etab, w_h2h, cell.h2h.bias, cell.score.weight, w_ih_ctx, w_hh, cell.rnn.bias_hh, w_gen, self.generator.bias, w_inv)

    def _decode(self, batch_H, Hproj, eproj, hid=None, h=None, c=None):
        cell = self.attention_cell
        if self.x3_ok():
            w_h2h, w_ih_ctx, w_hh, w_inv = self._packed_x3()
        else:
            (w_h2h, w_ih_ctx, w_hh), w_inv = self._packed(), None
        return ops.attn_decoder(batch_H, Hproj, eproj, w_h2h, cell.h2h.bias, cell.score.weight,
                                w_ih_ctx, w_hh, cell.rnn.bias_hh, self.hidden_size, hid=hid, h_state=h, c_state=c, w_inv=w_inv)

    def _fused(self, S, eos):
        """what beam_fused, lexicon_fused and score_fused share: MRN_ATTN_BEAM (read per call), the kernels' hidden size, steps, classes"""
        return (ops.attn_beam_mode() == "fused" and self.hidden_size == 256 and 1 <= S <= 512 and self.num_class >= 2
                and 0 <= eos < self.num_class)

    def _search_operands(self, who, batch_H, sos, eos, batch_max_length, width=None, Hproj=None):
        """what every search starts with -> (start, batch_H, Hproj, S, eos): the hidden size and the end token (and, where the search
        has one, the width) checked, start = the start token as a one-element int64 tensor, batch_H contiguous, Hproj = i2h(batch_H)
        unless the caller has it (None for CPU tensors: the host forms make their own)"""
        check_hidden(None, "Attn", self.hidden_size)
        S, eos = int(batch_max_length) + 1, int(eos)
        if (width is not None and int(width) < 1) or not 0 <= eos < self.num_class:
            needs, got = ("width >= 1 and ", f"{width}, ") if width is not None else ("", "")
            raise ValueError(f"{who} needs {needs}0 <= eos < {self.num_class}, got {got}{eos}")
        start = sos.reshape(-1)[:1].contiguous() if torch.is_tensor(sos) else torch.tensor([int(sos)], dtype=torch.int64, device=batch_H.device)
        batch_H = batch_H.contiguous()
        if Hproj is None and batch_H.is_cuda:
            Hproj = ops.linear(batch_H, self.attention_cell.i2h.weight)
        return start, batch_H, Hproj, S, eos

    @torch.no_grad()
    def search(self, req, batch_H, sos, batch_max_length, tokens=None, Hproj=None):
        """the second decode a decoding.AttnSearch asks for, ending on ATTN_EOS -> (path int64 [B,S], prob [B,S], word int32 [B] or None)
        of every sample's best entry: the one place that maps a request to the four searches below.  tokens: shortlist_search's; Hproj:
        score_candidates'"""
        from .decoding import ATTN_EOS, best_of
        if req.kind == "beam":
            lm, weight, bonus, top_n = req.lm or (None, 0.0, 0.0, 15)
            res = self.beam_search(batch_H, sos, ATTN_EOS, req.width, batch_max_length, lm=lm, lm_weight=weight, lm_bonus=bonus, top_n=top_n)
        elif req.kind == "lexicon":
            res = self.lexicon_search(batch_H, sos, ATTN_EOS, req.width, req.trie, batch_max_length)
        elif req.kind == "candidates":
            res = self.score_candidates(batch_H, sos, ATTN_EOS, req.cands, batch_max_length, Hproj=Hproj)
        else:
            res = self.shortlist_search(batch_H, sos, ATTN_EOS, req.words, req.K, req.max_dist, batch_max_length, tokens=tokens)
        return best_of(req.kind, res)

    def beam_fused(self, D, T, S, eos, width):
        """does beam_search take the fused launch (mrn_attn_beam_decode_*): its limits, the LDS budget and MRN_ATTN_BEAM (read per call)"""
        return self._fused(S, eos) and ops.attn_beam_whole_context(D, T, width, self.x3_ok())

    def beam_lm_fused(self, D, T, S, eos, width, lm, top_n):
        """does beam_search(lm=) take the fused launch (mrn_attn_beam_lm_decode_*): beam_fused's limits with that launch's LDS sum, classes
        that fit a 16-bit context, top_n >= 1 (the launch is given min(top_n, 16): N = min(16, max(W, top_n)) is the same search) and a
        model the kernel takes"""
        from .decoding import beam_lm_supported
        return (self._fused(S, eos) and self.num_class <= 65535 and top_n >= 1 and beam_lm_supported(lm.lm)
                and ops.attn_beam_lm_whole_context(D, T, width, self.x3_ok()))

    @torch.no_grad()
    def beam_search(self, batch_H, sos, eos, width, batch_max_length=25, lm=None, lm_weight=0.0, lm_bonus=0.0, top_n=15):
        """beam search of width `width` (modules/decoding.py states the algorithm): batch_H [B,T,D], sos an int or a device int64
        tensor whose first element is the start token -> (tokens int32 [B,W,S], length int32 [B,W], score [B,W], logp [B,W,S],
        path int64 [B,S], prob [B,S]), entries in descending score.  One launch where the kernel's limits and the LDS budget allow,
        otherwise (or under MRN_ATTN_BEAM=stepwise) the step loop of forward() on the B * W-row batch.  Inference only (no_grad).
        lm (the handle of ops.upload_char_lm; lm_weight >= 0, lm_bonus, top_n >= 1): the search fused with that character n-gram model
        -> the six outputs with the entries in descending fused key and fused [B,W], that key; score and logp stay acoustic.  One
        launch where beam_lm_fused says so; CPU tensors, calls beyond the launch's limits and MRN_ATTN_BEAM=stepwise take
        decoding.attn_beam_host(lm=) in float64: there is no device step loop with a model"""
        B, T, D = batch_H.shape
        start, batch_H, Hproj, S, eos = self._search_operands("beam_search", batch_H, sos, eos, batch_max_length, width)
        W = int(width)
        if lm is not None:
            from .decoding import attn_beam_host, attn_lm_proposals, check_lm_weights
            if not isinstance(lm, ops.CharLMHandle):
                raise ValueError(f"beam_search needs the handle of ops.upload_char_lm, got {type(lm).__name__}")
            lm_weight, lm_bonus = check_lm_weights(lm_weight, lm_bonus)
            attn_lm_proposals(W, top_n)
            if batch_H.is_cuda and self.beam_lm_fused(D, T, S, eos, W, lm, int(top_n)):
                etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, w_inv = self.greedy_args()
                return ops.attn_beam_lm_decode(batch_H, Hproj, etab, start, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen,
                                               self.hidden_size, S, eos, W, lm, lm_weight, lm_bonus, min(int(top_n), 16), w_inv=w_inv)
            res = _host_result(attn_beam_host(self.state_dict(), batch_H, int(start[0]), eos, W, S - 1, lm=lm.lm, lm_weight=lm_weight,
                                              lm_bonus=lm_bonus, top_n=int(top_n)))
            return tuple(r.to(batch_H.device) for r in res)
        if self.beam_fused(D, T, S, eos, W):
            etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, w_inv = self.greedy_args()
            return ops.attn_beam_decode(batch_H, Hproj, etab, start, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen,
                                        self.hidden_size, S, eos, W, w_inv=w_inv)
        return self._search_stepwise(batch_H, Hproj, start, eos, W, S, None)

    def lexicon_fused(self, D, T, S, eos, width, trie):
        """does lexicon_search take the fused launch (mrn_attn_lexicon_decode_*): beam_fused's limits with the lexicon launch's LDS sum"""
        return self._fused(S, eos) and trie.depth <= S - 1 and ops.attn_lexicon_whole_context(D, T, width, self.x3_ok())

    @torch.no_grad()
    def lexicon_search(self, batch_H, sos, eos, width, trie_handle, batch_max_length=25):
        """beam search of width `width` walked along the trie of a lexicon (modules/decoding.py states the algorithm): the operands of
        beam_search and the handle of ops.upload_trie -> beam_search's six outputs and word int32 [B,W] (the lexicon index of the
        entry's word, -1 for a dead slot).  One launch where the kernel's limits and the LDS budget allow, otherwise (or under
        MRN_ATTN_BEAM=stepwise) beam_search's step loop with the same constraint; CPU tensors go to decoding.attn_lexicon_host"""
        from .decoding import attn_lexicon_host
        if not isinstance(trie_handle, ops.TrieHandle):
            raise ValueError(f"lexicon_search needs the handle of ops.upload_trie, got {type(trie_handle).__name__}")
        if trie_handle.depth > int(batch_max_length):
            raise ValueError(f"lexicon_search: the longest word has {trie_handle.depth} classes, more than batch_max_length={int(batch_max_length)}")
        B, T, D = batch_H.shape
        start, batch_H, Hproj, S, eos = self._search_operands("lexicon_search", batch_H, sos, eos, batch_max_length, width)
        W = int(width)
        if not batch_H.is_cuda:
            return _host_result(attn_lexicon_host(self.state_dict(), batch_H, int(start[0]), eos, W, S - 1, trie_handle.trie))
        if self.lexicon_fused(D, T, S, eos, W, trie_handle):
            etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, w_inv = self.greedy_args()
            return ops.attn_lexicon_decode(batch_H, Hproj, etab, start, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen,
                                           self.hidden_size, S, eos, W, trie_handle, w_inv=w_inv)
        return self._search_stepwise(batch_H, Hproj, start, eos, W, S, trie_handle)

    def score_fused(self, D, T, S, eos, n):
        """does score_candidates take the fused launch (mrn_attn_score_candidates_*): its limits, the LDS budget and MRN_ATTN_BEAM (read
        per call: "stepwise" forces the step form of every search and scorer on the attention head)"""
        return self._fused(S, eos) and self.num_class <= 65535 and 1 <= n <= 16 and ops.attn_score_whole_context(D, T, self.x3_ok())

    SCORE_ROWS_BYTES = 256 << 20      # the stepwise scorer's (sample, slot) rows go in chunks whose features and logits stay within this

    @torch.no_grad()
    def score_candidates(self, batch_H, sos, eos, handle, batch_max_length=25, want_logp=False, Hproj=None):
        """exact log p(word, eos | sample) of every sample's candidate words (modules/decoding.py states the algorithm): batch_H
        [B,T,D], sos as in beam_search, handle = ops.upload_words(...).with_cand(cand [B,K], S) -> (index int32 [B,n], score [B,n],
        score_all [B,K], path int64 [B,S], prob [B,S]) and, with want_logp, logp [B,K,S].  One launch where the kernel's limits and
        the LDS budget allow, otherwise (or under MRN_ATTN_BEAM=stepwise) the teacher-forced decoder on the (sample, slot) rows;
        CPU tensors go to decoding.attn_candidates_host.  Hproj: i2h(batch_H) where the caller has it already.  Inference only
        (no_grad)"""
        from .decoding import attn_candidates_host
        if not isinstance(handle, ops.CandidateHandle) or handle.cand is None:
            raise ValueError(f"score_candidates needs the handle of ops.upload_words(...).with_cand(...), got {type(handle).__name__}")
        B, T, D = batch_H.shape
        if handle.cand.shape[0] != B:
            raise ValueError(f"score_candidates: {handle.cand.shape[0]} candidate rows for {B} samples")
        start, batch_H, Hproj, S, eos = self._search_operands("score_candidates", batch_H, sos, eos, batch_max_length, Hproj=Hproj)
        if not batch_H.is_cuda:
            return _host_result(attn_candidates_host(self.state_dict(), batch_H, int(start[0]), eos, handle.tokens, handle.lengths, handle.cand,
                                                     handle.n, S - 1, want_logp=want_logp))
        tokens, lengths, cand = handle.tokens_dev, handle.lengths_dev, handle.cand_dev
        if self.score_fused(D, T, S, eos, handle.n):
            etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, w_inv = self.greedy_args()
            return ops.attn_score_candidates(batch_H, Hproj, etab, start, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen,
                                             self.hidden_size, S, eos, tokens, lengths, cand, n=handle.n, want_logp=want_logp,
                                             w_inv=w_inv, check=False)
        score_all, logp = self._score_stepwise(batch_H, Hproj, start, eos, tokens, lengths, cand, S)
        index, score, path, prob = (r[0] for r in ops.rank_candidates(score_all.unsqueeze(0), logp.unsqueeze(0), tokens, lengths, cand,
                                                                      handle.n, eos))
        out = (index, score, score_all, path, prob)
        return out + (logp,) if want_logp else out

    @torch.no_grad()
    def shortlist_search(self, batch_H, sos, eos, handle, K, max_dist=None, batch_max_length=25, want_logp=False, tokens=None):
        """the lexicon protocol on a shared word table (modules/decoding.py, "lexicon shortlists"): the greedy decode, the hypothesis =
        its tokens before the first eos, the K words nearest to it by edit distance (ops.lexicon_shortlist), and the exact scores of
        those (score_candidates): batch_H [B,T,D], sos as in beam_search, handle = ops.upload_words(...) -> score_candidates' outputs
        (index int32 [B,n], score [B,n], score_all [B,K], path int64 [B,S], prob [B,S], and logp [B,K,S] with want_logp), then cand
        int32 [B,K] and dist int32 [B,K].  No beam is run and no width is read.  The greedy decode is the fused launch
        (mrn_attn_greedy_decode*), the forward's own step loop under MRN_GREEDY_DECODE=stepwise; CPU tensors take the host forms
        (decoding.attn_beam_host at width 1 is greedy decoding).  tokens int64 [B,S]: the greedy tokens where the caller has decoded
        already (the arg-max of the forward's logits): no greedy launch then.  Inference only (no_grad)"""
        from . import decoding as D
        if not isinstance(handle, ops.CandidateHandle):
            raise ValueError(f"shortlist_search needs the handle of ops.upload_words, got {type(handle).__name__}")
        start, batch_H, Hproj, S, eos = self._search_operands("shortlist_search", batch_H, sos, eos, batch_max_length)
        if not batch_H.is_cuda:
            path = D.attn_beam_host(self.state_dict(), batch_H, int(start[0]), eos, 1, S - 1)[4] if tokens is None else tokens.numpy()
            hyp, hyp_len = D.hypothesis_of_path(path, eos)
            cand, dist = D.lexicon_shortlist_host(hyp, hyp_len, handle.tokens, handle.lengths, K, max_dist)
            res = self.score_candidates(batch_H, sos, eos, handle.with_cand(cand, S), S - 1, want_logp=want_logp)
            return res + (torch.from_numpy(cand), torch.from_numpy(dist))
        if tokens is None and ops.greedy_decode_mode() == "fused":
            etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, w_inv = self.greedy_args()
            tokens = ops.attn_greedy_decode(batch_H, Hproj, etab, start, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen,
                                            self.hidden_size, S, want_tokens=True, w_inv=w_inv)[1]
        elif tokens is None:
            tokens = ops.argmax_lastdim(self.forward(batch_H, start, is_train=False, batch_max_length=S - 1))
        cand, dist = ops.lexicon_shortlist(*ops.hypothesis_of_path(tokens, eos), handle, K, max_dist)
        res = self.score_candidates(batch_H, start, eos, handle.with_cand(cand, S), S - 1, want_logp=want_logp, Hproj=Hproj)
        return res + (cand, dist)

    def _score_stepwise(self, batch_H, Hproj, start, eos, tokens, lengths, cand, S):
        """score_candidates outside the fused launch: the teacher-forced decoder and the generator on chunks of the B * K (sample,
        slot) rows, log-softmax and gather in torch -> (score_all [B,K], logp [B,K,S])"""
        cell = self.attention_cell
        B, T, D = batch_H.shape
        K, C, dev = cand.shape[1], self.num_class, batch_H.device
        neg = torch.tensor(float("-inf"), device=dev)
        Lmax = tokens.shape[1]
        used = torch.arange(Lmax, device=dev).unsqueeze(0) < lengths.unsqueeze(1)
        spelled = ((tokens < C) | ~used).all(dim=1)
        word = cand.long().clamp(min=0)
        live = (cand >= 0) & spelled[word]
        L = torch.where(live, lengths.long()[word], -1)                                  # [B,K]
        cols = min(Lmax, S)
        target = torch.full((B, K, S), eos, dtype=torch.int64, device=dev)              # the word's classes, then eos
        target[:, :, :cols] = torch.where(torch.arange(cols, device=dev) < L.unsqueeze(2), tokens.long()[word][:, :, :cols], eos)
        fed = torch.cat([start.expand(B * K, 1), target.view(B * K, S)[:, :S - 1]], dim=1)
        w_emb = cell.rnn.weight_ih[:, D:]
        logp = torch.empty(B * K, S, device=dev)
        chunk = max(1, self.SCORE_ROWS_BYTES // (4 * (T * (D + self.hidden_size) + S * (C + 5 * self.hidden_size))))
        for r0 in range(0, B * K, chunk):
            r1 = min(B * K, r0 + chunk)
            b = torch.arange(r0, r1, device=dev) // K
            emb = ops.embed_gather(fed[r0:r1].contiguous(), self.char_embeddings.weight, C)
            eproj = ops.linear(emb, w_emb, cell.rnn.bias_ih)
            hid = self._decode(batch_H[b], Hproj[b], eproj)
            x = ops.linear(hid, self.generator.weight, self.generator.bias)
            lp = torch.log_softmax(torch.where(torch.isnan(x), neg, x), dim=2)
            logp[r0:r1] = lp.gather(2, target.view(B * K, S)[r0:r1].unsqueeze(2)).squeeze(2)
        logp = torch.where(torch.arange(S, device=dev) <= L.unsqueeze(2), logp.view(B, K, S), torch.zeros((), device=dev))
        score_all = logp.sum(dim=2)
        dead = ~live | torch.isnan(score_all) | (score_all == float("-inf"))
        return torch.where(dead, neg, score_all), torch.where(dead.unsqueeze(2), torch.zeros((), device=dev), logp)

    @staticmethod
    def _admitted(trie, node, C, eos):
        """node int64 [B * W] -> (admitted bool [B * W, C], step_to int64 [B * W, C]): the classes the rows' nodes admit and the node
        each leads to, a ragged expand of the trie's CSR rows; eos is admitted where a word ends and leads nowhere"""
        dev = node.device
        lo = trie.child_off[node].to(torch.int64)
        count = trie.child_off[node + 1].to(torch.int64) - lo
        row = torch.repeat_interleave(torch.arange(node.numel(), device=dev), count)
        edge = torch.arange(row.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(count, 0) - count, count) + torch.repeat_interleave(lo, count)
        cls = trie.child_tok[edge].to(torch.int64)
        ok = cls < C
        row, cls, edge = row[ok], cls[ok], edge[ok]
        admitted = torch.zeros(node.numel(), C, dtype=torch.bool, device=dev)
        step_to = node.view(-1, 1).repeat(1, C)
        admitted[row, cls] = True
        step_to[row, cls] = trie.child_node[edge].to(torch.int64)
        admitted[:, eos] |= trie.word_of[node] >= 0
        return admitted, step_to

    def _search_stepwise(self, batch_H, Hproj, start, eos, W, S, trie):
        """the step loop of beam_search (trie None) and lexicon_search (a TrieHandle: only the classes an entry's node admits are
        candidates, a node is carried per row, and word is one more output): gather, Linear, one decoder step with carried state and the
        generator on B * W rows; the selection on the sorted candidates"""
        cell = self.attention_cell
        B, T, D = batch_H.shape
        dev = batch_H.device
        C, H = self.num_class, self.hidden_size
        w_emb = cell.rnn.weight_ih[:, D:]
        Hb_rows = batch_H.repeat_interleave(W, dim=0)
        Hproj_rows = Hproj.repeat_interleave(W, dim=0)
        h = torch.zeros(B * W, H, device=dev)
        c = torch.zeros(B * W, H, device=dev)
        hid = torch.empty(B * W, 1, H, device=dev)
        targets = start.expand(B * W).contiguous().view(B * W, 1)
        neg = torch.tensor(float("-inf"), device=dev)
        score = torch.full((B, W), float("-inf"), device=dev)
        score[:, 0] = 0.0
        finished = torch.zeros(B, W, dtype=torch.bool, device=dev)
        tokens = torch.full((B, W, S), eos, dtype=torch.int32, device=dev)
        logp = torch.zeros(B, W, S, device=dev)
        rows = torch.arange(B, device=dev).view(B, 1)
        node = torch.zeros(B, W, dtype=torch.int64, device=dev)
        for s in range(S):
            emb = ops.embed_gather(targets, self.char_embeddings.weight, C)
            eproj = ops.linear(emb, w_emb, cell.rnn.bias_ih)
            self._decode(Hb_rows, Hproj_rows, eproj, hid=hid, h=h, c=c)
            x = ops.linear(hid, self.generator.weight, self.generator.bias).view(B, W, C)
            lp = torch.log_softmax(torch.where(torch.isnan(x), neg, x), dim=2)
            done = torch.full((B, W, C), float("-inf"), device=dev)
            done[:, :, eos] = score
            cand = score.unsqueeze(2) + lp
            if trie is not None:
                admitted, step_to = self._admitted(trie, node.view(-1), C, eos)
                cand = torch.where(admitted.view(B, W, C), cand, neg)
            cand = torch.where(finished.unsqueeze(2), done, cand)
            cand = torch.where(torch.isnan(cand), neg, cand).view(B, W * C)               # candidate order (i, c)
            val, idx = torch.sort(cand, dim=1, descending=True, stable=True)
            val, idx = val[:, :W], idx[:, :W]
            if val.shape[1] < W:               # (W * C < W cannot happen: C >= 1)
                raise RuntimeError("beam_search: fewer candidates than entries")
            par, cls = idx // C, idx % C
            alive = val > float("-inf")
            was_done = finished[rows, par]
            tokens, logp = tokens[rows, par], logp[rows, par]
            tokens[:, :, s] = torch.where(alive, cls, eos).to(torch.int32)
            logp[:, :, s] = torch.where(alive & ~was_done, lp[rows, par, cls], 0.0)
            tokens[~alive] = eos
            logp[~alive] = 0.0
            h = h.view(B, W, H)[rows, par].reshape(B * W, H).contiguous()
            c = c.view(B, W, H)[rows, par].reshape(B * W, H).contiguous()
            targets = torch.where(alive, cls, eos).reshape(B * W, 1).contiguous()
            if trie is not None:                   # a finished or dead entry keeps its node
                node = torch.where(alive & ~was_done, step_to.view(B, W, C)[rows, par, cls], node[rows, par])
            finished = alive & (cls == eos)
            score = val
        alive = score > float("-inf")
        is_eos = tokens == eos
        length = torch.where(is_eos.any(dim=2), is_eos.to(torch.int32).argmax(dim=2) + 1, S).to(torch.int32)
        length[~alive] = -1
        out = (tokens, length, score, logp, tokens[:, 0].to(torch.int64), torch.exp(logp[:, 0]))
        if trie is not None:
            out += (torch.where(alive, trie.word_of[node], -1).to(torch.int32),)
        return out

    def forward(self, batch_H, text, is_train=True, batch_max_length=25, out=None):
        """batch_H [B,T,D]; text [B,S] (teacher forcing) or [B] of [SOS] (greedy) -> logits [B,S,num_class].
        `out` may be a preallocated (possibly strided) [B,S,num_class] buffer."""
        from ..functional import AttnDecoderFn, needs_grad
        check_hidden(None, "Attn", self.hidden_size)          # the decoder kernels are built for 256 only: refuse before any launch
        cell = self.attention_cell
        B = batch_H.shape[0]
        S = batch_max_length + 1
        if needs_grad(self, batch_H):
            if not is_train:
                raise NotImplementedError("greedy decoding is inference only; call it under torch.no_grad()")
            probs = AttnDecoderFn.apply(batch_H, text, cell.i2h.weight, cell.h2h.weight, cell.h2h.bias, cell.score.weight,
                                        cell.rnn.weight_ih, cell.rnn.weight_hh, cell.rnn.bias_ih, cell.rnn.bias_hh,
                                        self.char_embeddings.weight, self.generator.weight, self.generator.bias, S)
            if out is not None:
                out.copy_(probs)
                return out
            return probs
        D = cell.input_size
        batch_H = batch_H.contiguous()
        Hproj = ops.linear(batch_H, cell.i2h.weight)
        w_emb = cell.rnn.weight_ih[:, D:]                      # [4H, E] strided view
        if is_train:
            emb = ops.embed_gather(text[:, :S], self.char_embeddings.weight, self.num_class)
            eproj = ops.linear(emb, w_emb, cell.rnn.bias_ih)
            hid = self._decode(batch_H, Hproj, eproj)
            return ops.linear(hid, self.generator.weight, self.generator.bias, out=out)
        # greedy decode (reference :70-86): token_{s+1} = argmax(generator(h_s))
        dev = batch_H.device
        if ops.greedy_decode_mode() == "fused":
            # all S steps in one launch; faster than the step loop at every measured shape ("Greedy decoding")
            etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, w_inv = self.greedy_args()
            return ops.attn_greedy_decode(batch_H, Hproj, etab, text, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen,
                                          self.hidden_size, S, out=out, w_inv=w_inv)
        # MRN_GREEDY_DECODE=stepwise: five launches per step (gather, Linear, one decoder step with carried state, generator, argmax)
        targets = text[0].expand(B).contiguous().view(B, 1)
        probs = out if out is not None else torch.empty(B, S, self.num_class, device=dev, dtype=torch.float32)
        h = torch.zeros(B, self.hidden_size, device=dev)
        c = torch.zeros(B, self.hidden_size, device=dev)
        hid = torch.empty(B, 1, self.hidden_size, device=dev)
        for s in range(S):
            emb = ops.embed_gather(targets, self.char_embeddings.weight, self.num_class)
            eproj = ops.linear(emb, w_emb, cell.rnn.bias_ih)
            self._decode(batch_H, Hproj, eproj, hid=hid, h=h, c=c)
            step = probs[:, s:s + 1, :]
            ops.linear(hid, self.generator.weight, self.generator.bias, out=step)
            targets = ops.argmax_lastdim(step).view(B, 1)
        return probs
