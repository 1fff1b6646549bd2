"""validation(): greedy-decode evaluation with the reference's return convention and scoring rules (reference
test.py:139-279).  Accuracy = exact match against the RAW label string (a predicted [UNK] never counts as correct,
test.py:232-236), norm_ED = ICDAR-2019 normalised edit distance, confidence = product of the per-step max-probabilities.
(the forward / decoding path runs on the HIP kernels.)  Scoring runs on the device too: one
mrn_greedy_score_f32 launch per batch (CTC collapse / [EOS] cut, edit distance, exact match, confidence) on integer tokens, with
the same eight return values, bit for bit, as the reference's per-sample string loop.  That loop is kept as the host path: for a
batch outside the kernel's limits (modules/scoring.py), for predictions that are not on the GPU, for the samples the kernel flags
(a predicted [UNK] / [PAD] / [SOS] where it counts), and for everything under MRN_VALIDATION_SCORING=host.

Reference quirks reproduced on purpose (pinned by tests/golden/validation.npz):
  * attention head: the prediction is cut at prd.find("[EOS]"); when there is NO [EOS] find() returns -1, so the LAST
    character (and the last probability) is dropped (test.py:224-226);
  * the returned strings / confidences / labels are those of the LAST batch only (test.py:270-279);
  * an empty pruned prediction has confidence 0 (the reference's bare `except`, test.py:262-265).

opt.ctc_decode = "beam" (modules/decoding.py; absent or "greedy": best path, as above and bit for bit) decodes a CTC head by prefix
beam search of width opt.beam_width over the opt.beam_top_n best classes of a frame: one mrn_ctc_beam_decode_f32 launch per batch,
or the float64 host form for predictions that are not on the GPU and for batches outside the kernel's limits.  The decoder hands
over the best label as a row of frames whose greedy collapse is that label, and its probability as that row's first factor, so
everything behind the decoding line -- scoring on either path, the returned strings -- is the code above, unchanged; the confidence
is then the label's (pruned) probability instead of the product of the per-frame maxima.  The attention head has no alignments to
sum over: it ignores the option.

opt.ctc_lm = a CharLM (modules/char_lm.py build_char_lm; absent or None: as above, bit for bit) fuses a character n-gram model into
that beam search: candidates are ranked by log p_ctc + opt.lm_weight * log p_lm + opt.lm_bonus * length (defaults 0.5 and 0;
modules/decoding.py), one mrn_ctc_beam_lm_decode_f32 launch per batch with the model checked and uploaded once per call, or the
float64 host form where the beam decoder takes it.  The best entry by the fused key goes to the unchanged scorer, and its confidence is
still its acoustic probability.  The options are read only with ctc_decode = "beam" on a CTC head: ctc_lm without it, or together with
lexicon or candidates, is an error; the attention head ignores the option.

opt.attn_decode = "beam" (absent or "greedy": as above, bit for bit; CTC heads ignore it) decodes an attention head by beam search of
width opt.beam_width: the evaluation forward is asked for the beam pair (attn_beam=width: one more launch per heads group on the
same features, modules/decoding.py) and preds_index / preds_max_prob are the best entry's tokens and their probabilities instead of
the per-step arg-max and its probability.  The loss is still computed on the greedy decoder's logits, and the scorer, the "no [EOS]
drops the last character" quirk and the returned strings are the code above, unchanged: the confidence is then the probability of
the kept tokens of the best entry.

opt.attn_lm = a CharLM over the attention head's classes (build_char_lm on the AttnLabelConverter; absent or None: as above, bit for
bit; CTC heads ignore it, as the attention head ignores ctc_lm) fuses a character n-gram model into that beam search: an entry proposes
its min(16, max(beam_width, opt.beam_top_n)) best classes and the proposals are ranked by log p + opt.lm_weight * log p_lm +
opt.lm_bonus * length (the keys ctc_lm reads; modules/decoding.py), one mrn_attn_beam_lm_decode_* launch per heads group with the model
checked and uploaded once per call (attn_lm=(handle, weight, bonus, top_n) beside attn_beam on the evaluation forward), or the
float64 host form where the launch does not take the batch.  The best entry by the fused key goes to the unchanged scorer, and its
confidence is still the probability of its kept tokens.  The option is read only with attn_decode = "beam" on an attention head:
attn_lm without it, or together with attn_lexicon, candidates or lexicon_shortlist, is an error.

opt.lexicon = a sequence of words (absent or None: as above, bit for bit; the attention head ignores it: opt.attn_lexicon below is its
counterpart there) decodes a CTC head to the
lexicon word of largest log p(word | image), the exact CTC forward score of every (sample, word) pair (modules/decoding.py): the words
the converter can spell are encoded and uploaded once per call, then one mrn_ctc_lexicon_decode_f32 call per batch, or the float64
host form for predictions that are not on the GPU and for lexicons or batches outside the kernel's limits (a word of more than 31
characters).  The hand-over is the beam decoder's: the best word as a row of frames whose greedy collapse is that word, its probability
as that row's first factor, and the scorer behind it unchanged.  opt.lexicon_top_n (default 1) is the number of entries the decoder
ranks per sample; validation() scores the best one.  A lexicon together with ctc_decode = "beam" is an error: both replace best path.

opt.attn_lexicon = a sequence of words (absent or None: as above, bit for bit; CTC heads ignore it) is opt.lexicon's counterpart on the
attention head: the beam search of width opt.beam_width (whatever attn_decode says) is walked along a trie of the lexicon, so every
entry is a lexicon word and its score log p(word, [EOS] | image) of the model, not renormalised (modules/decoding.py; with a width of
at least the number of distinct words the best entry is the exact arg-max over the lexicon).  The words the converter can spell within
batch_max_length characters are encoded, the trie built, checked and uploaded once per call; the evaluation forward is asked for the
constrained beam pair (attn_beam=width, attn_lexicon=handle: one more launch per heads group, one trie for all experts) and the pair
goes to the unchanged scorer as in beam mode: the confidence is the product of the kept tokens' probabilities, the loss is still the
greedy logits'.  A sample none of whose words the routed expert can spell scores as an empty prediction with confidence 0.

opt.candidates (absent or None: as above, bit for bit) gives every image a word list of its own, the protocol of IIIT5K-50, SVT-50 and
IC03-50: a callable that takes the batch's list of label strings and returns one sequence of words per sample, or a dict label ->
words (a label without an entry is an error).  Nothing relies on the order of the loader.  The word table is the union of the lists,
encoded once per call by the head's lexicon encoder (words the converter cannot spell are dropped; for a callable the loader's labels
are read once more before the first batch), the candidate table cand [B, K] is built per batch.  A CTC head takes
ops.ctc_lexicon_decode(cand=) or its host form; an attention head scores every (sample, word) pair exactly (attn_candidates=handle on
the evaluation forward: one more launch per heads group, modules/decoding.py), so the best word is the arg-max of log p(word, [EOS] |
image) over the list whatever a beam width would have been.  opt.lexicon_top_n entries are ranked, the best one is scored, by the
unchanged scorer.  Together with lexicon, attn_lexicon, ctc_decode = "beam" or attn_decode = "beam" the option is an error.

opt.lexicon_shortlist = K (absent or None: as above, bit for bit) decodes against a large shared lexicon, opt.lexicon on a CTC head and
opt.attn_lexicon on the attention head, by the lexicon protocol of the CRNN paper (Shi et al., section 3.3): the lexicon-free
transcription the forward already has (the arg-max per step; on a CTC head collapsed), the K words nearest to it by edit distance
over class tokens (one ops.lexicon_shortlist call per batch, a tie to the lower word index; opt.lexicon_max_distance, absent or None:
no cut-off, drops the words further away), and among those the word of largest probability by the exact candidate scoring of
opt.candidates (ops.ctc_lexicon_decode(cand=) / attn_shortlist=(handle, K, max distance) on the evaluation forward).  The word table
is encoded and uploaded once per call and the candidate table never leaves the device.  On the attention head the trie beam is not
run and beam_width is not read.  opt.lexicon_top_n still applies.  A sample whose shortlist is empty scores as the empty prediction
with confidence 0.  Without the head's lexicon option, or together with candidates, the option is an error.
"""
import time

import numpy as np
import torch

from . import functional as Fn
from . import ops
from .modules import decoding as D
from .modules import scoring as S

SCORE_TIMER = None     # a list here collects, per batch, the host seconds from the loss being on the host to the scores being there


def edit_distance(a, b):
    """Levenshtein distance (the reference uses nltk.metrics.distance.edit_distance with its default unit costs)."""
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def _search_option(shortlist, candidates, lexicon=False):
    """the option behind an attention head's second decode, as an error names it"""
    return "lexicon_shortlist" if shortlist else "candidates" if candidates else "attn_lexicon" if lexicon else "attn_decode='beam'"


def _forward(model, image, opt, converter, val_choose, attn_beam=None, attn_lexicon=None, attn_candidates=None, attn_shortlist=None,
             attn_lm=None):
    """the reference's call patterns (test.py:163-201): "FF" = newest expert, "TF" = routed ensemble, else a plain Model.
    attn_beam (a width, attention heads only): -> (logits, (beam path, beam probabilities)) instead of the logits; attn_lexicon (a
    trie handle beside it): the pair of the lexicon-constrained search; attn_candidates (a candidate handle instead of both): the pair
    of the batch's exact candidate scoring; attn_shortlist ((word handle, K, max distance) instead of all three): the pair of the best
    word of the greedy hypothesis' shortlist; attn_lm ((model handle, weight, bonus, top_n) beside attn_beam alone): the pair of the
    beam search fused with that language model"""
    if "CTC" in opt.Prediction:
        if val_choose == "FF":
            out = model(image, cross=False, is_train=False)
        elif val_choose == "TF":
            out = model(image, cross=True, is_train=False)
        else:
            out = model(image, is_train=False)
    else:
        sos = torch.full((image.size(0),), converter.dict["[SOS]"], dtype=torch.long, device=image.device)
        kw = {k: v for k, v in (("attn_beam", attn_beam), ("attn_lexicon", attn_lexicon), ("attn_candidates", attn_candidates),
                                ("attn_shortlist", attn_shortlist), ("attn_lm", attn_lm)) if v is not None}
        if val_choose == "FF":
            out = model(image, cross=False, text=sos, is_train=False, **kw)
        elif val_choose == "TF":
            out = model(image, cross=True, text=sos, is_train=False, **kw)
        else:
            out = model(image, text=sos, is_train=False, **kw)
    logits = out["logits"] if "logits" in out else out["predict"]
    if attn_beam is None and attn_candidates is None and attn_shortlist is None:
        return logits
    if "beam_path" not in out:
        what = _search_option(attn_shortlist is not None, attn_candidates is not None)
        raise RuntimeError(f"{what}: the evaluation forward returned no beam pair (it runs under torch.no_grad() only)")
    return logits, (out["beam_path"], out["beam_prob"])


def _ned_term(n_gt, n_prd, distance):
    """one sample's ICDAR-2019 normalised edit distance term (test.py:243-250), or None when there is nothing to add"""
    if n_gt == 0 or n_prd == 0:
        return None
    if n_gt > n_prd:
        return 1 - distance() / n_gt
    return 1 - distance() / n_prd


def _host_scores(labels, preds_str, probs, attn, ned):
    """the reference's per-sample loop on strings (test.py:222-260) -> per sample (NED term or None, exact match, confidence)"""
    out = []
    for gt, prd, prd_max_prob in zip(labels, preds_str, probs):
        if attn:
            eos = prd.find("[EOS]")
            prd = prd[:eos]                 # find() == -1 (no [EOS]): drops the last character, as the reference does
            prd_max_prob = prd_max_prob[:eos]
        term = _ned_term(len(gt), len(prd), lambda: edit_distance(prd, gt)) if ned else None
        conf = float(np.cumprod(prd_max_prob.astype(np.float32))[-1]) if len(prd_max_prob) else 0
        out.append((term, prd == gt, conf))
    return out


def _device_scores(labels, preds_index, preds_max_prob, converter, canon, attn, ned, width):
    """one H2D copy of the canonical labels, one launch, one D2H copy of result + confidence; the samples the kernel flags are
    scored by _host_scores from one fetch of the batch's indices / probabilities -> (per-sample scores, kept tokens, host strings)"""
    B, T = preds_index.shape
    lab, lab_len = S.canonical_labels(converter, labels, width)
    host = torch.from_numpy(np.concatenate([lab_len, lab.reshape(-1)])).pin_memory().to(preds_index.device, non_blocking=True)
    tokens, _, _, packed = ops.greedy_score(preds_index.contiguous(), preds_max_prob.contiguous(), host[B:].view(B, width), host[:B],
                                            canon, S.MODE_ATTN if attn else S.MODE_CTC, converter.dict["[EOS]"] if attn else 0)
    packed = packed.cpu().numpy()
    result, conf = packed[:B * 4].reshape(B, 4).tolist(), packed[B * 4:].view(np.float32)
    flagged = [b for b in range(B) if result[b][3]]
    host_rows = {}
    if flagged:
        index, probs = preds_index.cpu().numpy(), preds_max_prob.cpu().numpy()
        strings = converter.decode(index[flagged], [T] * len(flagged))
        scored = _host_scores([labels[b] for b in flagged], strings, probs[flagged], attn, ned)
        host_rows = {b: (sc, st) for b, sc, st in zip(flagged, scored, strings)}
    out = []
    for b in range(B):
        if b in host_rows:
            out.append(host_rows[b][0])
            continue
        n_prd, dist, match, _ = result[b]
        term = _ned_term(int(lab_len[b]), n_prd, lambda: dist) if ned else None
        out.append((term, bool(match), float(conf[b]) if not attn or n_prd else 0))    # attention: kept tokens = kept probabilities
    return out, (tokens, result), {b: st for b, (_, st) in host_rows.items()}


def _beam_pair(preds, prediction, width, top_n, fusion=None):
    """the beam decoder's (path, prob) for CTC logits [B,T,C], on the device of `preds`: one launch when the kernel takes the batch,
    else the host form; fusion = a _BeamLM (opt.ctc_lm) or None"""
    if fusion is not None:
        return fusion.pair(preds, prediction, width, top_n)
    if preds.is_cuda and D.beam_supported(prediction, preds.size(1), preds.size(2), width, top_n):
        return ops.ctc_beam_decode(preds if preds.stride(-1) == 1 else preds.contiguous(), width, top_n)[3:]
    path, prob = D.ctc_beam_host(preds.detach().cpu().numpy(), width, top_n)[3:]
    return torch.from_numpy(path).to(preds.device), torch.from_numpy(prob).to(preds.device)


class _BeamLM:
    """opt.ctc_lm with its weights for one validation() call; the model is checked and uploaded when the first CUDA batch needs it"""

    def __init__(self, lm, weight, bonus):
        self.lm, self.weight, self.bonus, self.handle = lm, weight, bonus, None

    def pair(self, preds, prediction, width, top_n):
        """the fused beam decoder's (path, prob) of the best entry by the fused key; prob[0] is still exp(acoustic score)"""
        if (preds.is_cuda and D.beam_supported(prediction, preds.size(1), preds.size(2), width, top_n)
                and D.beam_lm_supported(self.lm)):
            if self.handle is None:
                self.handle = ops.upload_char_lm(self.lm, preds.device)
            return ops.ctc_beam_decode(preds if preds.stride(-1) == 1 else preds.contiguous(), width, top_n, self.handle, self.weight,
                                       self.bonus)[3:5]
        path, prob = D.ctc_beam_host(preds.detach().cpu().numpy(), width, top_n, self.lm, self.weight, self.bonus)[3:5]
        return torch.from_numpy(path).to(preds.device), torch.from_numpy(prob).to(preds.device)


class _AttnLM:
    """opt.attn_lm with its weights for one validation() call; the model is checked and uploaded when the first batch needs it"""

    def __init__(self, lm, weight, bonus, top_n):
        self.lm, self.weight, self.bonus, self.top_n, self.handle = lm, weight, bonus, top_n, None

    def on(self, device):
        """the attn_lm= of the evaluation forward"""
        if self.handle is None:
            self.handle = ops.upload_char_lm(self.lm, device)
        return self.handle, self.weight, self.bonus, self.top_n


class _Lexicon:
    """opt.lexicon encoded once per validation() call; the device copies are made when the first CUDA batch needs them"""

    def __init__(self, converter, words, n, shortlist=None):
        self.tokens, self.lengths, self.words = D.encode_lexicon(converter, words)
        self.n = n
        self.device = None
        self.shortlist, self.handle = shortlist, None        # (K, max distance) of opt.lexicon_shortlist

    def _shortlist_pair(self, preds, prediction):
        """pair() by the lexicon protocol: the best path's tokens, their K nearest words, the exact scores of those"""
        K, max_dist = self.shortlist
        if self.handle is None:
            self.handle = ops.upload_words(self.tokens, self.lengths, preds.device, self.n)
        if preds.is_cuda:
            cand, _ = ops.lexicon_shortlist(*ops.hypothesis_of_frames(ops.argmax_lastdim(preds)), self.handle, K, max_dist)
            if D.lexicon_supported(prediction, preds.size(1), preds.size(2), int(self.lengths.max()), len(self.lengths), self.n):
                return ops.ctc_lexicon_decode(preds if preds.stride(-1) == 1 else preds.contiguous(), *self.handle.on_device(), n=self.n,
                                              cand=cand)[3:]
            cand = cand.cpu().numpy()
        else:
            cand, _ = D.lexicon_shortlist_host(*D.hypothesis_of_frames(preds.argmax(dim=2).numpy()), self.tokens, self.lengths, K, max_dist)
        path, prob = D.ctc_lexicon_host(preds.detach().cpu().numpy(), self.tokens, self.lengths, self.n, cand)[3:]
        return torch.from_numpy(path).to(preds.device), torch.from_numpy(prob).to(preds.device)

    def pair(self, preds, prediction):
        """the lexicon decoder's (path, prob) for CTC logits [B,T,C], on the device of `preds`: the kernel when it takes the batch,
        else the host form"""
        if self.shortlist is not None:
            return self._shortlist_pair(preds, prediction)
        N = len(self.lengths)
        if preds.is_cuda and D.lexicon_supported(prediction, preds.size(1), preds.size(2), int(self.lengths.max()), N, self.n):
            if self.device is None:
                self.device = (torch.from_numpy(self.tokens).to(preds.device), torch.from_numpy(self.lengths).to(preds.device))
            return ops.ctc_lexicon_decode(preds if preds.stride(-1) == 1 else preds.contiguous(), *self.device, n=self.n)[3:]
        path, prob = D.ctc_lexicon_host(preds.detach().cpu().numpy(), self.tokens, self.lengths, self.n)[3:]
        return torch.from_numpy(path).to(preds.device), torch.from_numpy(prob).to(preds.device)


class _AttnLexicon:
    """opt.attn_lexicon encoded and built into a trie once per validation() call; checked and uploaded when the first batch needs it"""

    def __init__(self, converter, words, batch_max_length):
        tokens, lengths, self.words = D.encode_attn_lexicon(converter, words, batch_max_length)
        self.trie = D.build_trie(tokens, lengths)
        self.handle = None

    def on(self, device):
        if self.handle is None:
            self.handle = ops.upload_trie(self.trie, device)
        return self.handle


class _AttnShortlist:
    """opt.attn_lexicon with opt.lexicon_shortlist: the word table encoded once per validation() call, uploaded when the first batch needs
    it; no trie"""

    def __init__(self, converter, words, batch_max_length, n, K, max_dist):
        self.tokens, self.lengths, self.words = D.encode_attn_lexicon(converter, words, batch_max_length)
        self.n, self.K, self.max_dist, self.handle = n, K, max_dist, None

    def on(self, device):
        """the attn_shortlist= of the evaluation forward"""
        if self.handle is None:
            self.handle = ops.upload_words(self.tokens, self.lengths, device, self.n)
        return self.handle, self.K, self.max_dist


class _Candidates:
    """opt.candidates: the union of the word lists encoded once per validation() call, the candidate table built per batch"""

    def __init__(self, converter, candidates, loader, attn, batch_max_length, n):
        self.candidates, self.attn, self.n, self.S = candidates, attn, n, batch_max_length + 1
        if isinstance(candidates, dict):
            lists = D.candidate_lists(candidates, list(candidates))
        else:                               # the union is over the loader's labels, whatever order they come in
            lists = [words for _, labels in loader for words in D.candidate_lists(candidates, labels)]
        self.table = D.CandidateTable(converter, lists, attn, batch_max_length)
        self.device = self.handle = None

    def cand(self, labels):
        return self.table.rows(D.candidate_lists(self.candidates, labels))

    def on(self, device, labels):
        """attention head: the handle of the evaluation forward for this batch"""
        if self.handle is None:
            self.handle = ops.upload_words(self.table.tokens, self.table.lengths, device, self.n)
        return self.handle.with_cand(self.cand(labels), self.S)

    def pair(self, preds, prediction, labels):
        """CTC head: the lexicon decoder's (path, prob) for logits [B,T,C] against the batch's candidate table, on the device of
        `preds`: the kernel when it takes the batch, else the host form"""
        cand, t = self.cand(labels), self.table
        if preds.is_cuda and D.lexicon_supported(prediction, preds.size(1), preds.size(2), int(t.lengths.max()), len(t.lengths), self.n):
            if self.device is None:
                self.device = (torch.from_numpy(t.tokens).to(preds.device), torch.from_numpy(t.lengths).to(preds.device))
            return ops.ctc_lexicon_decode(preds if preds.stride(-1) == 1 else preds.contiguous(), *self.device, n=self.n,
                                          cand=torch.from_numpy(cand).to(preds.device))[3:]
        path, prob = D.ctc_lexicon_host(preds.detach().cpu().numpy(), t.tokens, t.lengths, self.n, cand)[3:]
        return torch.from_numpy(path).to(preds.device), torch.from_numpy(prob).to(preds.device)


def validation(model, criterion, evaluation_loader, converter, opt, val_choose="val", tqdm_position=1):
    n_correct, norm_ED, length_of_data, infer_time = 0, 0.0, 0, 0.0
    loss_sum, loss_n = 0.0, 0
    preds_str, confidence_score_list, labels = [], [], []
    params = list(model.parameters()) if hasattr(model, "parameters") else []
    dev = params[0].device if params else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    attn, ned = "Attn" in opt.Prediction, getattr(opt, "NED", False)
    canon, last = None, None
    ctc_decode, beam_width, beam_top_n = D.decode_options(opt)
    attn_decode, attn_width = D.attn_decode_options(opt)
    attn_beam = attn_width if attn and attn_decode == "beam" else None
    attn_words, attn_lexicon_width = D.attn_lexicon_options(opt)
    attn_lexicon = attn_shortlist = None
    lexicon_words, lexicon_n = D.lexicon_options(opt)
    shortlist = D.shortlist_request(opt, attn)               # (K, max distance) or None
    if attn and attn_words is not None and shortlist is not None:
        attn_shortlist, attn_beam = _AttnShortlist(converter, attn_words, opt.batch_max_length, lexicon_n, *shortlist), None
    elif attn and attn_words is not None:
        attn_lexicon, attn_beam = _AttnLexicon(converter, attn_words, opt.batch_max_length), attn_lexicon_width
    if lexicon_words is not None and not attn and ctc_decode == "beam":
        raise ValueError("lexicon and ctc_decode='beam' both replace best-path decoding on a CTC head: set one of them")
    lexicon = _Lexicon(converter, lexicon_words, lexicon_n, shortlist) if lexicon_words is not None and not attn else None
    ctc_lm, lm_weight, lm_bonus = D.lm_options(opt, attn)
    fusion = _BeamLM(ctc_lm, lm_weight, lm_bonus) if ctc_lm is not None else None
    attn_lm = D.attn_lm_options(opt, attn)
    attn_fusion = _AttnLM(*attn_lm) if attn_lm[0] is not None else None
    cand_fn, cand_n = D.candidates_options(opt)
    candidates = None
    if cand_fn is not None:
        candidates = _Candidates(converter, cand_fn, evaluation_loader, attn, opt.batch_max_length, cand_n)
    if (attn_beam is not None or attn_shortlist is not None or (attn and candidates is not None)) and converter.dict["[EOS]"] != D.ATTN_EOS:
        what = _search_option(attn_shortlist is not None, candidates is not None, attn_lexicon is not None)
        raise ValueError(f"{what} ends an entry on token {D.ATTN_EOS}, the converter's [EOS] is {converter.dict['[EOS]']}")
    for image_tensors, labels in evaluation_loader:
        batch_size = image_tensors.size(0)
        length_of_data += batch_size
        image = image_tensors.to(dev)
        labels_index, labels_length = converter.encode(labels, batch_max_length=opt.batch_max_length)
        if image.is_cuda:
            torch.cuda.synchronize()                 # the launches are asynchronous: infer_time is forward time, not host issue time
        start = time.time()
        attn_cands = candidates.on(image.device, labels) if attn and candidates is not None else None
        preds = _forward(model, image, opt, converter, val_choose, attn_beam=attn_beam,
                         attn_lexicon=None if attn_lexicon is None else attn_lexicon.on(image.device), attn_candidates=attn_cands,
                         attn_shortlist=None if attn_shortlist is None else attn_shortlist.on(image.device),
                         attn_lm=None if attn_fusion is None else attn_fusion.on(image.device))
        if attn_beam is not None or attn_cands is not None or attn_shortlist is not None:
            preds, beam_pair = preds
        if image.is_cuda:
            torch.cuda.synchronize()
        infer_time += time.time() - start
        if criterion is not None:               # the learners' Criterion (il_modules/base.py): CTC or CE(ignore [PAD]) :178-207
            cost = criterion(preds, labels_index, labels_length)
        elif attn:
            cost = Fn.cross_entropy(preds, labels_index[:, 1:], converter.dict["[PAD]"])
        else:
            cost = Fn.ctc_loss(preds.contiguous() if preds.stride(-1) != 1 else preds, labels_index, labels_length)
        loss_sum += float(cost)
        loss_n += 1
        if SCORE_TIMER is not None:
            t_score = time.perf_counter()
        if candidates is not None and not attn:
            preds_index, preds_max_prob = candidates.pair(preds, opt.Prediction, labels)
        elif lexicon is not None:
            preds_index, preds_max_prob = lexicon.pair(preds, opt.Prediction)
        elif ctc_decode == "beam" and not attn:
            preds_index, preds_max_prob = _beam_pair(preds, opt.Prediction, beam_width, beam_top_n, fusion)
        elif attn_beam is not None or attn_cands is not None or attn_shortlist is not None:
            preds_index, preds_max_prob = beam_pair
        else:
            preds_index, preds_max_prob = ops.argmax_prob_lastdim(preds)                     # :211, :218-219
        T = preds.size(1)
        width = max((len(gt) for gt in labels), default=0)
        if preds_index.is_cuda and S.device_scoring_supported(converter, opt.Prediction, T, width):
            if canon is None:               # once per call, never kept on the converter: MRN rebuilds its character set per task
                canon = torch.from_numpy(S.canonical_table(converter, opt.Prediction)).to(preds_index.device)
            scores, kept, host_strings = _device_scores(labels, preds_index, preds_max_prob, converter, canon, attn, ned, width)
            last = (preds_index, kept, host_strings)
        else:
            preds_str = converter.decode(preds_index.cpu().numpy(), [T] * batch_size)
            scores = _host_scores(labels, preds_str, preds_max_prob.cpu().numpy(), attn, ned)
            last = None
        confidence_score_list = []
        for term, correct, conf in scores:  # the reference's accumulation, sample by sample in its order
            if term is not None:
                norm_ED += term
            if correct:
                n_correct += 1
            confidence_score_list.append(conf)
        if SCORE_TIMER is not None:
            SCORE_TIMER.append(time.perf_counter() - t_score)
    if last is not None:                    # the reference returns the LAST batch's strings only: decode nothing else
        preds_index, (tokens, result), host_strings = last
        if attn:                            # the returned strings are the unpruned decode of all T steps (test.py:213,274)
            preds_str = converter.decode(preds_index.cpu().numpy(), [preds_index.size(1)] * preds_index.size(0))
        else:
            tokens = tokens.cpu().numpy()
            preds_str = [host_strings[b] if b in host_strings else "".join(converter.character[k] for k in tokens[b, :result[b][0]])
                         for b in range(len(result))]
    ned_score = norm_ED / float(length_of_data) * 100 if ned else None
    score = n_correct / float(length_of_data) * 100
    valid_loss = loss_sum / max(loss_n, 1)
    return valid_loss, score, ned_score, preds_str, confidence_score_list, labels, infer_time, length_of_data
