"""mrn_ctc_lexicon_decode_f32 (mrn_amd/csrc/ctc_lexicon.hip) against the independent reference of tests/lexicon_cases.py (torch
ctc_loss, float64, CPU) and against the float64 host form (mrn_amd/modules/decoding.py::ctc_lexicon_host) on the inputs
tests/test_lexicon_cpu.py holds the host form to the reference on; ties, dead slots, non-finite logits; the limits; validation()
with opt.lexicon.

Tolerance.  score_all against the float64 reference on live pairs: atol = 1e-5, rtol = 1e-5, the band tests/test_long_labels_gpu.py
holds the CTC loss kernels to against torch; pairs at -inf agree exactly.  The ranking is checked on the kernel's own scores (it is
exact there: descending score, a tie to the lower position), and against the host form's wherever the host form's neighbouring
scores are further apart than twice the band."""
import math

import numpy as np
import pytest
import torch

from tests import lexicon_cases as LC

pytestmark = pytest.mark.gpu


def band(ref):
    return LC.ATOL + LC.RTOL * np.abs(ref)


def decode(case, x=None, **kw):
    from mrn_amd import ops
    x = torch.from_numpy(np.array(case["x"])).cuda() if x is None else x
    cand = None if case["cand"] is None else torch.from_numpy(case["cand"]).cuda()
    out = ops.ctc_lexicon_decode(x, torch.from_numpy(case["tokens"]).cuda(), torch.from_numpy(case["lens"]).cuda(), kw.pop("n", case["n"]),
                                 cand, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def host(case):
    from mrn_amd.modules.decoding import ctc_lexicon_host
    return ctc_lexicon_host(case["x"], case["tokens"], case["lens"], case["n"], cand=case["cand"])


def check_outputs(case, outs, ref):
    """score_all within the band of ref (float64 [B][Nc], -inf = dead); index / score = the exact ranking of the kernel's own
    score_all; path / prob = the best word's hand-over"""
    from mrn_amd.modules.decoding import frame_path
    index, score, score_all, path, prob = outs
    B, T, _ = case["x"].shape
    n = index.shape[1]
    assert index.dtype == np.int32 and score.dtype == np.float32 and score_all.dtype == np.float32
    assert path.dtype == np.int64 and prob.dtype == np.float32 and path.shape == (B, T) and prob.shape == (B, T)
    dead = ref == -np.inf
    assert (score_all[dead] == -np.inf).all()
    live_err = np.abs(score_all[~dead].astype(np.float64) - ref[~dead])
    print(f"live pairs {live_err.size}, largest |score - reference| {live_err.max(initial=0.0):.3e}, "
          f"largest share of the band {(live_err / band(ref[~dead])).max(initial=0.0):.3f}")
    assert np.isfinite(score_all[~dead]).all() and (live_err <= band(ref[~dead])).all()
    words = LC.unpack(case["tokens"], case["lens"])
    for b in range(B):
        at = np.arange(len(words)) if case["cand"] is None else case["cand"][b]
        order = LC.rank(score_all[b], n)
        assert index[b, :len(order)].tolist() == [int(at[q]) for q in order]
        assert score[b, :len(order)].tobytes() == score_all[b, order].tobytes()
        assert (index[b, len(order):] == -1).all() and (score[b, len(order):] == -np.inf).all()
        if order:
            assert path[b].tolist() == frame_path(words[index[b, 0]], T)
            assert prob[b, 0] > 0 or score[b, 0] < -87
            assert abs(float(prob[b, 0]) - math.exp(float(score[b, 0]))) <= 2e-6 * math.exp(float(score[b, 0])) + 2e-45
        else:
            assert (path[b] == 0).all() and prob[b, 0] == 0
        assert (prob[b, 1:] == 1).all()


def check_ranking_against_host(case, outs):
    """where the host form's kept entries (and the first dropped one) are further apart than twice the band, the indices agree"""
    index = outs[0]
    h_index, _, h_all, _, _ = host(case)
    for b in range(len(index)):
        top = np.sort(h_all[b][h_all[b] > -np.inf])[::-1][:index.shape[1] + 1]
        gaps = top[:-1] - top[1:]
        if len(top) > 1 and (gaps <= 2 * band(top[:-1])).any():
            continue
        assert index[b].tolist() == h_index[b].tolist()


def run_case(name, maker, *args):
    case = maker(*args)
    outs = decode(case)
    check_outputs(case, outs, LC.reference(name, maker, *args))
    return case, outs


# ---- 1. all pairs ----------------------------------------------------------------------------------------------------------------
def test_all_pairs_with_a_padded_row_stride():
    case = LC.all_pairs()
    B, T, C = case["x"].shape
    padded = torch.full((B, T, C + 3), float("nan"), device="cuda")
    padded[:, :, :C] = torch.from_numpy(np.array(case["x"]))
    view = padded[:, :, :C]
    assert view.stride() == (T * (C + 3), C + 3, 1)
    outs = decode(case, view)
    check_outputs(case, outs, LC.reference("all_pairs", LC.all_pairs))
    check_ranking_against_host(case, outs)
    assert (outs[2] == -np.inf).any() and outs[0].shape == (3, 4)
    stepped = torch.zeros(B, 2 * T, C, device="cuda")               # a step stride of its own, too
    stepped[:, ::2] = view
    for a, b in zip(outs, decode(case, stepped[:, ::2])):
        assert a.tobytes() == b.tobytes()


# ---- 2. 3. 4. 5. the edges of states, frames, classes, word and sample counts ------------------------------------------------------
@pytest.mark.parametrize("L,T", LC.STATE_EDGE)
def test_state_edge(L, T):
    case, outs = run_case("state_edge", LC.state_edge, L, T)
    check_ranking_against_host(case, outs)


@pytest.mark.parametrize("T", [1, 2, 512])
def test_frames(T):
    run_case("frames", LC.frames, T)


@pytest.mark.parametrize("C", [2, 65535])
def test_classes(C):
    run_case("classes", LC.classes, C)


@pytest.mark.parametrize("N,B", LC.TAILS)
def test_tails(N, B):
    case, outs = run_case("tails", LC.tails, N, B)
    check_ranking_against_host(case, outs)


# ---- 6. candidate lists ------------------------------------------------------------------------------------------------------------
def test_candidate_lists_equal_the_gathered_full_scoring():
    case, outs = run_case("candidates", LC.candidates)
    full = decode({**case, "cand": None})[2]
    cand = case["cand"]
    gathered = np.where(cand >= 0, np.take_along_axis(full, np.maximum(cand, 0), axis=1), np.float32(-np.inf))
    assert outs[2].tobytes() == gathered.astype(np.float32).tobytes()           # the same recursion on the same operands: bit for bit
    assert (outs[0][3] == -1).all() and (outs[3][3] == 0).all() and outs[4][3, 0] == 0
    assert outs[2][0, 2] == outs[2][0, 3]                                        # a word named twice


# ---- 7. ties and dead slots --------------------------------------------------------------------------------------------------------
def test_ties_and_dead_slots():
    case, (index, score, score_all, path, prob) = run_case("ties", LC.ties)
    for b in range(3):
        assert score_all[b, 0] == score_all[b, 2] == score_all[b, 5] and score_all[b, 1] == score_all[b, 3]      # bit-equal
        live = index[b][index[b] >= 0].tolist()
        assert len(live) == 6 and live.index(0) < live.index(2) < live.index(5) and live.index(1) < live.index(3)
        assert index[b, 6:].tolist() == [-1, -1] and (score[b, 6:] == -np.inf).all()
    case, (index, score, score_all, path, prob) = run_case("all_dead", LC.all_dead)
    assert (index == -1).all() and (score == -np.inf).all() and (score_all == -np.inf).all()
    assert (path == 0).all() and (prob[:, 0] == 0).all() and (prob[:, 1:] == 1).all()


# ---- 8. non-finite logits ----------------------------------------------------------------------------------------------------------
def test_non_finite_logits():
    case = LC.non_finite()
    ref = host(case)[2]                   # the rules for NaN / inf are the algorithm's; test_lexicon_cpu.py states them on the host form
    clean = LC.reference_scores({**case, "x": case["x"][:1]})
    assert np.abs(ref[0] - clean[0]).max() <= 1e-9
    outs = decode(case)
    check_outputs(case, outs, ref)
    index, score, score_all, path, prob = outs
    assert not np.isnan(score_all).any() and not np.isnan(prob).any()
    for b in (1, 3, 4):
        assert (score_all[b] == -np.inf).all() and (index[b] == -1).all() and (path[b] == 0).all() and prob[b, 0] == 0
    words = LC.unpack(case["tokens"], case["lens"])
    for q, w in enumerate(words):
        assert (score_all[2, q] == -np.inf) == (3 in w)
    assert (score_all[0] > -np.inf).all()


# ---- 9. agreement with the host form at an evaluation shape ------------------------------------------------------------------------
def test_agreement_with_the_host_form():
    case = LC.agreement()
    h_index, h_score, h_all, _, _ = host(case)
    outs = decode(case)
    check_outputs(case, outs, h_all)
    narrow = (h_score[:, 0] - h_score[:, 1]) < 1e-3
    assert narrow.mean() <= 0.05
    assert (outs[0][~narrow, 0] == h_index[~narrow, 0]).all()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------
def raw_call(B=1, T=8, C=12, words=([1, 2], [3]), n=2, cand=None, K=None, tokens=None, lens=None, N=None):
    """one mrn_ctc_lexicon_decode_f32 call on zero logits with recognisable output buffers -> (the error or None, outputs untouched)"""
    from mrn_amd import _lib
    from mrn_amd.ops import _p, _stream
    tk, ln = LC.pack([list(w) for w in words])
    tk = torch.from_numpy(tk if tokens is None else np.asarray(tokens, dtype=np.int32)).cuda()
    ln = torch.from_numpy(ln if lens is None else np.asarray(lens, dtype=np.int32)).cuda()
    N = tk.shape[0] if N is None else N
    cd = None if cand is None else torch.from_numpy(np.asarray(cand, dtype=np.int32)).cuda()
    K = (0 if cd is None else cd.shape[1]) if K is None else K
    x = torch.zeros(B, max(T, 1), max(C, 1), device="cuda")
    keep = max(n, 1)
    outs = [torch.full((B, keep), 77, device="cuda", dtype=torch.int32), torch.full((B, keep), 77.0, device="cuda"),
            torch.full((B, max(K if cd is not None else N, 1)), 77.0, device="cuda"),
            torch.full((B, max(T, 1)), 77, device="cuda", dtype=torch.int64), torch.full((B, max(T, 1)), 77.0, device="cuda")]
    error = None
    try:
        _lib.call("mrn_ctc_lexicon_decode_f32", _p(x), x.stride(0), x.stride(1), B, T, C, _p(tk), tk.shape[1], _p(ln), N, _p(cd), K, n,
                  *[_p(o) for o in outs], _stream())
    except RuntimeError as e:
        error = str(e)
    torch.cuda.synchronize()
    return error, all(bool((o == 77).all()) for o in outs)


def test_limits_are_error_codes_and_leave_the_outputs_alone():
    error, untouched = raw_call()
    assert error is None and not untouched
    big = np.zeros(((1 << 20) + 1, 1), dtype=np.int32)
    for what, kw in (("T = 513", dict(T=513)), ("T = 0", dict(T=0)), ("C = 1", dict(C=1)), ("C = 65536", dict(C=65536)),
                     ("N = 0", dict(N=0)), (f"N = {(1 << 20) + 1}", dict(tokens=big, lens=big[:, 0])), ("n = 0", dict(n=0)),
                     ("n = 17", dict(n=17)), ("K = 0", dict(cand=[[0]], K=0)),
                     ("word length", dict(T=80, C=40, words=([5] * 16 + [6] * 16,))),             # L = 32
                     ("word length", dict(lens=[3, 1])),                                          # above the table's width
                     ("word length", dict(lens=[-1, 1])),
                     ("word token", dict(words=([1, 0], [3]))), ("word token", dict(words=([1, 12], [3]))),
                     ("word token", dict(words=([1, -4], [3]))),
                     ("candidate index", dict(cand=[[0, 2]])), ("candidate index", dict(cand=[[-2, 1]]))):
        error, untouched = raw_call(**kw)
        assert error is not None and "mrn_ctc_lexicon_decode_f32 failed (code -1)" in error and what in error, (what, error)
        assert untouched, what
    error, untouched = raw_call(words=([1, 2], [3] * 2 + [0]), lens=[2, 2])        # whatever lies behind a word's length is not read
    assert error is None
    error, untouched = raw_call(T=70, C=40, words=(list(range(1, 32)),))          # L = 31 is inside
    assert error is None


def test_ops_checks_its_operands_and_takes_the_host_form_outside_the_limits():
    from mrn_amd import ops
    from tests.test_scoring_gpu import recorded_calls
    case = LC.all_pairs()
    x = torch.from_numpy(np.array(case["x"])).cuda()
    tk, ln = torch.from_numpy(case["tokens"]).cuda(), torch.from_numpy(case["lens"]).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_lexicon_decode(x.cpu(), tk, ln)
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        ops.ctc_lexicon_decode(torch.zeros(3, 12, 14, device="cuda")[:, :, ::2], tk, ln)
    with pytest.raises(RuntimeError, match="int32"):
        ops.ctc_lexicon_decode(x, tk.long(), ln)
    with pytest.raises(RuntimeError, match="K >= 1"):
        ops.ctc_lexicon_decode(x, tk, ln, cand=torch.zeros(3, 0, device="cuda", dtype=torch.int32))
    assert ops.ctc_lexicon_decode(x[:0], tk, ln, 2)[0].shape == (0, 2)
    # a table of 33 columns and 17 entries per sample are outside the kernel: the host form answers, the kernel is never called
    wide = torch.zeros(40, 33, device="cuda", dtype=torch.int32)
    wide[:, :tk.shape[1]] = tk
    ref = host(case)
    for kw in (dict(lex_tokens=wide, n=4), dict(lex_tokens=tk, n=17)):
        with recorded_calls() as log:
            outs = ops.ctc_lexicon_decode(x, kw["lex_tokens"], ln, kw["n"])
        assert log.count("mrn_ctc_lexicon_decode_f32") == 0
        assert all(o.is_cuda for o in outs) and outs[2].dtype == torch.float32 and outs[0].shape == (3, kw["n"])
        assert outs[0][:, :4].cpu().numpy().tolist() == ref[0].tolist()
        assert outs[2].cpu().numpy().tobytes() == ref[2].astype(np.float32).tobytes()
        assert outs[3].cpu().numpy().tolist() == ref[3].tolist()
    with recorded_calls() as log:
        ops.ctc_lexicon_decode(x, tk, ln, 4)
    assert log.count("mrn_ctc_lexicon_decode_f32") == 1                           # one call per batch


def test_a_batch_is_cut_into_chunks_of_samples(monkeypatch):
    """a score table above the budget: the batch goes through in chunks, the outputs are those of one call, score_all is dropped"""
    from mrn_amd import ops
    from tests.test_scoring_gpu import recorded_calls
    case = LC.tails(257, 17)
    one = decode(case)
    monkeypatch.setattr(ops, "LEXICON_SCORE_BYTES", 5 * 257 * 4)               # five samples per call
    with recorded_calls() as log:
        cut = decode_chunked(case)
    assert log.count("mrn_ctc_lexicon_decode_f32") == 4
    assert cut[2] is None
    for i in (0, 1, 3, 4):
        assert cut[i].tobytes() == one[i].tobytes()


def decode_chunked(case):
    from mrn_amd import ops
    out = ops.ctc_lexicon_decode(torch.from_numpy(np.array(case["x"])).cuda(), torch.from_numpy(case["tokens"]).cuda(),
                                 torch.from_numpy(case["lens"]).cuda(), case["n"])
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in out]


# ---- 11. validation() --------------------------------------------------------------------------------------------------------------
def lexicon_of(batches, conv, logits):
    """what best path reads in the tiny CRNN's logits (its weights are random: the labels are far from it), labels of the batches,
    near misses of both, a word the converter cannot spell, a tripled character, the empty word; no word twice, so that a sample's
    top two are never a tie"""
    T = logits[0].shape[1]
    chars = conv.character[4:]
    read = [s for lg in logits for s in conv.decode(lg.argmax(axis=2), [T] * len(lg))]
    read = [s for s in read if all(ch in chars for ch in s)]          # (a predicted [PAD] / [UNK] decodes to its name: no word)
    labels = [gt for _, batch in batches for gt in batch]
    near = [w[:-1] + chars[(chars.index(w[-1]) + 3) % len(chars)] for w in read[:8] + labels[:8] if w]
    words = list(dict.fromkeys(read + labels[:12] + near + [chars[5] * 3, ""]))
    return words[:5] + ["not in the character set"] + words[5:]


def test_validation_with_a_lexicon(monkeypatch):
    from mrn_amd.modules import decoding as D
    from mrn_amd.test import _host_scores
    from tests.test_ctc_beam_gpu import run_validation, validation_case
    from tests.test_scoring_gpu import recorded_calls
    _, conv, _, _, batches, logits = validation_case()
    lexicon = lexicon_of(batches, conv, logits)
    tokens, lengths, kept = D.encode_lexicon(conv, lexicon)
    assert len(kept) == len(lexicon) - 1
    T = logits[0].shape[1]
    n_correct, norm_ed, strings, scores = 0, 0.0, None, []
    for (_, labels), lg in zip(batches, logits):          # the expected returns: the host form's best words through the host string loop
        index, score, score_all, path, prob = D.ctc_lexicon_host(lg, tokens, lengths, 2)
        assert ((score[:, 0] - score[:, 1]) > 2 * band(score[:, 0])).all()     # the inputs' own property: float32 cannot swap the top two
        strings = conv.decode(path, [T] * len(path))
        assert strings == [kept[i] for i in index[:, 0]]
        scores = score[:, 0].tolist()
        for term, correct, _ in _host_scores(labels, strings, prob, False, True):
            norm_ed += term if term is not None else 0
            n_correct += bool(correct)
    with recorded_calls() as log:
        lex = run_validation(monkeypatch, lexicon=lexicon)
    assert log.count("mrn_ctc_lexicon_decode_f32") == 2 and log.count("mrn_argmax_prob_f32") == 0       # one call per batch
    assert list(lex[3]) == strings
    assert lex[1] == n_correct / 16 * 100 and lex[2] == norm_ed / 16 * 100 and lex[7] == 16
    for conf, s in zip(lex[4], scores):
        print(f"confidence {conf:.6e}, exp(host score) {math.exp(s):.6e}, host score {s:.4f}")
        assert abs(conf - math.exp(s)) <= math.exp(s) * math.expm1(2 * band(s)) + 2e-45    # the score's band, exp rounded to float32
    assert max(lex[4]) > 1e-6                              # ... and not every probability underflows: the check above has teeth
    host_scored = run_validation(monkeypatch, scoring="host", lexicon=lexicon)
    for i in (0, 1, 2, 3, 4, 5, 7):                       # all but infer_time, which is a clock reading
        assert lex[i] == host_scored[i], (i, lex[i], host_scored[i])
    # outside the kernel's limits (a word of 32 characters): the host form decodes, the kernel is never called, the words agree
    long_word = "".join(conv.character[4 + i % 30] for i in range(32))
    with recorded_calls() as log:
        wide = run_validation(monkeypatch, lexicon=lexicon + [long_word])
    assert log.count("mrn_ctc_lexicon_decode_f32") == 0
    assert wide[3] == lex[3] and wide[1] == lex[1] and wide[2] == lex[2]
    # without the key, and with None: best path, bit for bit; the loss does not depend on the decoder, the confidences do
    default = run_validation(monkeypatch)
    for other in (run_validation(monkeypatch, lexicon=None), run_validation(monkeypatch, lexicon_top_n=3)):
        for i in (0, 1, 2, 3, 4, 5, 7):
            assert default[i] == other[i], (i, default[i], other[i])
    assert lex[0] == default[0] and lex[4] != default[4]
    with pytest.raises(ValueError, match="lexicon.*ctc_decode"):
        run_validation(monkeypatch, lexicon=lexicon, ctc_decode="beam")
    beam = run_validation(monkeypatch, ctc_decode="beam")
    assert beam[0] == default[0]


def test_the_attention_head_ignores_the_lexicon():
    from mrn_amd.test import validation
    from tests.helpers import crafted_validation_case
    from tests.test_validation_gpu import converter_and_criterion, make_opt
    chars, batches, logits = crafted_validation_case("trba")
    conv, crit = converter_and_criterion("trba", chars)
    res = []
    for keys in ({}, dict(lexicon=["a", "b"], ctc_decode="beam")):
        opt = make_opt("trba")
        vars(opt).update(keys)
        calls = iter(logits)
        res.append(validation(lambda image, *a, **k: {"predict": next(calls).cuda(), "feature": None}, crit, batches, conv, opt))
    for i in (0, 1, 2, 3, 4, 5, 7):
        assert res[0][i] == res[1][i]
