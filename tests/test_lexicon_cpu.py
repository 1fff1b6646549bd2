"""Lexicon-constrained decoding on the host: mrn_amd/modules/decoding.py::ctc_lexicon_host (float64 numpy) against the independent
reference of tests/lexicon_cases.py (torch ctc_loss, float64) on the inputs tests/test_lexicon_gpu.py gives the kernel; the ranking
rules; encode_lexicon / lexicon_options / lexicon_supported; the C ABI's header; validation() with opt.lexicon on CPU predictions."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import lexicon_cases as LC
from tests.test_ctc_beam_cpu import ctc_converter

HOST_TOL = 1e-9


def host(case, **kw):
    from mrn_amd.modules.decoding import ctc_lexicon_host
    return ctc_lexicon_host(case["x"], case["tokens"], case["lens"], kw.pop("n", case["n"]), cand=case["cand"], **kw)


def check_host_against_reference(name, maker, *args):
    case = maker(*args)
    ref = LC.reference(name, maker, *args)
    index, score, score_all, path, prob = host(case)
    assert score_all.dtype == np.float64 and score_all.shape == ref.shape
    dead = ref == -np.inf
    assert not np.isnan(ref).any()
    assert (score_all[dead] == -np.inf).all() and (score_all[~dead] > -np.inf).all()
    assert np.abs(score_all[~dead] - ref[~dead]).max(initial=0.0) <= HOST_TOL
    words = LC.unpack(case["tokens"], case["lens"])
    T = case["x"].shape[1]
    for b in range(len(ref)):
        at = np.arange(len(words)) if case["cand"] is None else case["cand"][b]
        for q in np.flatnonzero(dead[b]):                           # dead = unused slot or a word that does not fit the frames
            assert at[q] < 0 or LC.needs(words[at[q]]) > T
        order = LC.rank(score_all[b], case["n"])                   # the ranking is checked on the host form's own scores: ties are exact
        assert index[b, :len(order)].tolist() == [int(at[q]) for q in order]
        assert (index[b, len(order):] == -1).all() and (score[b, len(order):] == -np.inf).all()
        assert score[b, :len(order)].tolist() == [score_all[b, q] for q in order]
    return case, (index, score, score_all, path, prob)


# ---- 1. the host form against torch ctc_loss -------------------------------------------------------------------------------------
def test_all_pairs_against_ctc_loss():
    case, (_, _, score_all, _, _) = check_host_against_reference("all_pairs", LC.all_pairs)
    words = LC.unpack(case["tokens"], case["lens"])
    assert {len(w) for w in words} >= set(range(7)) and (score_all == -np.inf).any()          # L = 0 .. 6 and infeasible words
    assert sum(LC.needs(w) > len(w) for w in words) >= 5                                       # repeats


@pytest.mark.parametrize("L,T", LC.STATE_EDGE)
def test_state_edge_against_ctc_loss(L, T):
    case, (_, _, score_all, _, _) = check_host_against_reference("state_edge", LC.state_edge, L, T)
    if T == "tight" and L >= 2:
        assert (score_all[:, 2] == -np.inf).all() and (score_all[:, 1] > -np.inf).all()       # L equal classes do not fit, L + r do


@pytest.mark.parametrize("T", [1, 2, 512])
def test_frames_against_ctc_loss(T):
    check_host_against_reference("frames", LC.frames, T)


@pytest.mark.parametrize("C", [2, 65535])
def test_classes_against_ctc_loss(C):
    check_host_against_reference("classes", LC.classes, C)


@pytest.mark.parametrize("N,B", LC.TAILS)
def test_tails_against_ctc_loss(N, B):
    check_host_against_reference("tails", LC.tails, N, B)


def test_candidate_lists_equal_the_gathered_full_scoring():
    from mrn_amd.modules.decoding import ctc_lexicon_host
    case, (index, score, score_all, _, prob) = check_host_against_reference("candidates", LC.candidates)
    full = ctc_lexicon_host(case["x"], case["tokens"], case["lens"], 4)[2]
    cand = case["cand"]
    gathered = np.where(cand >= 0, np.take_along_axis(full, np.maximum(cand, 0), axis=1), -np.inf)
    assert score_all.tobytes() == gathered.tobytes()
    assert index[0, :2].tolist() != [7, 7] or score[0, 0] == score[0, 1]          # a word named twice: both slots, equal scores
    assert (index[3] == -1).all() and prob[3, 0] == 0                              # a row of unused slots
    assert (index[2] == 11).all() or score_all[2, 0] == -np.inf                    # a row of one word fills every entry with it


# ---- 2. ties, dead slots, non-finite logits --------------------------------------------------------------------------------------
def test_ties_and_dead_slots():
    case, (index, score, score_all, path, prob) = check_host_against_reference("ties", LC.ties)
    for b in range(3):
        assert score_all[b, 0] == score_all[b, 2] == score_all[b, 5] and score_all[b, 1] == score_all[b, 3]
        live = index[b][index[b] >= 0].tolist()
        assert len(live) == 6 and live.index(0) < live.index(2) < live.index(5) and live.index(1) < live.index(3)
        assert index[b, 6:].tolist() == [-1, -1] and (score[b, 6:] == -np.inf).all()
    case, (index, score, score_all, path, prob) = check_host_against_reference("all_dead", LC.all_dead)
    assert (index == -1).all() and (score == -np.inf).all() and (score_all == -np.inf).all()
    assert (path == 0).all() and (prob[:, 0] == 0).all() and (prob[:, 1:] == 1).all()


def test_non_finite_logits():
    case = LC.non_finite()
    index, score, score_all, path, prob = host(case)
    assert not np.isnan(score_all).any()
    clean = LC.reference_scores({**case, "x": case["x"][:1]})
    assert np.abs(score_all[0] - clean[0]).max() <= HOST_TOL
    for b in (1, 3, 4):                                              # a NaN, a +inf, a frame of -inf: the sample is dead, it alone
        assert (score_all[b] == -np.inf).all() and (index[b] == -1).all() and (path[b] == 0).all() and prob[b, 0] == 0
    words = LC.unpack(case["tokens"], case["lens"])
    for q, w in enumerate(words):                                    # class 3 at -inf: the words that need it are dead, the others live
        assert (score_all[2, q] == -np.inf) == (3 in w)
    assert 3 not in [c for i in index[2] if i >= 0 for c in words[i]]


# ---- 3. the agreement case: how many samples the GPU test may except ---------------------------------------------------------------
def test_agreement_case_has_few_narrow_margins():
    """tests/test_lexicon_gpu.py excepts the samples whose float64 top-2 margin is below 1e-3 from "the best index agrees", and may
    except 5 % at the most: the share is known here, on the same inputs, before any GPU run"""
    case = LC.agreement()
    index, score, _, _, _ = host(case)
    narrow = (score[:, 0] - score[:, 1]) < 1e-3
    assert narrow.mean() <= 0.05
    assert sum(int(index[b, 0]) == 31 * b for b in range(32)) >= 24           # the planted word is found: the ranking is not noise


# ---- 4. the hand-over ------------------------------------------------------------------------------------------------------------
def test_frame_path_of_the_best_word_collapses_back_to_it():
    conv = ctc_converter(33)
    for case in (LC.all_pairs(), LC.ties(), LC.state_edge(31, 65), LC.classes(2)):
        index, score, _, path, prob = host(case)
        words = LC.unpack(case["tokens"], case["lens"])
        T = case["x"].shape[1]
        assert path.dtype == np.int64 and prob.dtype == np.float32
        for b in range(len(index)):
            prev, got = 0, []
            for k in path[b]:
                if k != 0 and k != prev:
                    got.append(int(k))
                prev = k
            assert got == words[index[b, 0]]
            assert np.cumprod(prob[b])[-1] == np.float32(np.exp(score[b, 0])) and (prob[b, 1:] == 1).all()
        if case["x"].shape[2] <= 37:
            assert conv.decode(path, [T] * len(path)) == ["".join(conv.character[c] for c in words[i]) for i in index[:, 0]]


# ---- 5. encode_lexicon, lexicon_options, lexicon_supported -------------------------------------------------------------------------
def test_encode_lexicon():
    from mrn_amd.modules.decoding import encode_lexicon
    conv = ctc_converter(10)
    ch = [chr(0x4E00 + i) for i in range(10)]
    words = [ch[0] + ch[1], "x" + ch[0], ch[2], ch[0] + ch[1], "", ch[3] * 4 + " ", ch[4] + "?"]
    tokens, lengths, kept = encode_lexicon(conv, words)
    assert kept == [ch[0] + ch[1], ch[2], ch[0] + ch[1], "", ch[3] * 4 + " "]                  # order and duplicates kept
    assert tokens.dtype == np.int32 and lengths.dtype == np.int32 and tokens.shape == (5, 5) and lengths.tolist() == [2, 1, 2, 0, 5]
    assert tokens[0].tolist() == [conv.dict[ch[0]], conv.dict[ch[1]], 0, 0, 0] and tokens[4, 4] == conv.dict[" "]
    assert tokens[lengths[:, None] > np.arange(5)[None, :]].min() > conv.dict["[UNK]"]
    conv.dict["u"] = conv.dict["[UNK]"]                                                     # a character of the [UNK] class
    conv.dict["b"] = 0                                                                      # ... and one of the blank's
    assert encode_lexicon(conv, ["u" + ch[0], ch[0] + "b", ch[5]])[2] == [ch[5]]
    with pytest.raises(ValueError, match="lexicon"):
        encode_lexicon(conv, ["xyz", "u"])
    assert encode_lexicon(conv, [""])[0].shape == (1, 1)


def test_lexicon_options_and_limits():
    from mrn_amd.modules import decoding as D
    assert D.lexicon_options(types.SimpleNamespace()) == (None, 1)
    assert D.lexicon_options(types.SimpleNamespace(lexicon=None, lexicon_top_n=3)) == (None, 3)
    assert D.lexicon_options(types.SimpleNamespace(lexicon=("ab", "c"))) == (["ab", "c"], 1)
    for bad in (0, -1, 2.5, "8", True, None):
        with pytest.raises(ValueError, match="lexicon_top_n must be an integer >= 1"):
            D.lexicon_options(types.SimpleNamespace(lexicon=["a"], lexicon_top_n=bad))
    for bad in ("word", 5, ["a", 3], [b"a"]):
        with pytest.raises(ValueError, match="lexicon must be a sequence of words"):
            D.lexicon_options(types.SimpleNamespace(lexicon=bad))
    assert D.decode_options(types.SimpleNamespace(lexicon=["a"])) == ("greedy", 8, 15)        # the other options stay as they are
    assert D.attn_decode_options(types.SimpleNamespace(lexicon=["a"])) == ("greedy", 8)
    ok = dict(prediction="CTC", T=63, C=97, Lmax=25, N=1000, n=1)
    assert D.lexicon_supported(**ok)
    for key, inside, outside in (("T", 512, 513), ("T", 1, 0), ("C", 65535, 65536), ("C", 2, 1), ("Lmax", 31, 32), ("Lmax", 0, -1),
                                 ("N", 1 << 20, (1 << 20) + 1), ("N", 1, 0), ("n", 16, 17), ("n", 1, 0)):
        assert D.lexicon_supported(**{**ok, key: inside}), (key, inside)
        assert not D.lexicon_supported(**{**ok, key: outside}), (key, outside)
    assert not D.lexicon_supported(**{**ok, "prediction": "Attn"})
    case = LC.frames(2)
    long_word = np.arange(40, dtype=np.int32)[None, :] % 4 + 1                                # the host form has no such limits
    assert D.ctc_lexicon_host(np.zeros((1, 80, 5), np.float32), long_word, np.array([40]), 20)[0][0, 0] == 0
    for bad in (dict(x=case["x"][0]), dict(n=0), dict(lens=case["lens"][:-1]), dict(lens=case["lens"] + 3), dict(tokens=case["tokens"] + 4),
                dict(cand=np.full((2, 1), 9)), dict(cand=np.zeros((3, 1), np.int64))):
        a = {**case, **bad}
        with pytest.raises(ValueError, match="ctc_lexicon_host"):
            D.ctc_lexicon_host(a["x"], a["tokens"], a["lens"], a["n"], cand=a["cand"])


def test_entry_point_is_declared_exported_and_cited():
    """include/mrn_lexicon.h is parsed and bound like include/mrn_hip.h: the prototype there, the symbol in the library, the reference
    op site and the limits in its comment"""
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.LEXICON_HEADER_PATH)
    assert list(protos) == ["mrn_ctc_lexicon_decode_f32"]
    ret, argtypes, argnames = protos["mrn_ctc_lexicon_decode_f32"]
    assert ret == "int" and argnames == ["logits", "stride_b", "stride_t", "B", "T", "C", "lex_tokens", "Lmax", "lex_len", "N", "cand", "K",
                                         "n", "index", "score", "score_all", "path", "prob", "stream"]
    assert argtypes == ["const float*", "int64_t", "int64_t", "int", "int", "int", "const int32_t*", "int", "const int32_t*", "int",
                        "const int32_t*", "int", "int", "int32_t*", "float*", "float*", "int64_t*", "float*", "void*"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mrn_ctc_lexicon_decode_f32")
    for other in (_lib.HEADER_PATH, _lib.DECODE_HEADER_PATH, _lib.ATTN_BEAM_HEADER_PATH):
        assert not set(protos) & set(_lib.parse_header(other))
    bound = _lib.LIB.load().mrn_ctc_lexicon_decode_f32
    assert bound.restype is ctypes.c_int and len(bound.argtypes) == 19
    header = open(_lib.LEXICON_HEADER_PATH).read()
    comment = header[:header.index("int mrn_ctc_lexicon_decode_f32(")].rsplit("/*", 1)[1]
    assert "test.py:211-219" in comment and "1 <= T <= 512" in comment and "1 <= n <= 16" in comment


# ---- 6. validation() on CPU predictions --------------------------------------------------------------------------------------------
N_CHARS = 8


def cpu_validation_case():
    """two batches of hand-made CTC logits on the CPU (T = 10, 12 classes), their labels, a lexicon that holds some of them"""
    conv = ctc_converter(N_CHARS)
    chars = conv.character[4:]
    rng = np.random.default_rng(5100)
    labels = [["".join(chars[i] for i in rng.integers(0, N_CHARS, size=int(rng.integers(1, 5)))) for _ in range(4)] for _ in range(2)]
    logits = []
    for batch in labels:
        x = 1.5 * rng.standard_normal((4, 10, N_CHARS + 4)).astype(np.float32)
        for b, word in enumerate(batch):
            for t, c in enumerate(LC_path(conv, word)):
                x[b, t, c] += 3.0
        logits.append(torch.from_numpy(x))
    lexicon = [labels[0][0], labels[0][1], "??", labels[1][2], chars[0] * 2, chars[1] + chars[2], labels[0][0], ""]
    batches = [(torch.zeros(4, 4, 32, 64), batch) for batch in labels]
    opt = types.SimpleNamespace(Prediction="CTC", batch_max_length=25, NED=True)
    return conv, opt, batches, logits, lexicon


def LC_path(conv, word):
    from mrn_amd.modules.decoding import frame_path
    return frame_path([conv.dict[ch] for ch in word], 10)


def run_cpu_validation(opt, conv, batches, logits):
    from mrn_amd.test import validation
    calls = iter(logits)
    return validation(lambda image, *a, **k: {"predict": next(calls), "feature": None}, lambda preds, text, length: torch.tensor(0.25),
                      batches, conv, opt)


def expected_returns(conv, batches, pairs):
    """the unchanged scorer on the decoder's (path, prob) pairs: the reference's string loop, accumulated as validation() does"""
    from mrn_amd.test import _host_scores
    n_correct, norm_ed, n = 0, 0.0, 0
    for (_, labels), (path, prob) in zip(batches, pairs):
        strings = conv.decode(path, [path.shape[1]] * len(path))
        conf = []
        for term, correct, c in _host_scores(labels, strings, prob, False, True):
            norm_ed += term if term is not None else 0
            n_correct += bool(correct)
            conf.append(c)
        n += len(labels)
    return n_correct / n * 100, norm_ed / n * 100, strings, conf


def test_validation_on_cpu_predictions(monkeypatch):
    from mrn_amd import ops
    from mrn_amd.modules import decoding as D
    conv, opt, batches, logits, lexicon = cpu_validation_case()
    tokens, lengths, kept = D.encode_lexicon(conv, lexicon)
    assert len(kept) == len(lexicon) - 1
    pairs = [D.ctc_lexicon_host(x.numpy(), tokens, lengths, 1)[3:] for x in logits]
    acc, ned, strings, conf = expected_returns(conv, batches, pairs)
    assert set(strings) <= set(kept)
    res = run_cpu_validation(types.SimpleNamespace(**vars(opt), lexicon=lexicon), conv, batches, logits)
    assert (res[0], res[1], res[2], list(res[3]), res[4], res[5], res[7]) == (0.25, acc, ned, strings, conf, batches[-1][1], 8)
    top3 = run_cpu_validation(types.SimpleNamespace(**vars(opt), lexicon=tuple(lexicon), lexicon_top_n=3), conv, batches, logits)
    assert top3[:6] == res[:6]                                    # validation() scores the best entry, however many are ranked

    # without the key: best path, as before.  The arg-max pass is a kernel; a torch stand-in for it lets the rest run on the CPU
    def argmax_prob(x):
        p, i = torch.softmax(x, dim=-1).max(dim=-1)
        return i, p
    monkeypatch.setattr(ops, "argmax_prob_lastdim", argmax_prob)
    greedy_pairs = [tuple(t.numpy() for t in argmax_prob(x)) for x in logits]
    acc_g, ned_g, strings_g, conf_g = expected_returns(conv, batches, greedy_pairs)
    for o in (opt, types.SimpleNamespace(**vars(opt), lexicon=None), types.SimpleNamespace(**vars(opt), lexicon_top_n=4)):
        plain = run_cpu_validation(o, conv, batches, logits)
        assert (plain[0], plain[1], plain[2], list(plain[3]), plain[4], plain[7]) == (0.25, acc_g, ned_g, strings_g, conf_g, 8)
    assert strings_g != strings or conf_g != conf
    # with the beam decoder the key is an error that names both; a lexicon the converter cannot spell a word of is one, too
    with pytest.raises(ValueError, match="lexicon.*ctc_decode"):
        run_cpu_validation(types.SimpleNamespace(**vars(opt), lexicon=lexicon, ctc_decode="beam"), conv, batches, logits)
    with pytest.raises(ValueError, match="lexicon"):
        run_cpu_validation(types.SimpleNamespace(**vars(opt), lexicon=["??"]), conv, batches, logits)
