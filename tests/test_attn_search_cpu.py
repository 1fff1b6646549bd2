"""decoding.attn_search_request resolves the four keywords of an evaluation forward (attn_beam, attn_lexicon, attn_candidates,
attn_shortlist) into one AttnSearch record.  It must return or raise exactly what the four *_request functions, composed in the order
Model.heads called them in before the record existed, return or raise: the same exception type and text, or a record whose members are
their four results.  best_of picks (path, prob, word) out of a search's output tuple for any number of leading dimensions."""
import itertools

import numpy as np
import pytest
import torch

from mrn_amd.modules import decoding as D

TRIE, CANDS, WORDS = object(), object(), object()       # the request functions pass handles through unlooked-at
SET = {"attn_beam": 4, "attn_lexicon": TRIE, "attn_candidates": CANDS, "attn_shortlist": (WORDS, 3, 1)}
KEYS = tuple(SET)


def composed(prediction, is_train, attn_beam=None, attn_lexicon=None, attn_candidates=None, attn_shortlist=None):
    """the four functions as Model.heads composed them -> (width, trie, cands, short)"""
    width = D.attn_beam_request(attn_beam, prediction, is_train)
    trie = D.attn_lexicon_request(attn_lexicon, attn_beam)
    cands = D.attn_candidates_request(attn_candidates, prediction, is_train, attn_beam)
    short = D.attn_shortlist_request(attn_shortlist, prediction, is_train, attn_beam, attn_candidates)
    return width, trie, cands, short


def outcome(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except Exception as e:      # noqa: BLE001  (the type is part of what is compared)
        return type(e), str(e)


def check(prediction, is_train, grad, kw):
    with torch.set_grad_enabled(grad):
        want = outcome(composed, prediction, is_train, **kw)
        got = outcome(D.attn_search_request, prediction, is_train, **kw)
    if isinstance(want[0], type):
        assert got == want, (prediction, is_train, grad, kw)
        return "error"
    width, trie, cands, short = want
    if short is not None:
        assert got == D.AttnSearch("shortlist", words=short[0], K=short[1], max_dist=short[2]) and got.has_word
    elif cands is not None:
        assert got == D.AttnSearch("candidates", cands=cands) and got.has_word
    elif width is not None and trie is not None:
        assert got == D.AttnSearch("lexicon", width=width, trie=trie) and got.has_word
    elif width is not None:
        assert got == D.AttnSearch("beam", width=width) and not got.has_word
    else:
        assert got is None
    return None if got is None else got.kind


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("is_train", [False, True])
@pytest.mark.parametrize("prediction", ["CTC", "Attn"])
def test_every_combination_of_the_keywords(prediction, is_train, grad):
    seen = []
    for chosen in itertools.product([False, True], repeat=len(KEYS)):
        kw = {k: SET[k] for k, on in zip(KEYS, chosen) if on}
        seen.append(check(prediction, is_train, grad, kw))
    assert seen.count("error") == 11                 # a lexicon without a width (4), two replacements of greedy at once (7): whatever the head
    if prediction == "Attn" and not is_train and not grad:
        assert {k for k in seen if k not in (None, "error")} == set(D.ATTN_SEARCHES)
    else:
        assert {k for k in seen if k != "error"} == {None}


@pytest.mark.parametrize("kw", [{"attn_beam": 0}, {"attn_beam": True}, {"attn_beam": 2.0}, {"attn_shortlist": WORDS},
                                {"attn_shortlist": (WORDS, 0, None)}, {"attn_shortlist": (WORDS, 3, -1)},
                                {"attn_beam": 0, "attn_lexicon": TRIE}, {"attn_beam": 0, "attn_candidates": CANDS}])
def test_malformed_values(kw):
    for prediction, is_train, grad in itertools.product(["CTC", "Attn"], [False, True], [False, True]):
        check(prediction, is_train, grad, kw)
    assert check("Attn", False, False, kw) == "error"


def test_a_shortlist_request_becomes_the_candidates_request_that_scores_its_table():
    from mrn_amd import ops
    tokens, lengths = np.array([[5, 6], [7, 0]], dtype=np.int32), np.array([2, 1], dtype=np.int32)
    words = ops.upload_words(tokens, lengths, "cpu", 2)
    with torch.no_grad():
        req = D.attn_search_request("Attn", False, attn_shortlist=(words, 2, None))
    cand = np.array([[1, 0], [0, -1], [-1, -1]], dtype=np.int32)
    scoring = req.scoring(cand, 4)
    assert scoring.kind == "candidates" and scoring.has_word and scoring[1:3] == (None, None) and scoring[4:] == (None, None, None)
    assert isinstance(scoring.cands, ops.CandidateHandle) and np.array_equal(scoring.cands.cand, cand) and scoring.cands.n == 2
    assert scoring.cands.tokens is words.tokens and req.words is words and words.cand is None


@pytest.mark.parametrize("lead", [(3,), (2, 3), (2, 2, 3)])
def test_best_of_reads_the_documented_positions(lead):
    """element i of a fabricated output tuple holds i + 10 * (index along its last axis): distinct markers everywhere"""
    res = tuple(np.broadcast_to(i + 10 * np.arange(4), lead + (4,)).copy() for i in range(8))
    where = {"beam": (4, 5, None), "lexicon": (4, 5, 6), "candidates": (3, 4, 0), "shortlist": (3, 4, 0)}
    assert set(where) == set(D.ATTN_SEARCHES)
    for kind, (p, q, w) in where.items():
        path, prob, word = D.best_of(kind, res)
        assert path is res[p] and prob is res[q]
        if w is None:
            assert word is None
        else:
            assert word.shape == lead and np.all(word == w)
    torch_res = tuple(torch.from_numpy(r) for r in res)
    assert torch.equal(D.best_of("lexicon", torch_res)[2], torch.full(lead, 6))
