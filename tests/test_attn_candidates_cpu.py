"""Host side of exact candidate scoring on the attention head and of validation()'s per-image lexicons (no kernel is launched): the
option, the float64 form attn_candidates_host against two independent yardsticks (attn_lexicon_host at a width that prunes nothing,
and the log-softmax of the greedy logits), its conventions, the C ABI of include/mrn_attn_score.h, the LDS rule, validation() on CPU
tensors, and the cases tests/test_decode_attn_candidates_gpu.py scores: how many of their samples are decisive is a property of the float64
form alone."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.test_attn_beam_cpu import EOS, SOS, TOKEN_BAND, beam_fixture
from tests.test_attn_lexicon_cpu import as_arrays, draw_lexicon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE = ("mrn_attn_score_candidates_grouped_f32", "mrn_attn_score_candidates_x3_grouped")
# name: (B, T, D, C, S, K, seed0, generator weight scale).  Seeds and scales are chosen, as for BEAM_CASES, so that the float64 form
# alone leaves at most B // 4 samples whose two best scores are closer than three bands
CAND_CASES = {
    "k3": (5, 9, 256, 37, 6, 3, 300, 50.0),              # per = 4: four samples per workgroup, B ends inside one, ragged class tile
    "k16": (3, 31, 256, 97, 12, 16, 200, 100.0),          # one sample per workgroup, every row in use
    "k17": (3, 17, 256, 331, 8, 17, 500, 400.0),          # two slot blocks per sample, the second nearly empty
    "k50": (2, 17, 512, 1045, 8, 50, 1100, 400.0),        # four slot blocks, the last one ragged
    "c5374": (2, 127, 256, 5374, 4, 5, 200, 50.0),        # per = 8: two samples per workgroup
    "k1": (4, 9, 256, 37, 6, 1, 300, 50.0),               # per = 1: sixteen samples per workgroup
}
_REF = {}


def draw_candidates(B, C, S, K, seed0):
    """(words, cand int32 [B][K]): a table of distinct words of 0 .. S - 1 classes (draw_lexicon: one of exactly S - 1, the empty word),
    one word with a class >= C and one duplicate of word 1; every row holds distinct random words, then row 0 gets an unused slot, row
    1 % B the duplicate pair (words 1 and its copy: with K = 1 the copy alone), row 2 % B the word this head cannot spell"""
    rng = np.random.default_rng(seed0 + 11)
    words = list(dict.fromkeys(draw_lexicon(C, S, seed0, max(2 * K, 12), 0, True)))
    bad, copy = len(words), len(words) + 1
    words = words + [(4, C + 3)[:S - 1], words[1]]
    cand = np.stack([rng.permutation(bad)[:K] for _ in range(B)]).astype(np.int32)
    cand[0, K - 1] = -1
    cand[1 % B, 0] = copy
    if K > 1:
        cand[1 % B, 1] = 1
        cand[1 % B, 2:][cand[1 % B, 2:] == 1] = 0 if K < 3 or 0 not in cand[1 % B, 2:] else 2
    cand[2 % B, K // 2] = bad
    return words, cand


def cand_case(name):
    """(sd, Hb, words, tokens, lengths, cand, outputs of attn_candidates_host with logp) of a case, computed once and shared (never
    modified)"""
    if name not in _REF:
        from mrn_amd.modules import decoding
        B, T, D, C, S, K, seed0, scale = CAND_CASES[name]
        sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
        words, cand = draw_candidates(B, C, S, K, seed0)
        tokens, lengths = as_arrays(words)
        ref = decoding.attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, cand, min(K, 3), S - 1, want_logp=True)
        _REF[name] = (sd, Hb, words, tokens, lengths, cand, ref)
    return _REF[name]


def decisive_samples(words, cand, score_all):
    """samples whose two best scores differ by at least 3 (L + 1) TOKEN_BAND, L the longer of the two words (one live slot, or none: decisive)"""
    out = []
    for b in range(len(cand)):
        order = np.argsort(-score_all[b], kind="stable")[:2]
        if len(order) < 2 or not np.isfinite(score_all[b, order[1]]):
            out.append(True)
            continue
        L = max(len(words[cand[b, q]]) for q in order)
        out.append(score_all[b, order[0]] - score_all[b, order[1]] >= 3 * (L + 1) * TOKEN_BAND)
    return np.array(out)


def test_options_and_conflicts():
    from mrn_amd.modules import decoding as D
    fn = lambda labels: [["a"] for _ in labels]  # noqa: E731
    assert D.candidates_options(SimpleNamespace()) == (None, 1)
    assert D.candidates_options(SimpleNamespace(candidates=None, lexicon_top_n=3)) == (None, 3)
    assert D.candidates_options(SimpleNamespace(candidates=fn)) == (fn, 1)
    table = {"x": ["a", "b"]}
    assert D.candidates_options(SimpleNamespace(candidates=table, lexicon_top_n=np.int64(2))) == (table, 2)
    for bad in (["a"], "word", 7):
        with pytest.raises(ValueError, match="candidates must be a callable"):
            D.candidates_options(SimpleNamespace(candidates=bad))
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="lexicon_top_n"):
            D.candidates_options(SimpleNamespace(candidates=fn, lexicon_top_n=bad))
    for other, named in (({"lexicon": ["a"]}, "lexicon"), ({"attn_lexicon": ["a"]}, "attn_lexicon"), ({"ctc_decode": "beam"}, "ctc_decode='beam'"),
                         ({"attn_decode": "beam"}, "attn_decode='beam'")):
        with pytest.raises(ValueError, match="candidates and " + re.escape(named)):
            D.candidates_options(SimpleNamespace(candidates=fn, **other))
    # greedy spelled out, and the neighbours' None, are no conflict; the neighbours do not read the key
    assert D.candidates_options(SimpleNamespace(candidates=fn, ctc_decode="greedy", attn_decode="greedy", lexicon=None, attn_lexicon=None))[0] is fn
    assert D.lexicon_options(SimpleNamespace(candidates=fn)) == (None, 1) and D.attn_lexicon_options(SimpleNamespace(candidates=fn)) == (None, 8)
    # the lists of a batch
    assert D.candidate_lists(table, ["x", "x"]) == [["a", "b"], ["a", "b"]]
    assert D.candidate_lists(lambda labels: [(gt, gt + "s") for gt in labels], ["ab", "c"]) == [["ab", "abs"], ["c", "cs"]]
    with pytest.raises(ValueError, match="no word list for the label 'y'"):
        D.candidate_lists(table, ["x", "y"])
    with pytest.raises(ValueError, match="1 word lists for 2 labels"):
        D.candidate_lists(lambda labels: [["a"]], ["x", "y"])
    for bad in ("ab", 3):
        with pytest.raises(ValueError, match="sequence of str"):
            D.candidate_lists({"x": bad}, ["x"])
    with pytest.raises(ValueError, match="got an entry 3"):
        D.candidate_lists({"x": ["a", 3]}, ["x"])
    with pytest.raises(ValueError, match="attn_beam"):
        D.attn_candidates_request(object(), "Attn", False, 4)
    assert D.attn_candidates_request(None, "Attn", False, 4) is None and D.attn_candidates_request(object(), "CTC", False) is None


def test_candidate_table_is_the_union_and_rows_follow_the_lists():
    from mrn_amd.modules import decoding as D
    from mrn_amd.tools.utils import AttnLabelConverter, CTCLabelConverter
    lists = [["abc", "b", "ÄÖ"], ["b", "", "abcdefgh"], []]
    attn = D.CandidateTable(AttnLabelConverter("abcdefgh"), lists, True, 5)
    assert attn.words == ["abc", "b", ""]                                   # first occurrence, what cannot be spelled in 5 is dropped
    assert attn.rows(lists).tolist() == [[0, 1], [1, 2], [-1, -1]] and attn.rows(lists).dtype == np.int32
    assert attn.rows([[]]).tolist() == [[-1]]                               # K >= 1
    ctc = D.CandidateTable(CTCLabelConverter("abcdefgh"), lists, False, 5)
    assert ctc.words == ["abc", "b", "", "abcdefgh"]
    with pytest.raises(ValueError, match="none of the"):
        D.CandidateTable(AttnLabelConverter("abcdefgh"), [["xyz"]], True, 5)


def test_entry_points_are_declared_bound_exported_and_cited():
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.ATTN_SCORE_HEADER_PATH)
    assert tuple(protos) == SCORE
    others = [_lib.parse_header(), _lib.parse_header(_lib.DECODE_HEADER_PATH), _lib.parse_header(_lib.ATTN_BEAM_HEADER_PATH),
              _lib.parse_header(_lib.LEXICON_HEADER_PATH), _lib.parse_header(_lib.ATTN_LEXICON_HEADER_PATH)]
    assert not any(set(protos) & set(o) for o in others)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    loaded = _lib.LIB.load()
    header = open(_lib.ATTN_SCORE_HEADER_PATH).read()
    greedy = others[0]["mrn_attn_greedy_decode_x3_grouped"][2]
    for name in SCORE:
        ret, argtypes, argnames = protos[name]
        assert hasattr(dll, name) and name in _lib.LIB._protos
        bound = getattr(loaded, name)
        assert bound.restype is ctypes.c_int and len(bound.argtypes) == len(argnames)
        operands = [a for a in greedy[:greedy.index("num_class") + 1] if "x3" in name or a != "w_inv"]
        assert argnames[:len(operands)] == operands                # the operands of the grouped greedy entry points, in their order
        assert argnames[len(operands):] == ["eos", "lex_tokens", "Lmax", "lex_len", "N", "cand", "K", "score_all", "logp", "groups", "B", "T",
                                            "D", "S", "hidden", "stream"]
        assert [argtypes[argnames.index(a)] for a in ("lex_tokens", "lex_len", "cand")] == ["const int32_t*"] * 3
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "modules/prediction.py:70-86" in comment, name
        for limit in ("1 <= S <= 512", "2 <= num_class <= 65535", "hidden = 256", "1 <= N <= 2^20", "K >= 1",
                      "multiple of " + ("32" if "x3" in name else "16")):
            assert limit in comment, (name, limit)


def test_rule_matches_the_launch_helper():
    """ops.attn_score_whole_context restates the scorer's LDS sum in csrc/attn_decode.hip, and the limits stand before the first launch"""
    from mrn_amd import ops
    src = open(os.path.join(ROOT, "mrn_amd", "csrc", "attn_decode.hip")).read()
    consts = dict(re.findall(r"(?m)^constexpr int (\w+) = ([^;]+);", src))
    assert re.sub(r"\s+", " ", consts["SCORE_LDS_EXTRA"]).strip() == "4 * (5 * BT + 2 * NW * BT)"
    assert ops.ATTN_SCORE_LDS_EXTRA == 4 * (5 * 16 + 2 * 16 * 16) == 2368
    launch = re.sub(r"\s+", " ", src[src.index("static int score_launch("):src.index("static int score_grouped(")])
    assert "lds = attn_tile_lds(x3, D, T, SCORE_LDS_EXTRA)" in launch and "CTX_CHUNK" not in launch
    body = re.sub(r"\s+", " ", src[src.index("static int score_grouped("):src.index("MRN_EXPORT int mrn_attn_score_candidates_grouped_f32")])
    for check in ("attn_tile_lds(x3, D, T, SCORE_LDS_EXTRA) <= 160 * 1024", "S >= 1 && S <= 512", "N >= 1 && N <= (1 << 20)", "K >= 1 && cand",
                  "o.num_class[g] >= 2 && o.num_class[g] <= 65535", "eos >= 0 && eos < o.num_class[g]"):
        assert check in body and body.index(check) < body.index("score_launch("), check
    # the step is the greedy kernel's: the shared device functions, no copy of them
    kernel = src[src.index("void attn_score_kernel("):src.index("}  // namespace")]
    assert "attn_scores<X3, false>(v, p, step);" in kernel and "attn_cell<X3, false, false>(v, p, step, acc5, c, h, act);" in kernel
    assert "generator_tiles<X3>(v, gp, r_gen, inv_gen," in kernel and "gp.logits" not in kernel
    for T in (17, 65, 129):
        for x3 in (True, False):
            for D in list(range(32, 2600, 32)) + [48, 264]:
                lds = 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + (1024 if x3 else 0) + 2368
                assert ops.attn_score_whole_context(D, T, x3) == (lds <= 160 * 1024 and D % (32 if x3 else 16) == 0), (D, T, x3)
    assert ops.attn_score_whole_context(1792, 65, True) and not ops.attn_score_whole_context(2304, 65, True)
    edge = max(D for D in range(32, 2600, 32) if ops.attn_score_whole_context(D, 65, True))
    assert ops.attn_score_whole_context(edge, 65, True) and not ops.attn_score_whole_context(edge + 32, 65, True)


def test_host_form_is_the_lexicon_search_without_pruning():
    """for N distinct words attn_lexicon_host at width >= N returns every word's exact score: an independent route (a trie walk with a
    selection per step) to the same numbers.  Scores to 1e-10, the best word the same"""
    from mrn_amd.modules import decoding as D
    B, T, Dm, C, S = 4, 9, 256, 37, 6
    sd, Hb = beam_fixture(B, T, Dm, C, 300, 50.0)
    words = list(dict.fromkeys(draw_lexicon(C, S, 300, 12, 0, True)))
    N = len(words)
    assert 8 <= N <= 16 and () in words and max(map(len, words)) == S - 1
    tokens, lengths = as_arrays(words)
    cand = np.tile(np.arange(N, dtype=np.int32), (B, 1))
    index, score, score_all, path, prob, logp = D.attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, cand, N, S - 1, want_logp=True)
    ref = D.attn_lexicon_host(sd, Hb, SOS, EOS, 16, S - 1, D.build_trie(tokens, lengths))
    assert index.dtype == np.int32 and index.shape == (B, N) and score_all.shape == (B, N) and path.dtype == np.int64 and prob.dtype == np.float32
    for b in range(B):
        want = {int(w): s for w, s in zip(ref[6][b], ref[2][b]) if w >= 0}
        assert set(want) == set(range(N))
        for i in range(N):
            assert abs(score_all[b, i] - want[i]) <= 1e-10, (b, i)
            assert abs(logp[b, i].sum() - score_all[b, i]) <= 1e-12 and np.all(logp[b, i, lengths[i] + 1:] == 0)
        assert index[b, 0] == ref[6][b, 0] and np.array_equal(path[b], ref[4][b])
        np.testing.assert_allclose(prob[b], ref[5][b], rtol=1e-6)
        assert np.array_equal(index[b], np.argsort(-score_all[b], kind="stable")) and np.array_equal(score[b], score_all[b, index[b]])


def test_the_greedy_decode_scores_as_the_log_softmax_of_the_greedy_logits():
    """the sample's greedy decode as its one candidate: the score is the sum, up to the first eos, of the float64 log-softmax of the
    greedy logits at the chosen tokens -- computed here directly, step by step, without the candidate code"""
    from mrn_amd.modules import decoding as D
    B, T, Dm, C, S = 4, 9, 256, 37, 6
    sd, Hb = beam_fixture(B, T, Dm, C, 300, 50.0)
    w = {k: v.double().numpy() for k, v in sd.items()}
    a = "attention_cell."
    H = Hb.double().numpy()
    words, want = [], []
    for b in range(B):
        h, c, tok, total, word = np.zeros(256), np.zeros(256), SOS, 0.0, []
        for s in range(S):
            e = np.tanh(H[b] @ w[a + "i2h.weight"].T + h @ w[a + "h2h.weight"].T + w[a + "h2h.bias"]) @ w[a + "score.weight"][0]
            alpha = np.exp(e - e.max()) / np.exp(e - e.max()).sum()
            g = (np.concatenate([alpha @ H[b], w["char_embeddings.weight"][tok]]) @ w[a + "rnn.weight_ih"].T + w[a + "rnn.bias_ih"]
                 + h @ w[a + "rnn.weight_hh"].T + w[a + "rnn.bias_hh"])
            gi, gf, gg, go = np.split(g, 4)
            sig = lambda x: 1.0 / (1.0 + np.exp(-x))  # noqa: E731
            c = sig(gf) * c + sig(gi) * np.tanh(gg)
            h = sig(go) * np.tanh(c)
            x = h @ w["generator.weight"].T + w["generator.bias"]
            tok = int(x.argmax())
            total += x[tok] - (x.max() + np.log(np.exp(x - x.max()).sum()))
            if tok == EOS:
                break
            word.append(tok)
        if tok != EOS:                      # never finished within S steps: no word of S - 1 classes spells it; take the prefix's score apart
            word, total = None, None
        words.append(word)
        want.append(total)
    kept = [b for b in range(B) if words[b] is not None]
    assert kept, "the fixture's greedy decodes must end within S steps for at least one sample"
    tokens, lengths = as_arrays([tuple(words[b]) for b in kept])
    cand = np.full((B, 1), -1, dtype=np.int32)
    cand[kept, 0] = np.arange(len(kept))
    index, score, score_all, path, prob = D.attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, cand, 1, S - 1)
    for k, b in enumerate(kept):
        assert abs(score_all[b, 0] - want[b]) <= 1e-10 and index[b, 0] == k
        assert path[b].tolist() == words[b] + [EOS] * (S - len(words[b]))
    for b in set(range(B)) - set(kept):
        assert index[b, 0] == -1 and np.isneginf(score_all[b, 0]) and np.all(path[b] == EOS) and np.all(prob[b] == 0)


def test_conventions():
    """the empty word, an unused slot, a class the head lacks, duplicates tie to the lower slot, a sample without a live slot, n > K"""
    from mrn_amd.modules import decoding as D
    B, T, Dm, C, S = 3, 9, 256, 37, 6
    sd, Hb = beam_fixture(B, T, Dm, C, 300, 50.0)
    words = [(5, 6), (), (5, 40), (5, 6), (7,)]
    tokens, lengths = as_arrays(words)
    cand = np.int32([[3, 0, 1, -1, 2], [2, -1, -1, -1, -1], [4, 4, 1, 0, 3]])
    index, score, score_all, path, prob, logp = D.attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, cand, 7, S - 1, want_logp=True)
    assert index.shape == (B, 7) and score.shape == (B, 7) and score_all.shape == (B, 5) and logp.shape == (B, 5, S)
    assert np.isneginf(score_all[0, 3]) and np.isneginf(score_all[0, 4]) and np.all(np.isfinite(score_all[0, :3]))
    assert score_all[0, 0] == score_all[0, 1]                                   # words 3 and 0 spell the same
    order = index[0, :3].tolist()
    assert order.index(3) < order.index(0) and np.all(index[0, 3:] == -1) and np.all(np.isneginf(score[0, 3:]))      # the lower slot first
    assert np.all(logp[0, 3:] == 0) and np.all(logp[0, 2, 1:] == 0) and logp[0, 2, 0] == score_all[0, 2]              # the empty word: eos alone
    assert np.all(index[1] == -1) and np.all(np.isneginf(score_all[1])) and np.all(path[1] == EOS) and np.all(prob[1] == 0)
    assert score_all[2, 0] == score_all[2, 1] and score_all[2, 3] == score_all[2, 4]
    rank = index[2].tolist()
    assert rank.index(0) < rank.index(3) and sorted(rank[:5]) == [0, 1, 3, 4, 4]
    best = int(np.argmax(score_all[0]))
    L = len(words[cand[0, best]])
    assert path[0].tolist() == list(words[cand[0, best]]) + [EOS] * (S - L) and np.all(prob[0, L + 1:] == 1.0)
    np.testing.assert_allclose(prob[0, :L + 1], np.exp(logp[0, best, :L + 1]), rtol=1e-6)
    # a permuted row gives the permuted scores, bit for bit
    perm = np.random.default_rng(1).permutation(5)
    again = D.attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, cand[:, perm], 7, S - 1)
    assert np.array_equal(again[2], score_all[:, perm])
    # what the host check refuses
    for bad, msg in ((dict(cand=np.int32([[5]] * B)), "candidate index"), (dict(cand=np.int32([[-2]] * B)), "candidate index"),
                     (dict(cand=np.zeros((B, 0), np.int32)), "K >= 1"), (dict(cand=cand[:2]), "cand"),
                     (dict(lengths=np.int32([2, 0, 2, 2, 6])), "word lengths"), (dict(tokens=-tokens), "negative class")):
        kw = dict(tokens=tokens, lengths=lengths, cand=cand)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            D.attn_candidates_host(sd, Hb, SOS, EOS, kw["tokens"], kw["lengths"], kw["cand"], 1, S - 1)
    with pytest.raises(ValueError, match="word lengths"):
        D.attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, cand, 1, 1)      # a word of two classes needs S >= 3


def test_gpu_cases_hold_what_they_must_and_are_decisive_enough():
    for name, (B, T, Dm, C, S, K, _, _) in CAND_CASES.items():
        sd, Hb, words, tokens, lengths, cand, ref = cand_case(name)
        index, score, score_all, path, prob, logp = ref
        used = cand[cand >= 0]
        assert cand.shape == (B, K) and (cand == -1).any() and any(max(words[w], default=0) >= C for w in used), name
        assert {len(w) for w in words} >= {0, S - 1}
        spelled = [[words[w] for w in row if w >= 0] for row in cand]
        assert any(len(set(r)) < len(r) for r in spelled) or K == 1, name          # a duplicate pair inside a row
        assert len(set(words)) < len(words)
        dead = (cand < 0) | np.array([[w >= 0 and max(words[w], default=0) >= C for w in row] for row in cand])
        assert np.array_equal(np.isneginf(score_all), dead), name
        loose = int((~decisive_samples(words, cand, score_all)).sum())
        print(f"{name}: {loose} of {B} samples are not decisive (cap {B // 4})")
        assert loose <= B // 4, name


# ---- validation() on CPU tensors ---------------------------------------------------------------------------------------------------
CHARS = "abcdefgh"
LABELS = ["abc", "b", "hg", "deaf"]
LISTS = {"abc": ["abd", "abc", "ÄÖ", "ab"], "b": ["b", "d", "bb"], "hg": ["gh", "hg", "h", ""], "deaf": ["dead", "deaf", "deafabcdefgh"]}


class TinyCTC(nn.Module):
    """`image` [B,T,C] is the logits"""

    def __init__(self):
        super().__init__()
        self.p = nn.Parameter(torch.zeros(1))

    def forward(self, image, is_train=False, **kw):
        return {"predict": image}


def ctc_logits(conv, labels, T, noise_seed):
    """logits whose best path spells the label: 6 on the path's class, noise below 1 elsewhere"""
    from mrn_amd.modules.decoding import frame_path
    C = len(conv.character)
    x = torch.rand(len(labels), T, C, generator=torch.Generator().manual_seed(noise_seed))
    for b, gt in enumerate(labels):
        for t, k in enumerate(frame_path([conv.dict[ch] for ch in gt], T)):
            x[b, t, k] += 6.0
    return x


def run_validation(model, batches, conv, prediction, **keys):
    from mrn_amd.test import validation
    opt = SimpleNamespace(Prediction=prediction, batch_max_length=7, NED=True, **keys)
    with torch.no_grad():
        res = validation(model, lambda preds, li, ll: torch.zeros(()), batches, conv, opt)
    return res[:6] + res[7:]


@pytest.mark.parametrize("form", ["dict", "callable"])
def test_validation_on_a_ctc_head(form):
    """CPU tensors: the host form with a candidate table.  Lists that hold the label leave a model that reads the label right at 100 %;
    lists without it give the list's best word, as ctc_lexicon_host ranks it"""
    from mrn_amd.modules import decoding as D
    from mrn_amd.tools.utils import CTCLabelConverter
    conv = CTCLabelConverter(CHARS)
    x = ctc_logits(conv, LABELS, 9, 5)
    batches = [(x[:3], LABELS[:3]), (x[3:], LABELS[3:])]
    cands = LISTS if form == "dict" else (lambda labels: [LISTS[gt] for gt in labels])
    got = run_validation(TinyCTC(), batches, conv, "CTC", candidates=cands)      # (the default decode of CPU logits needs the device)
    assert got[1] == 100.0 and got[2] == 100.0 and got[3] == ["deaf"] and got[5] == ["deaf"] and got[6] == 4
    without = {gt: [w for w in ws if w != gt] for gt, ws in LISTS.items()}
    miss = run_validation(TinyCTC(), batches, conv, "CTC", candidates=without, lexicon_top_n=2)
    table = D.CandidateTable(conv, [without[gt] for gt in LABELS], False, 7)
    ref = D.ctc_lexicon_host(x.numpy(), table.tokens, table.lengths, 2, table.rows([without[gt] for gt in LABELS]))
    assert miss[1] == 0.0 and miss[3] == [table.words[ref[0][3, 0]]] and miss[3][0] in without["deaf"]
    assert abs(miss[4][0] - float(np.exp(ref[1][3, 0]))) <= 1e-6 * float(np.exp(ref[1][3, 0]))
    with pytest.raises(ValueError, match="no word list for the label"):
        run_validation(TinyCTC(), batches, conv, "CTC", candidates={"abc": ["abc"]})
    with pytest.raises(ValueError, match="candidates and lexicon"):
        run_validation(TinyCTC(), batches, conv, "CTC", candidates=cands, lexicon=["abc"])


class TinyAttn(nn.Module):
    """`image` [B,T,D] is the features: the greedy logits come from the oracle's loop, the candidate pair from Attention.score_candidates
    on CPU tensors (the float64 host form)"""

    def __init__(self, att):
        super().__init__()
        self.att = att
        self.calls = []

    def forward(self, image, text=None, is_train=False, attn_candidates=None, **kw):
        from mrn_amd.modules.decoding import ATTN_EOS
        from oracle import mrn_oracle as O
        sd = self.att.state_dict()
        osd = {"P." + k: v for k, v in sd.items()}
        out = {"predict": O.attention_forward(osd, "P.", image, text, False, 7, sd["generator.weight"], sd["generator.bias"])}
        self.calls.append(attn_candidates)
        if attn_candidates is not None:
            res = self.att.score_candidates(image, text, ATTN_EOS, attn_candidates, 7)
            out["beam_path"], out["beam_prob"], out["beam_word"] = res[3], res[4], res[0][:, 0]
        return out


@pytest.mark.parametrize("form", ["dict", "callable"])
def test_validation_on_an_attention_head(form):
    """CPU tensors: every prediction is the word of its own list with the largest float64 score, its confidence that word's
    probability; the table is uploaded once, cand goes per batch; candidates=None is the call without the option"""
    from mrn_amd import ops
    from mrn_amd.modules import decoding as D
    from mrn_amd.modules.prediction import Attention
    from mrn_amd.tools.utils import AttnLabelConverter
    conv = AttnLabelConverter(CHARS)
    C = len(conv.character)
    sd, Hb = beam_fixture(len(LABELS), 9, 256, C, 300, 50.0)
    att = Attention(256, 256, C, nn.Linear(256, C))
    att.load_state_dict(sd)
    batches = [(Hb[:3], LABELS[:3]), (Hb[3:], LABELS[3:])]
    cands = LISTS if form == "dict" else (lambda labels: [LISTS[gt] for gt in labels])
    model = TinyAttn(att)
    got = run_validation(model, batches, conv, "Attn", candidates=cands, lexicon_top_n=2)
    assert all(isinstance(h, ops.CandidateHandle) for h in model.calls) and [h.cand.shape[0] for h in model.calls] == [3, 1]
    assert model.calls[0].tokens is model.calls[1].tokens and model.calls[0].n == 2
    lists = [LISTS[gt] for gt in LABELS]
    table = D.CandidateTable(conv, lists, True, 7)
    assert "ÄÖ" not in table.words and "deafabcdefgh" not in table.words and "" in table.words
    ref = D.attn_candidates_host(sd, Hb, conv.dict["[SOS]"], D.ATTN_EOS, table.tokens, table.lengths, table.rows(lists), 2, 7, want_logp=True)
    best = [table.words[i] for i in ref[0][:, 0]]
    assert all(w in lst for w, lst in zip(best, lists))
    assert got[1] == 100.0 * sum(w == gt for w, gt in zip(best, LABELS)) / len(LABELS)
    assert got[3] == [best[3] + "[EOS]" * (8 - len(best[3]))]
    want = float(np.cumprod(ref[4][3][:len(best[3])])[-1]) if best[3] else 0
    assert abs(got[4][0] - want) <= 1e-6 * want
    with pytest.raises(ValueError, match="candidates and attn_decode='beam'"):
        run_validation(model, batches, conv, "Attn", candidates=cands, attn_decode="beam")
    with pytest.raises(ValueError, match="candidates and attn_lexicon"):
        run_validation(model, batches, conv, "Attn", candidates=cands, attn_lexicon=["abc"])
    # a handle without a batch's table, and a table of another batch size, are refused
    with pytest.raises(ValueError, match="with_cand"):
        att.score_candidates(Hb, 2, D.ATTN_EOS, ops.upload_words(table.tokens, table.lengths, "cpu"), 7)
    with pytest.raises(ValueError, match="candidate rows"):
        att.score_candidates(Hb[:2], 2, D.ATTN_EOS, model.calls[0], 7)
