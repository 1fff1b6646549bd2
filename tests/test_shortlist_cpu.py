"""Lexicon shortlists by edit distance (mrn_lexicon_shortlist_i32, csrc/lexicon_shortlist.hip): what can be checked without a GPU.  The
options, the numpy host form mrn_amd/modules/decoding.py::lexicon_shortlist_host against a plain dynamic programme, the header, the
errors of the combinations, and the protocol's one property: the shortlist only orders the candidates, so with K >= N and no cut-off
the shortlist decoder's best word is the exact arg-max over the lexicon."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import EOS, SOS, beam_fixture
from tests.test_attn_lexicon_cpu import LEXICON_CASES, as_arrays, draw_lexicon

SHORTLIST = ("mrn_lexicon_shortlist_work_bytes", "mrn_lexicon_shortlist_i32")


def levenshtein(a, b):
    """the O(L * H) table, row by row"""
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        table[i][0] = i
    for j in range(len(b) + 1):
        table[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            table[i][j] = min(table[i - 1][j] + 1, table[i][j - 1] + 1, table[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return table[len(a)][len(b)]


def shortlist_by_definition(hyps, words, K, max_dist):
    """(cand, dist) of the definition: the words in range ranked by (d, w), the first K, -1 behind"""
    cand = np.full((len(hyps), K), -1, dtype=np.int32)
    dist = np.full((len(hyps), K), -1, dtype=np.int32)
    for b, h in enumerate(hyps):
        d = [levenshtein(h, w) for w in words]
        order = sorted((w for w in range(len(words)) if max_dist is None or d[w] <= max_dist), key=lambda w: (d[w], w))[:K]
        cand[b, :len(order)] = order
        dist[b, :len(order)] = [d[w] for w in order]
    return cand, dist


def hyp_arrays(hyps, Hmax=None, junk=0):
    """hypotheses as (hyp [B][Hmax], hyp_len [B]); `junk` fills the places behind a hypothesis, which nobody may read"""
    Hmax = max([len(h) for h in hyps] + [1]) if Hmax is None else Hmax
    hyp = np.full((len(hyps), Hmax), junk, dtype=np.int32)
    for b, h in enumerate(hyps):
        hyp[b, :len(h)] = h
    return hyp, np.array([len(h) for h in hyps], dtype=np.int32)


def perturbed(rng, word, C, edits):
    """a word after `edits` random substitutions, insertions and deletions of classes 4 ... C - 1"""
    w = list(word)
    for _ in range(edits):
        kind = rng.integers(3)
        at = int(rng.integers(len(w) + 1))
        if kind == 0 and w:
            w[min(at, len(w) - 1)] = int(rng.integers(4, C))
        elif kind == 1:
            w.insert(at, int(rng.integers(4, C)))
        elif w:
            del w[min(at, len(w) - 1)]
    return tuple(w)


def test_options():
    from mrn_amd.modules.decoding import shortlist_options
    assert shortlist_options(SimpleNamespace()) == (None, None)
    assert shortlist_options(SimpleNamespace(lexicon_shortlist=None, lexicon_max_distance=None)) == (None, None)
    assert shortlist_options(SimpleNamespace(lexicon_shortlist=50)) == (50, None)
    assert shortlist_options(SimpleNamespace(lexicon_shortlist=np.int64(1), lexicon_max_distance=0)) == (1, 0)
    assert shortlist_options(SimpleNamespace(lexicon_max_distance=3)) == (None, 3)
    for bad in (0, -1, True, 2.5, "3", [3]):
        with pytest.raises(ValueError, match="lexicon_shortlist"):
            shortlist_options(SimpleNamespace(lexicon_shortlist=bad))
    for bad in (-1, False, 1.0, "1"):
        with pytest.raises(ValueError, match="lexicon_max_distance"):
            shortlist_options(SimpleNamespace(lexicon_shortlist=3, lexicon_max_distance=bad))


@pytest.mark.parametrize("name", ["c37_w3", "few_w8", "c97_w4"])
def test_host_form_is_the_definition(name):
    from mrn_amd.modules.decoding import lexicon_shortlist_host
    B, T, D, C, S, W, seed0, scale, n, shortest, empty = LEXICON_CASES[name]
    words = draw_lexicon(C, S, seed0, n, shortest, empty)
    tokens, lengths = as_arrays(words)
    rng = np.random.default_rng(seed0)
    hyps = [perturbed(rng, words[int(rng.integers(len(words)))], C, int(rng.integers(0, 4))) for _ in range(5)]
    hyps += [(), (C + 5,), tuple(int(c) for c in rng.integers(4, C, 70)), words[-1]]       # empty, a class of no word, longer than 64, a duplicate
    hyp, hyp_len = hyp_arrays(hyps, junk=4)
    N = len(words)
    for K, max_dist in ((1, None), (7, None), (N, None), (N + 3, None), (5, 0), (5, 2), (N, 3)):
        cand, dist = lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, K, max_dist)
        r_cand, r_dist = shortlist_by_definition(hyps, words, K, max_dist)
        assert cand.dtype == np.int32 and dist.dtype == np.int32 and cand.shape == (len(hyps), K)
        assert np.array_equal(cand, r_cand) and np.array_equal(dist, r_dist), (name, K, max_dist)
    # a length is clipped to 0 .. Hmax; bad operands are refused
    clipped = lexicon_shortlist_host(hyp, np.where(np.arange(len(hyps)) % 2 == 0, -3, 1000), tokens, lengths, 4)
    want = lexicon_shortlist_host(hyp, np.where(np.arange(len(hyps)) % 2 == 0, 0, hyp.shape[1]), tokens, lengths, 4)
    assert np.array_equal(clipped[0], want[0]) and np.array_equal(clipped[1], want[1])
    with pytest.raises(ValueError, match="K >= 1"):
        lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, 0)
    with pytest.raises(ValueError, match="max_dist"):
        lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, 3, -1)
    with pytest.raises(ValueError, match="word lengths"):
        lexicon_shortlist_host(hyp, hyp_len, tokens, lengths + tokens.shape[1], 3)


def test_hypotheses_of_the_two_heads():
    from mrn_amd import ops
    from mrn_amd.modules.decoding import hypothesis_of_frames, hypothesis_of_path
    path = np.array([[5, 6, 3, 7, 3], [3, 5, 5, 5, 5], [5, 6, 7, 8, 9]])
    hyp, n = hypothesis_of_path(path, 3)
    assert n.tolist() == [2, 0, 5] and hyp.dtype == np.int32 and np.array_equal(hyp, path)
    t_hyp, t_n = ops.hypothesis_of_path(torch.from_numpy(path), 3)
    assert np.array_equal(t_hyp.numpy(), hyp) and np.array_equal(t_n.numpy(), n) and t_n.dtype == torch.int32
    frames = np.array([[0, 4, 4, 0, 4, 5, 5, 0], [0, 0, 0, 0, 0, 0, 0, 0], [7, 7, 7, 7, 7, 7, 7, 7], [1, 2, 3, 4, 5, 6, 7, 8]])
    hyp, n = hypothesis_of_frames(frames)
    assert n.tolist() == [3, 0, 1, 8] and hyp[0].tolist() == [4, 4, 5, 0, 0, 0, 0, 0] and hyp[2, 0] == 7 and hyp[3].tolist() == list(range(1, 9))
    t_hyp, t_n = ops.hypothesis_of_frames(torch.from_numpy(frames))
    assert np.array_equal(t_hyp.numpy(), hyp) and np.array_equal(t_n.numpy(), n)


def test_entry_points_are_declared_bound_exported_and_cited():
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.SHORTLIST_HEADER_PATH)
    assert tuple(protos) == SHORTLIST
    others = [_lib.parse_header(), _lib.parse_header(_lib.DECODE_HEADER_PATH), _lib.parse_header(_lib.ATTN_BEAM_HEADER_PATH),
              _lib.parse_header(_lib.LEXICON_HEADER_PATH), _lib.parse_header(_lib.ATTN_LEXICON_HEADER_PATH),
              _lib.parse_header(_lib.ATTN_SCORE_HEADER_PATH)]
    assert not any(set(protos) & set(o) for o in others)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    loaded = _lib.LIB.load()
    for name in SHORTLIST:
        assert hasattr(dll, name) and name in _lib.LIB._protos
        assert len(getattr(loaded, name).argtypes) == len(protos[name][2])
    ret, argtypes, argnames = protos["mrn_lexicon_shortlist_i32"]
    assert ret == "int" and loaded.mrn_lexicon_shortlist_i32.restype is ctypes.c_int
    assert argnames == ["hyp", "Hmax", "hyp_len", "B", "lex_tokens", "Lmax", "lex_len", "N", "K", "max_dist", "cand", "dist", "flag", "work",
                        "work_bytes", "stream"]
    assert [argtypes[argnames.index(a)] for a in ("hyp", "hyp_len", "lex_tokens", "lex_len")] == ["const int32_t*"] * 4
    assert [argtypes[argnames.index(a)] for a in ("cand", "dist", "flag")] == ["int32_t*"] * 3
    assert protos["mrn_lexicon_shortlist_work_bytes"][0] == "int64_t" and loaded.mrn_lexicon_shortlist_work_bytes.restype is ctypes.c_int64
    header = open(_lib.SHORTLIST_HEADER_PATH).read()
    comment = header[:header.index("int mrn_lexicon_shortlist_i32(")].rsplit("/*", 1)[1]
    assert "test.py:243-250" in comment
    for limit in ("1 <= K <= 256", "1 <= N <= 2^20", "1 <= Lmax <= 255", "0 <= Hmax", "65534", "hyp_len > 64"):
        assert limit in comment, limit
    # the workspace rule: a histogram of 256 counts per sample and the distance bytes in rows of a multiple of 16 (host-side: no launch)
    for B, N in ((0, 1), (1, 1), (3, 17), (256, 1 << 20)):
        assert loaded.mrn_lexicon_shortlist_work_bytes(B, N) == B * 1024 + B * ((N + 15) // 16 * 16)
    assert loaded.mrn_lexicon_shortlist_work_bytes(1, 0) == -1 and loaded.mrn_lexicon_shortlist_work_bytes(1, (1 << 20) + 1) == -1


def test_limits_match_the_kernel_source():
    import os
    import re
    from mrn_amd.modules import decoding as D
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrn_amd", "csrc", "lexicon_shortlist.hip")).read()
    const = {m.group(1): m.group(2) for m in re.finditer(r"constexpr int (SL_\w+) = ([^;]+);", src)}
    assert int(const["SL_MAX_K"]) == D.SHORTLIST_MAX_K and int(const["SL_MAX_L"]) == D.SHORTLIST_MAX_LENGTH
    assert int(const["SL_MAX_HYP"]) == D.SHORTLIST_MAX_HYPOTHESIS and const["SL_MAX_N"] == "1 << 20" and D.SHORTLIST_MAX_WORDS == 1 << 20
    assert D.shortlist_supported(255, 1 << 20, 256, 65534) and D.shortlist_supported(1, 1, 1, 0)
    for bad in ((256, 10, 5, 40), (0, 10, 5, 40), (10, 0, 5, 40), (10, (1 << 20) + 1, 5, 40), (10, 10, 0, 40), (10, 10, 257, 40), (10, 10, 5, 65535)):
        assert not D.shortlist_supported(*bad), bad


def test_the_combinations_that_are_errors():
    from mrn_amd.modules import decoding as D
    from mrn_amd.test import validation
    words = ["lds", "wave"]
    assert D.shortlist_request(SimpleNamespace(lexicon=words), False) is None
    assert D.shortlist_request(SimpleNamespace(lexicon=words, lexicon_shortlist=4), False) == (4, None)
    assert D.shortlist_request(SimpleNamespace(attn_lexicon=words, lexicon_shortlist=4, lexicon_max_distance=2), True) == (4, 2)
    # the other head's lexicon is ignored, as without a shortlist: it does not stand in for the head's own
    with pytest.raises(ValueError, match="words of lexicon, which is not set"):
        D.shortlist_request(SimpleNamespace(attn_lexicon=words, lexicon_shortlist=4), False)
    with pytest.raises(ValueError, match="words of attn_lexicon, which is not set"):
        D.shortlist_request(SimpleNamespace(lexicon=words, lexicon_shortlist=4), True)
    with pytest.raises(ValueError, match="lexicon_shortlist and candidates"):
        D.shortlist_request(SimpleNamespace(lexicon=words, lexicon_shortlist=4, candidates={"a": words}), False)
    # validation() refuses them before it touches the model or the loader
    conv = SimpleNamespace(dict={"[EOS]": 3})
    for prediction, keys, match in (("CTC", dict(lexicon_shortlist=4), "words of lexicon"), ("Attn", dict(lexicon_shortlist=4, lexicon=words), "words of attn_lexicon"),
                                    ("CTC", dict(lexicon_shortlist=4, lexicon=words, candidates={"a": words}), "lexicon_shortlist and candidates"),
                                    ("CTC", dict(lexicon_shortlist=0, lexicon=words), "lexicon_shortlist must be"),
                                    ("Attn", dict(lexicon_shortlist=2, attn_lexicon=words, lexicon_max_distance=-1), "lexicon_max_distance must be")):
        with pytest.raises(ValueError, match=match):
            validation(object(), None, [], conv, SimpleNamespace(Prediction=prediction, batch_max_length=25, **keys))
    # the evaluation forwards' keyword
    handle = object()
    assert D.attn_shortlist_request(None, "Attn", False) is None
    with torch.no_grad():
        assert D.attn_shortlist_request((handle, 5, None), "Attn", False) == (handle, 5, None)
        assert D.attn_shortlist_request((handle, 5, 1), "CTC", False) is None and D.attn_shortlist_request((handle, 5, 1), "Attn", True) is None
        for bad, match in (((handle, 0, None), "lexicon_shortlist"), ((handle, 5, -1), "lexicon_max_distance"), ((handle, 5), "attn_shortlist must be"),
                           (handle, "attn_shortlist must be")):
            with pytest.raises(ValueError, match=match):
                D.attn_shortlist_request(bad, "Attn", False)
        with pytest.raises(ValueError, match="pass one"):
            D.attn_shortlist_request((handle, 5, None), "Attn", False, attn_beam=4)
        with pytest.raises(ValueError, match="pass one"):
            D.attn_shortlist_request((handle, 5, None), "Attn", False, attn_candidates=handle)
    assert D.attn_shortlist_request((handle, 5, None), "Attn", False) is None          # gradients enabled: no evaluation


def test_cpu_tensors_take_the_host_form():
    from mrn_amd import ops
    rng = np.random.default_rng(5)
    words = draw_lexicon(40, 12, 5, 80, 2, True)
    tokens, lengths = as_arrays(words)
    hyps = [perturbed(rng, words[int(rng.integers(len(words)))], 40, 2) for _ in range(6)]
    hyp, hyp_len = hyp_arrays(hyps)
    handle = ops.upload_words(tokens, lengths, "cpu")
    cand, dist = ops.lexicon_shortlist(torch.from_numpy(hyp), torch.from_numpy(hyp_len), handle, 9, 3)
    r_cand, r_dist = shortlist_by_definition(hyps, words, 9, 3)
    assert cand.dtype == torch.int32 and dist.dtype == torch.int32 and not cand.is_cuda
    assert np.array_equal(cand.numpy(), r_cand) and np.array_equal(dist.numpy(), r_dist)
    again = ops.lexicon_shortlist(torch.from_numpy(hyp).long(), torch.from_numpy(hyp_len).long(), handle, 9, 3)
    assert torch.equal(again[0], cand) and torch.equal(again[1], dist)
    with pytest.raises(ValueError, match="upload_words"):
        ops.lexicon_shortlist(torch.from_numpy(hyp), torch.from_numpy(hyp_len), (tokens, lengths), 9)
    with pytest.raises(ValueError, match="K >= 1"):
        ops.lexicon_shortlist(torch.from_numpy(hyp), torch.from_numpy(hyp_len), handle, 0)
    # a candidate tensor is taken as it is: the table is still checked against the steps
    batch = handle.with_cand(cand, 12)
    assert batch.cand_dev is cand and batch.cand is cand
    with pytest.raises(ValueError, match="word lengths"):
        handle.with_cand(cand, 5)
    with pytest.raises(ValueError, match="contiguous int32"):
        handle.with_cand(cand.long(), 12)


@pytest.mark.parametrize("name", ["c37_w3", "few_w8", "c97_w4"])
def test_with_every_word_kept_the_best_word_is_the_exact_arg_max(name):
    """float64 on both sides: Attention.shortlist_search on CPU tensors with K >= N and no cut-off against attn_candidates_host over all
    words in index order.  The shortlist is a permutation of the lexicon, so nothing may be lost: the same best word, the same score,
    the same path.  Equal scores (the lexicon holds a word twice) go to the lower slot on both sides, and the shortlist lists equal
    words in index order"""
    from mrn_amd import ops
    from mrn_amd.modules.decoding import attn_candidates_host
    from mrn_amd.modules.prediction import Attention
    B, T, D, C, S, W, seed0, scale, n, shortest, empty = LEXICON_CASES[name]
    B = min(B, 4)
    sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
    words = draw_lexicon(C, S, seed0, n, shortest, empty)
    tokens, lengths = as_arrays(words)
    N = len(words)
    att = Attention(D, 256, C, torch.nn.Linear(256, C))
    att.load_state_dict(sd)
    handle = ops.upload_words(tokens, lengths, "cpu", 2)
    index, score, score_all, path, prob, cand, dist = att.shortlist_search(Hb, SOS, EOS, handle, N + 2, None, S - 1)
    cand, dist = cand.numpy(), dist.numpy()
    assert np.array_equal(np.sort(cand[:, :N], axis=1), np.tile(np.arange(N), (B, 1))) and np.all(cand[:, N:] == -1)
    assert np.all(np.diff(dist[:, :N], axis=1) >= 0)
    ref = attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, np.tile(np.arange(N, dtype=np.int32), (B, 1)), 2, S - 1)
    assert np.isfinite(ref[1][:, 0]).all()
    assert np.array_equal(index.numpy()[:, 0], ref[0][:, 0]) and np.array_equal(path.numpy(), ref[3])
    assert np.allclose(score.numpy()[:, 0], ref[1][:, 0], rtol=1e-6, atol=1e-6) and np.allclose(prob.numpy(), ref[4], rtol=1e-5, atol=1e-30)
    for b in range(B):                                             # every word's score sits in the slot the shortlist gave it
        assert np.allclose(score_all.numpy()[b, :N], ref[2][b, cand[b, :N]], rtol=1e-6, atol=1e-6)
    # a cut-off that nothing survives: the empty prediction with confidence 0
    far = att.shortlist_search(Hb, SOS, EOS, ops.upload_words(tokens[:1] * 0 + C - 1, lengths[:1] * 0 + tokens.shape[1], "cpu"), 3, 0, S - 1)
    assert (far[5] == -1).all() and (far[6] == -1).all()           # (the one word, S - 1 times the last class, is nobody's greedy decode)
    assert (far[0] == -1).all() and (far[3] == EOS).all() and (far[4] == 0).all()
