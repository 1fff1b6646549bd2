"""Host side of lexicon-constrained beam search on the attention head (no kernel is launched): the option, the encoder, the trie and
its check, the float64 reference attn_lexicon_host against the teacher-forced oracle, the C ABI of include/mrn_attn_lexicon.h, the LDS
rule, and the reference cases tests/test_decode_attn_lexicon_gpu.py decodes: how many of their samples are decisive is a property of the
reference alone."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import BEAM_CASES, EOS, SOS, TOKEN_BAND, beam_fixture, decisive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEXICON = ("mrn_attn_lexicon_decode_grouped_f32", "mrn_attn_lexicon_decode_x3_grouped")
# name: (B, T, D, C, S, W, seed0, generator weight scale, drawn words, shortest word, with the empty word)
LEXICON_CASES = {
    "c97_w4": BEAM_CASES["c97_w4"] + (300, 6, False),
    "c331_w8": BEAM_CASES["c331_w8"] + (1000, 5, False),           # a root of several hundred children: more than one pass of 64 lanes
    "d512_w16": BEAM_CASES["d512_w16"] + (1000, 4, False),
    "c37_w3": BEAM_CASES["c37_w3"] + (60, 3, False),               # W does not divide 16: a row that belongs to no sample
    "few_w8": (19, 31, 256, 97, 12, 8, 200, 100.0, 5, 1, True),    # a root of fewer than W children, terminal itself
    "t127_c5374_w8": BEAM_CASES["t127_c5374_w8"] + (2000, 1, True),
}
_REF = {}


def draw_lexicon(C, S, seed0, words, shortest, empty):
    """the lexicon of a case as a list of class tuples: characters are the classes 4 ... C - 1; one word of exactly S - 1 characters,
    then `words` - 1 of length U[shortest, S - 1], a character with probability 0.6 one of the first 8 admissible classes (deep shared
    prefixes) and else any (a wide root); behind a word, with probability 0.15, its first half when that has at least max(shortest, 1)
    characters; the empty word where the case has it; finally the sixth word once more"""
    rng = np.random.default_rng(seed0 + 7)

    def word(n):
        near = rng.random(n) < 0.6
        return tuple(int(c) for c in np.where(near, rng.integers(4, min(12, C), n), rng.integers(4, C, n)))

    out = [word(S - 1)]
    for _ in range(words - 1):
        w = word(int(rng.integers(shortest, S)))
        out.append(w)
        if rng.random() < 0.15 and len(w) // 2 >= max(shortest, 1):
            out.append(w[:len(w) // 2])
    if empty:
        out.append(())
    out.append(out[min(5, len(out) - 1)])
    return out


def as_arrays(words):
    lengths = np.array([len(w) for w in words], dtype=np.int32)
    tokens = np.zeros((len(words), max(int(lengths.max()), 1)), dtype=np.int32)
    for i, w in enumerate(words):
        tokens[i, :len(w)] = w
    return tokens, lengths


def lexicon_case(name):
    """(sd, Hb, words, trie, reference outputs of attn_lexicon_host with the margin) of a case, computed once and shared (never modified)"""
    if name not in _REF:
        from mrn_amd.modules import decoding
        B, T, D, C, S, W, seed0, scale, n, shortest, empty = LEXICON_CASES[name]
        sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
        words = draw_lexicon(C, S, seed0, n, shortest, empty)
        trie = decoding.build_trie(*as_arrays(words))
        _REF[name] = (sd, Hb, words, trie, decoding.attn_lexicon_host(sd, Hb, SOS, EOS, W, S - 1, trie, want_margin=True))
    return _REF[name]


def test_options():
    from mrn_amd.modules import decoding as D
    assert D.attn_lexicon_options(SimpleNamespace()) == (None, 8)
    assert D.attn_lexicon_options(SimpleNamespace(attn_lexicon=None, beam_width=3)) == (None, 3)
    assert D.attn_lexicon_options(SimpleNamespace(attn_lexicon=("ab", "c"), attn_decode="greedy")) == (["ab", "c"], 8)
    assert D.attn_lexicon_options(SimpleNamespace(attn_lexicon=iter(["ab"]), beam_width=np.int64(5))) == (["ab"], 5)
    for bad in ("word", b"word", 7):
        with pytest.raises(ValueError, match=r"attn_lexicon must be a sequence of words \(str\)"):
            D.attn_lexicon_options(SimpleNamespace(attn_lexicon=bad))
    with pytest.raises(ValueError, match="got an entry 3"):
        D.attn_lexicon_options(SimpleNamespace(attn_lexicon=["a", 3]))
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="beam_width"):
            D.attn_lexicon_options(SimpleNamespace(attn_lexicon=["a"], beam_width=bad))
    # the neighbours do not read the key, and it does not read theirs
    assert D.lexicon_options(SimpleNamespace(attn_lexicon=["a"])) == (None, 1)
    assert D.attn_decode_options(SimpleNamespace(attn_lexicon=["a"])) == ("greedy", 8)
    assert D.attn_lexicon_options(SimpleNamespace(lexicon=["a"])) == (None, 8)
    assert D.ATTN_DECODERS == ("greedy", "beam")                   # no "constrained greedy"
    with pytest.raises(ValueError, match="attn_beam"):
        D.attn_lexicon_request(object(), None)
    assert D.attn_lexicon_request(None, None) is None


def test_encoder_keeps_what_the_converter_can_spell():
    from mrn_amd.modules import decoding as D
    from mrn_amd.tools.utils import AttnLabelConverter
    conv = AttnLabelConverter("abcdefghij")
    words = ["abc", "aBc", "a c", "[EOS]", "a[", "abc", "", "abcdefghij", "abcde", "xyz"]
    tokens, lengths, kept = D.encode_attn_lexicon(conv, words, 5)
    assert kept == ["abc", "a c", "abc", "", "abcde"]              # case-sensitive, duplicates and the empty word kept, ' ' a class
    assert tokens.dtype == np.int32 and lengths.dtype == np.int32 and tokens.shape == (5, 5)
    assert lengths.tolist() == [3, 3, 3, 0, 5]
    assert tokens[1].tolist() == [conv.dict["a"], conv.dict[" "], conv.dict["c"], 0, 0]
    assert D.encode_attn_lexicon(conv, [""], 5)[0].shape == (1, 1)
    # the specials are characters of the converter's table only as whole names, never reachable from a str; a table that holds one is refused
    odd = SimpleNamespace(dict={"[UNK]": 0, "[PAD]": 1, "[SOS]": 2, "[EOS]": 3, "a": 4, "#": 3})
    assert D.encode_attn_lexicon(odd, ["a#", "a"], 5)[2] == ["a"]
    for none_left in (["xyz", "ABC"], ["abcdef"], []):
        with pytest.raises(ValueError, match="attn_lexicon: none of the"):
            D.encode_attn_lexicon(conv, none_left, 5)


def test_trie_layout():
    from mrn_amd.modules import decoding as D
    words = [(5, 6, 7), (5, 6), (4,), (5, 6, 7), (), (9, 4), (5, 9)]
    trie = D.build_trie(*as_arrays(words))
    # level 1: 4, 5, 9 -> nodes 1, 2, 3; level 2: (5,6), (5,9), (9,4) -> 4, 5, 6; level 3: (5,6,7) -> 7
    assert trie.child_off.tolist() == [0, 3, 3, 5, 6, 7, 7, 7, 7]
    assert trie.child_tok.tolist() == [4, 5, 9, 6, 9, 4, 7]
    assert trie.child_node.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert trie.word_of.tolist() == [4, 2, -1, -1, 1, 6, 5, 0]      # the empty word at the root, a prefix word inside, duplicates -> lowest
    assert trie.depth == 3 and trie.words == 7
    assert all(a.dtype == np.int32 for a in trie[:4])
    assert D.check_trie(trie) == (8, 7)
    rng = np.random.default_rng(3)
    for name in ("c97_w4", "few_w8"):
        B, T, Dm, C, S, W, seed0, scale, n, shortest, empty = LEXICON_CASES[name]
        words = draw_lexicon(C, S, seed0, n, shortest, empty)
        trie = D.build_trie(*as_arrays(words))
        M = len(trie.word_of)
        assert len(trie.child_off) == M + 1 and len(trie.child_tok) == len(trie.child_node) == M - 1 and trie.depth == S - 1
        parent = np.repeat(np.arange(M), np.diff(trie.child_off))
        assert np.all(trie.child_node > parent) and np.all(np.diff(trie.child_node) == 1)         # breadth-first
        for n_ in range(M):
            kids = trie.child_tok[trie.child_off[n_]:trie.child_off[n_ + 1]]
            assert np.all(np.diff(kids) > 0)                       # ascending, distinct
        # every word is found by walking, and word_of is the lowest index that spells it
        lowest = {}
        for i, w in enumerate(words):
            lowest.setdefault(w, i)
        for w, i in lowest.items():
            node = 0
            for c in w:
                lo, hi = trie.child_off[node], trie.child_off[node + 1]
                e = lo + int(np.searchsorted(trie.child_tok[lo:hi], c))
                assert e < hi and trie.child_tok[e] == c
                node = trie.child_node[e]
            assert trie.word_of[node] == i
        assert int((trie.word_of >= 0).sum()) == len(lowest) and (trie.word_of[0] >= 0) == (() in lowest)
        # the numbering does not depend on the order of the words; word_of follows the lowest index
        perm = rng.permutation(len(words))
        other = D.build_trie(*as_arrays([words[p] for p in perm]))
        for a, b in zip(trie[:3], other[:3]):
            assert np.array_equal(a, b)
        ends = trie.word_of >= 0
        assert np.array_equal(ends, other.word_of >= 0)
        inverse = {w: min(k for k, p in enumerate(perm) if words[p] == w) for w in lowest}
        assert all(other.word_of[n_] == inverse[words[trie.word_of[n_]]] for n_ in np.flatnonzero(ends))
    for bad in ((np.zeros((2, 3)), np.array([1])), (np.zeros((0, 3)), np.zeros(0)), (np.zeros((1, 2)), np.array([3])),
                (np.array([[-1, 2]]), np.array([2]))):
        with pytest.raises(ValueError, match="build_trie"):
            D.build_trie(*bad)


def test_a_malformed_trie_is_refused_on_the_host():
    """ops.upload_trie's check, through its host-side function: everything that could send the kernel's reads outside the arrays"""
    from mrn_amd import ops
    from mrn_amd.modules import decoding as D
    good = D.build_trie(*as_arrays([(5, 6, 7), (5, 6), (4,), (9, 4)]))
    assert D.check_trie(good) == (7, 6)
    handle = ops.upload_trie(good, "cpu")
    assert (handle.nodes, handle.depth, handle.words) == (7, 3, 4) and handle.child_off.dtype == torch.int32

    def edit(field, fn):
        a = getattr(good, field).copy()
        return good._replace(**{field: fn(a)})

    def put(i, v):
        def fn(a):
            a[i] = v
            return a
        return fn

    bad = {
        "offsets do not start at 0": edit("child_off", put(0, 1)),
        "offsets fall": edit("child_off", put(2, 0)),
        "offsets end past the edges": edit("child_off", put(-1, 7)),
        "one offset short": edit("child_off", lambda a: a[:-1].copy()),
        "a child at its parent": edit("child_node", put(0, 0)),
        "a child below its parent": edit("child_node", put(5, 1)),
        "a child past the nodes": edit("child_node", put(5, 7)),
        "a negative class": edit("child_tok", put(1, -1)),
        "a word past the lexicon": edit("word_of", put(3, 4)),
        "a word below -1": edit("word_of", put(0, -2)),
        "int64": edit("child_tok", lambda a: a.astype(np.int64)),
        "not contiguous": edit("word_of", lambda a: np.repeat(a, 2)[::2]),
        "two-dimensional": edit("child_node", lambda a: a.reshape(1, -1)),
        "a list": good._replace(child_tok=good.child_tok.tolist()),
        "deeper than depth": good._replace(depth=2),
        "negative depth": good._replace(depth=-1),
        "no words": good._replace(words=0),
        "edges and nodes disagree": edit("child_tok", lambda a: a[:-1].copy()),
    }
    for what, trie in bad.items():
        with pytest.raises(ValueError, match="trie:"):
            D.check_trie(trie)
        with pytest.raises(ValueError, match="trie:"):
            ops.upload_trie(trie, "cpu")                           # before any tensor is made, whatever the device
    root = D.build_trie(np.zeros((1, 1), dtype=np.int32), np.zeros(1, dtype=np.int32))
    assert D.check_trie(root) == (1, 0) and root.word_of.tolist() == [0] and root.depth == 0


def teacher_forced(sd, Hb, b, words, S):
    """the oracle's teacher-forced log-softmax of every word for sample b: [N][S][C] float64"""
    from oracle import mrn_oracle as O
    osd = {"P." + k: v for k, v in sd.items()}
    text = torch.tensor([[SOS] + list(w) + [EOS] * (S - 1 - len(w)) for w in words], dtype=torch.int64)
    T, Dm = Hb.shape[1:]
    logits = O.attention_forward(osd, "P.", Hb[b:b + 1].expand(len(words), T, Dm), text, True, S - 1, sd["generator.weight"],
                                 sd["generator.bias"])
    return torch.log_softmax(logits.double(), dim=2).numpy()


def word_scores(lsm, words):
    return np.array([sum(lsm[i, s, c] for s, c in enumerate(w + (EOS,))) for i, w in enumerate(words)])


def test_reference_is_the_exact_arg_max_over_a_small_lexicon():
    """width >= the number of distinct words: nothing is pruned, the live entries are exactly the words, every score is the
    teacher-forced oracle's sum over the word and its eos (the oracle is float32: a band of 2e-4 per token), and the order is the
    oracle's wherever neighbouring oracle scores differ by at least three bands"""
    from mrn_amd.modules import decoding as D
    B, T, Dm, C, S, _, seed0, scale = BEAM_CASES["c97_w4"]
    sd, Hb = beam_fixture(B, T, Dm, C, seed0, scale)
    words = [w for w in draw_lexicon(C, S, seed0, 9, 2, True)]
    distinct = list(dict.fromkeys(words))
    assert len(distinct) <= 12 and () in distinct and len(distinct) < len(words)
    trie = D.build_trie(*as_arrays(words))
    W = 12
    tokens, length, score, logp, path, prob, word = D.attn_lexicon_host(sd, Hb[:6], SOS, EOS, W, S - 1, trie)
    assert word.dtype == np.int32 and word.shape == (6, W)
    for b in range(6):
        want = word_scores(teacher_forced(sd, Hb, b, distinct, S), distinct)
        live = length[b] >= 0
        assert int(live.sum()) == len(distinct) and np.all(live[:len(distinct)]) and np.all(word[b][~live] == -1)
        got = {}
        for w in range(len(distinct)):
            n = int(length[b, w])
            spelled = tuple(int(c) for c in tokens[b, w, :n - 1])
            assert tokens[b, w, n - 1] == EOS and words[word[b, w]] == spelled and words.index(spelled) == word[b, w]
            got[spelled] = score[b, w]
            assert abs(logp[b, w, :n].sum() - score[b, w]) < 1e-9
        assert set(got) == set(distinct)
        for i, w in enumerate(distinct):
            assert abs(got[w] - want[i]) <= (len(w) + 1) * TOKEN_BAND, (b, w)
        order = np.argsort(-want, kind="stable")
        rank = {tuple(int(c) for c in tokens[b, w, :length[b, w] - 1]): w for w in range(len(distinct))}
        for x, y in zip(order[:-1], order[1:]):
            if want[x] - want[y] >= 3 * (max(len(distinct[x]), len(distinct[y])) + 1) * TOKEN_BAND:
                assert rank[distinct[x]] < rank[distinct[y]], (b, distinct[x], distinct[y])
        assert np.array_equal(path[b], tokens[b, 0]) and np.all(score[b][:-1][live[1:]] >= score[b][1:][live[1:]])


def test_entries_of_a_narrow_beam_are_distinct_lexicon_words():
    """W below the number of words: every live entry is a lexicon word ending in eos, the words are distinct, the scores descend, dead
    slots come last -- on every case the GPU file decodes"""
    for name, (B, T, Dm, C, S, W, *_rest) in LEXICON_CASES.items():
        sd, Hb, words, trie, ref = lexicon_case(name)
        tokens, length, score, logp, path, prob, word, margin = ref
        assert tokens.shape == (B, W, S) and word.shape == (B, W)
        assert (len(set(words)) > W) == (name != "few_w8")
        for b in range(B):
            live = length[b] >= 0
            assert live[0] and np.all(live[:-1] >= live[1:])                      # dead slots last
            assert np.all(word[b][~live] == -1) and np.all(np.isneginf(score[b][~live])) and np.all(tokens[b][~live] == EOS)
            seen = set()
            for w in np.flatnonzero(live):
                n = int(length[b, w])
                spelled = tuple(int(c) for c in tokens[b, w, :n - 1])
                assert tokens[b, w, n - 1] == EOS and np.all(tokens[b, w, n:] == EOS) and EOS not in spelled
                assert words[word[b, w]] == spelled and words.index(spelled) == word[b, w]
                assert spelled not in seen
                seen.add(spelled)
            s = score[b][live]
            assert np.all(s[:-1] >= s[1:])
        if name == "few_w8":                                                     # six distinct words at W = 8: two dead slots per sample
            assert np.all((length >= 0).sum(axis=1) == len(set(words)))


def test_a_sample_without_an_admissible_word_is_all_dead():
    """an expert whose classes stop below every word's first class: no live entry at all"""
    from mrn_amd.modules import decoding as D
    B, T, Dm, C, S, W, seed0, scale = BEAM_CASES["c37_w3"]
    sd, Hb = beam_fixture(B, T, Dm, C, seed0, scale)
    trie = D.build_trie(*as_arrays([(40, 5), (41,), (300, 4, 4)]))
    tokens, length, score, logp, path, prob, word, margin = D.attn_lexicon_host(sd, Hb, SOS, EOS, W, S - 1, trie, want_margin=True)
    assert np.all(length == -1) and np.all(np.isneginf(score)) and np.all(word == -1) and np.all(tokens == EOS) and np.all(logp == 0)
    assert np.all(path == EOS) and np.all(prob == 1.0) and np.all(np.isposinf(margin))
    with pytest.raises(ValueError, match="longest word"):
        D.attn_lexicon_host(sd, Hb, SOS, EOS, W, 2, trie)


def test_reference_cases_are_decisive_enough():
    """at most B // 4 samples of a GPU case may be left to the self-consistency check alone"""
    for name, (B, T, Dm, C, S, W, *_rest) in LEXICON_CASES.items():
        ref = lexicon_case(name)[4]
        margin = ref[7]
        loose = int((~decisive(margin)).sum())
        print(f"{name}: {loose} of {B} samples are not decisive (cap {B // 4}); smallest margin {margin.min():.3e}; best words of "
              f"{int(ref[1][:, 0].min()) - 1} ... {int(ref[1][:, 0].max()) - 1} characters")
        assert loose <= B // 4, name
        assert np.all(ref[1][:, 0] >= 1)


def test_entry_points_are_declared_bound_exported_and_cited():
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.ATTN_LEXICON_HEADER_PATH)
    assert tuple(protos) == LEXICON
    others = [_lib.parse_header(), _lib.parse_header(_lib.DECODE_HEADER_PATH), _lib.parse_header(_lib.ATTN_BEAM_HEADER_PATH),
              _lib.parse_header(_lib.LEXICON_HEADER_PATH)]
    assert not any(set(protos) & set(o) for o in others)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    loaded = _lib.LIB.load()
    header = open(_lib.ATTN_LEXICON_HEADER_PATH).read()
    for name in LEXICON:
        ret, argtypes, argnames = protos[name]
        beam = others[2][name.replace("lexicon", "beam")][2]
        assert hasattr(dll, name) and name in _lib.LIB._protos
        bound = getattr(loaded, name)
        assert bound.restype is ctypes.c_int and len(bound.argtypes) == len(argnames) == len(beam) + 7
        trie = ["child_off", "child_tok", "child_node", "word_of", "nodes", "depth"]
        cut = beam.index("W") + 1
        assert argnames[:cut] == beam[:cut] and argnames[cut:cut + 6] == trie                # the beam's operands, then the trie
        rest = argnames[cut + 6:]
        assert rest == beam[cut:beam.index("groups")] + ["word"] + beam[beam.index("groups"):]
        assert [argtypes[argnames.index(a)] for a in trie[:4]] == ["const int32_t*"] * 4
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "modules/prediction.py:70-86" in comment, name
        for limit in ("1 <= W <= 16", "1 <= S <= 512", "num_class >= 2", "hidden = 256", "nodes >= 1", "depth <= S - 1",
                      "multiple of " + ("32" if "x3" in name else "16")):
            assert limit in comment, (name, limit)


def test_rule_matches_the_launch_helper():
    """ops.attn_lexicon_whole_context restates the lexicon launch's LDS sum in csrc/attn_decode.hip (the beam's plus LEX_LDS_MORE), and the two
    kernels share one body"""
    from mrn_amd import ops
    src = open(os.path.join(ROOT, "mrn_amd", "csrc", "attn_decode.hip")).read()
    consts = dict(re.findall(r"(?m)^constexpr int (\w+) = ([^;]+);", src))
    assert re.sub(r"\s+", " ", consts["LEX_LDS_MORE"]).strip() == "4 * (2 * BT + BT * BT)"
    assert ops.ATTN_LEXICON_LDS_EXTRA == ops.ATTN_BEAM_LDS_EXTRA + 4 * (2 * 16 + 16 * 16) == 3584 + 1152
    launch = re.sub(r"\s+", " ", src[src.index("static int beam_launch("):src.index("static int beam_grouped(")])
    assert "lds = attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA) + (lex ? LEX_LDS_MORE : 0)" in launch
    body = re.sub(r"\s+", " ", src[src.index("static int beam_grouped("):src.index("MRN_EXPORT int mrn_attn_beam_decode_grouped_f32")])
    fits = "attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA + LEX_LDS_MORE) <= 160 * 1024"
    for check in (fits, "nodes >= 1", "depth <= S - 1", "child_off && child_tok && child_node && word_of && word"):
        assert check in body and body.index(check) < body.index("beam_launch("), check      # refused before the first launch
    assert src.count("attn_beam_body<X3, false>(grp") == 1 and src.count("attn_beam_body<X3, true>(grp") == 1
    assert src.count("void attn_beam_body(") == 1
    for kernel in ("void attn_beam_kernel(const BeamGroup grp) {", "void attn_lexicon_kernel(const BeamGroup grp, const LexTrie lex) {"):
        after = src[src.index(kernel) + len(kernel):]
        assert after[:after.index("}")].strip().startswith("attn_beam_body<X3, ") and after.index("}") < 80      # one body, not a copy
    for T in (17, 65, 129):
        for x3 in (True, False):
            for D in list(range(32, 2600, 32)) + [48, 264]:
                for W in (0, 1, 3, 16, 17):
                    lds = 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + (1024 if x3 else 0) + 3584 + 1152
                    want = lds <= 160 * 1024 and 1 <= W <= 16 and D % (32 if x3 else 16) == 0
                    assert ops.attn_lexicon_whole_context(D, T, W, x3) == want, (D, T, W, x3)
    # the 1152 bytes matter at exactly one width of the x3 form at T = 65: the beam launch takes D = 2176, the lexicon launch does not
    assert ops.attn_beam_whole_context(1792, 65, 8, True) and ops.attn_lexicon_whole_context(1792, 65, 8, True)
    assert not ops.attn_lexicon_whole_context(2304, 65, 8, True)
    edge = [D for D in range(32, 2600, 32) if ops.attn_beam_whole_context(D, 65, 8, True) != ops.attn_lexicon_whole_context(D, 65, 8, True)]
    print("context widths the beam launch takes and the lexicon launch does not (T = 65, x3):", edge)


def test_cpu_tensors_take_the_host_form():
    """Attention.lexicon_search on CPU tensors is attn_lexicon_host; Model.heads refuses a lexicon without a width"""
    from mrn_amd import ops
    import torch.nn as nn
    from mrn_amd.modules.prediction import Attention
    name = "c37_w3"
    B, T, Dm, C, S, W, *_rest = LEXICON_CASES[name]
    sd, Hb, words, trie, ref = lexicon_case(name)
    att = Attention(Dm, 256, C, nn.Linear(256, C))
    att.load_state_dict(sd)
    got = att.lexicon_search(Hb, SOS, EOS, W, ops.upload_trie(trie, "cpu"), S - 1)
    assert len(got) == 7
    for g, r in zip(got, ref):
        assert np.array_equal(g.numpy(), r.astype(np.float32) if r.dtype == np.float64 else r)
    with pytest.raises(ValueError, match="upload_trie"):
        att.lexicon_search(Hb, SOS, EOS, W, trie, S - 1)
    with pytest.raises(ValueError, match="longest word"):
        att.lexicon_search(Hb, SOS, EOS, W, ops.upload_trie(trie, "cpu"), S - 2)
