"""Lexicon-constrained beam search on the attention head in one launch (mrn_attn_lexicon_decode_*, csrc/attn_decode.hip attn_lexicon_kernel)
against the float64 reference mrn_amd/modules/decoding.py::attn_lexicon_host.

Bands and the notion of a decisive sample are those of tests/test_decode_attn_beam_gpu.py: a chosen token's log-probability is held to
2e-4, a score of n tokens to n * 2e-4; a sample is decisive when every gap of the REFERENCE among its admissible candidates is at least
three times the step's band, and decisive samples must match the reference exactly in tokens, lengths, order and words.  Every live
entry, decisive or not, must be self-consistent: its tokens, fed through the teacher-forced decoder, give its log-probabilities and score
back.  tests/test_attn_lexicon_cpu.py holds the cases and checks on the CPU that at most B // 4 samples of a case are not decisive.

The file's name puts it behind tests/test_bench_gpu.py in the suite, as the beam file's does."""
import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import BEAM_CASES, EOS, SOS, TOKEN_BAND, beam_fixture, decisive
from tests.test_attn_lexicon_cpu import LEXICON_CASES, as_arrays, draw_lexicon, lexicon_case, teacher_forced, word_scores
from tests.test_decode_attn_beam_gpu import (CHARACTERS, LABELS, check_against_reference, check_self_consistent, kept_confidence,
                                             to_np, trba_nets, trba_opt)
from tests.test_greedy_decode_gpu import CASES, HID, case, module, sos

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def search(ops, att, Hb, W, S, trie, eos=EOS):
    return to_np(att.lexicon_search(Hb.cuda(), SOS, eos, W, ops.upload_trie(trie, "cuda"), S - 1))


def recorded_calls(monkeypatch, fn):
    """(fn(), the names of the library calls it made)"""
    from mrn_amd._lib import LIB
    names, real = [], LIB.call
    monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.setattr(LIB, "call", real)


def check_layout(got, B, W, S, words, eos=EOS, may_be_empty=False):
    """the beam tests' layout check with `word`: shapes, fills, dead slots last (a sample may have none but dead slots only where the
    test says so), every live entry a lexicon word ending in eos and named by the lowest index that spells it"""
    tokens, length, score, logp, path, prob, word = got
    assert tokens.shape == (B, W, S) and tokens.dtype == np.int32 and length.shape == (B, W) and length.dtype == np.int32
    assert score.shape == (B, W) and score.dtype == np.float32 and logp.shape == (B, W, S) and logp.dtype == np.float32
    assert path.shape == (B, S) and path.dtype == np.int64 and prob.shape == (B, S) and prob.dtype == np.float32
    assert word.shape == (B, W) and word.dtype == np.int32
    if not may_be_empty:
        assert np.all(length[:, 0] >= 1)
    for b in range(B):
        seen = set()
        for w in range(W):
            n = int(length[b, w])
            if n < 0:
                assert n == -1 and np.isneginf(score[b, w]) and np.all(tokens[b, w] == eos) and np.all(logp[b, w] == 0) and word[b, w] == -1
                assert np.all(length[b, w:] == -1)                          # dead slots come last
                continue
            assert 1 <= n <= S and np.isfinite(score[b, w])
            spelled = tuple(int(c) for c in tokens[b, w, :n - 1])
            assert tokens[b, w, n - 1] == eos and eos not in spelled and np.all(tokens[b, w, n:] == eos) and np.all(logp[b, w, n:] == 0)
            assert 0 <= word[b, w] < len(words) and words[word[b, w]] == spelled and words.index(spelled) == word[b, w]
            assert spelled not in seen
            seen.add(spelled)
        live = score[b][length[b] >= 0]
        assert np.all(live[:-1] >= live[1:])                                # descending score
    assert np.array_equal(path, tokens[:, 0].astype(np.int64))
    # (a token the lexicon forces may have a probability below float32's smallest normal number, 1.18e-38, where exp has no 24 bits
    # left and the device flushes to zero: the relative bound of the beam file holds above it, the absolute one below)
    np.testing.assert_allclose(prob, np.exp(logp[:, 0].astype(np.float64)), rtol=2e-6, atol=float(np.finfo(np.float32).tiny))
    assert np.all(prob[logp[:, 0] == 0] == 1.0)


def check_reference(name, got, ref):
    """check_against_reference of the beam file on the six shared outputs, and the words of decisive samples.  A sample whose
    reference has no live entry (every entry of a narrow beam ran into prefixes the expert's classes cannot continue) is compared here:
    the beam file's check divides by the live entries' lengths"""
    dead = ref[1][:, 0] < 0
    check_against_reference(name, got[:6], ref[:6] + (np.where(dead, 0.0, ref[7]),))
    for b in np.flatnonzero(decisive(ref[7])):
        assert np.array_equal(got[6][b], ref[6][b]), (name, b)
        if dead[b]:
            assert np.all(got[1][b] == -1) and np.all(np.isneginf(got[2][b])) and np.all(got[0][b] == ref[0][b]) and np.all(got[3][b] == 0)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("name", list(LEXICON_CASES))
def test_kernel_matches_the_reference_and_itself(ops, monkeypatch, name, x3):
    """the fused launch, both forms: layout, self-consistency, the reference on decisive samples"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, W, *_rest = LEXICON_CASES[name]
    sd, Hb, words, trie, ref = lexicon_case(name)
    att = module(sd, D, C)
    handle = ops.upload_trie(trie, "cuda")
    assert att.lexicon_fused(D, T, S, EOS, W, handle)
    got, names = recorded_calls(monkeypatch, lambda: to_np(att.lexicon_search(Hb.cuda(), SOS, EOS, W, handle, S - 1)))
    assert [n for n in names if "beam" in n or "lexicon" in n] == ["mrn_attn_lexicon_decode_x3_grouped" if x3 else
                                                                  "mrn_attn_lexicon_decode_grouped_f32"]
    check_layout(got, B, W, S, words)
    check_self_consistent(att, Hb, got[:6])
    check_reference(name, got, ref)


@pytest.mark.parametrize("x3", [True, False])
def test_a_wide_beam_is_the_exact_arg_max(ops, monkeypatch, x3):
    """at most 16 distinct words at W = 16: nothing is pruned, entry 0 is the arg-max of the teacher-forced scores of all words (the
    oracle's, float32: decisive = the two best oracle scores differ by three bands of the longer word), and all words are returned"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, _, seed0, scale = BEAM_CASES["c97_w4"]
    sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
    words = draw_lexicon(C, S, seed0, 13, 2, True)
    distinct = list(dict.fromkeys(words))
    assert len(distinct) <= 16 < len(distinct) + 3
    from mrn_amd.modules import decoding
    trie = decoding.build_trie(*as_arrays(words))
    att = module(sd, D, C)
    got = search(ops, att, Hb, 16, S, trie)
    check_layout(got, B, 16, S, words)
    assert np.all((got[1] >= 0).sum(axis=1) == len(distinct))
    checked = 0
    for b in range(B):
        want = word_scores(teacher_forced(sd, Hb, b, distinct, S), distinct)
        first, second = np.argsort(-want, kind="stable")[:2]
        if want[first] - want[second] < 3 * (max(len(distinct[first]), len(distinct[second])) + 1) * TOKEN_BAND:
            continue
        checked += 1
        assert words[got[6][b, 0]] == distinct[first], b
        assert abs(got[2][b, 0] - want[first]) <= (len(distinct[first]) + 1) * TOKEN_BAND
    print(f"{checked} decisive samples of {B}")
    assert checked >= B - B // 4


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("eos", [1, 320])
def test_ties_go_to_the_lower_entry_then_the_lower_class_among_admissible_children(ops, monkeypatch, x3, eos):
    """class 5's generator row, bias and embedding copied to 7, 300 and eos and all four lifted above every other class, as in the beam
    file's tie test: every lifted candidate of a step has the same log-probability lp, whatever the entry.  The lexicon is (5), (5 7),
    (5 300), (300), (5 7 5), (9): the root admits 5, 9 and 300 (7 is lifted too, but inadmissible), node (5) the classes 7 and 300 and the
    word end, (5 7) the class 5 and the word end.  W = 4, eos below (1) and above (320) the children's classes:
      step 0: [5], [300] at lp, [9] far below;
      step 1: four candidates at 2 lp in (entry, class) order -- eos = 1: [5 eos] [5 7] [5 300] [300 eos]; eos = 320: [5 7] [5 300] [5 eos]
              [300 eos] -- and [9 eos] is dropped;
      step 2: the two finished entries stay at 2 lp; three candidates at 3 lp, in (entry, class) order [5 7 eos], [5 7 5], [5 300 eos]
              for eos = 1 and [5 7 5], [5 7 eos], [5 300 eos] for eos = 320: the entry decides before the class, [5 300 eos] is dropped;
      step 3: [5 7 5 eos] at 4 lp.
    Entries: (5), (300), (5 7), (5 7 5)"""
    from mrn_amd.modules import decoding
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, _ = CASES["c331"]
    sd, Hb, _ = case("c331")
    sd = {k: v.clone() for k, v in sd.items()}
    sd["generator.bias"][5] += 30.0
    for other in (7, 300, eos):
        sd["generator.weight"][other] = sd["generator.weight"][5]
        sd["generator.bias"][other] = sd["generator.bias"][5]
        sd["char_embeddings.weight"][other] = sd["char_embeddings.weight"][5]
    words = [(5,), (5, 7), (5, 300), (300,), (5, 7, 5), (9,)]
    trie = decoding.build_trie(*as_arrays(words))
    att = module(sd, D, C)
    got = search(ops, att, Hb, 4, S, trie, eos=eos)
    check_layout(got, B, 4, S, words, eos=eos)
    tokens, length, score, logp, path, prob, word = got
    assert np.array_equal(word, np.tile(np.int32([0, 3, 1, 4]), (B, 1)))
    assert np.array_equal(length, np.tile(np.int32([2, 2, 3, 4]), (B, 1)))
    for k, w in enumerate(((5,), (300,), (5, 7), (5, 7, 5))):
        assert np.array_equal(tokens[:, k], np.tile(np.int32(list(w) + [eos] * (S - len(w))), (B, 1))), k
    assert np.all(score[:, 0] == score[:, 1]) and np.all(score[:, 1] > score[:, 2]) and np.all(score[:, 2] > score[:, 3])


def lexicon_grouped_fixture(G, B, T, S):
    """G experts with class counts 37 / 97 / 331 cycling, on their own features"""
    classes = [(37, 97, 331)[g % 3] for g in range(G)]
    atts, Hbs, sds = [], [], []
    for g, C in enumerate(classes):
        sd, Hb = beam_fixture(B, T, 256, C, 700 + 40 * g, 100.0)
        sds.append(sd)
        atts.append(module(sd, 256, C))
        Hbs.append(Hb)
    return classes, atts, torch.stack(Hbs).cuda(), sds


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("G", [3, 9])
def test_grouped_equals_single_launches_and_the_host_form(ops, monkeypatch, G, x3):
    """one lexicon over the 331-class alphabet for experts of 37 / 97 / 331 classes in one launch (nine experts in two): every group
    bit-identical to its single launch, and the host form on decisive samples -- a child whose class an expert does not have is
    skipped, never read.  With a lexicon whose every word starts above class 36 the 37-class experts return only dead slots"""
    from mrn_amd.modules import decoding
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, S, W = 7, 31, 12, 4
    classes, atts, Hb, sds = lexicon_grouped_fixture(G, B, T, S)
    words = draw_lexicon(331, S, 900, 400, 3, False)
    high = [w for w in words if w[0] > 36]
    assert len(high) > 50 and any(w[0] < 37 and max(w) > 96 for w in words) and any(max(w) < 37 for w in words)
    for lexicon in (words, high):
        trie = decoding.build_trie(*as_arrays(lexicon))
        handle = ops.upload_trie(trie, "cuda")
        with torch.no_grad():
            Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
            cols = list(zip(*[a.greedy_args() for a in atts]))
            grouped = ops.attn_lexicon_decode_grouped(Hb, Hproj, cols[0], sos(SOS), *cols[1:9], HID, S, EOS, W, handle,
                                                      w_inv=cols[9] if x3 else None)
            assert len(grouped) == 7 and grouped[6].shape == (G, B, W) and (cols[9][0] is not None) == x3
            for g, a in enumerate(atts):
                one = ops.attn_lexicon_decode(Hb[g], Hproj[g], cols[0][g], sos(SOS), *[c[g] for c in cols[1:9]], HID, S, EOS, W, handle,
                                              w_inv=cols[9][g] if x3 else None)
                for x, y in zip(grouped, one):
                    assert torch.equal(x[g], y), f"expert {g}"
                got = to_np(one)
                dead = lexicon is high and classes[g] == 37
                # (fewer classes than the lexicon's alphabet: a narrow beam may follow only prefixes whose continuations need a class the
                # expert does not have, and end with no entry)
                check_layout(got, B, W, S, lexicon, may_be_empty=classes[g] < 331)
                if g < 3 and not dead:                                      # (the later experts repeat the class counts)
                    ref = decoding.attn_lexicon_host(sds[g], Hb[g].cpu(), SOS, EOS, W, S - 1, trie, want_margin=True)
                    check_reference(f"G={G} expert {g} ({classes[g]} classes)", got, ref)
                    assert np.all(got[0][got[1] >= 0] < classes[g])
                if dead:
                    tokens, length, score, logp, path, prob, word = got
                    assert np.all(length == -1) and np.all(np.isneginf(score)) and np.all(word == -1) and np.all(tokens == EOS)
                    assert np.all(path == EOS) and np.all(prob == 1.0) and np.all(logp == 0)


def test_fused_and_stepwise_agree(ops, monkeypatch):
    """the step loop on the B * W-row batch with the ragged expand of the trie against the fused launch, on decisive samples"""
    name = "c97_w4"
    B, T, D, C, S, W, *_rest = LEXICON_CASES[name]
    sd, Hb, words, trie, ref = lexicon_case(name)
    att = module(sd, D, C)
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    fused = search(ops, att, Hb, W, S, trie)
    monkeypatch.setenv("MRN_ATTN_BEAM", "stepwise")
    handle = ops.upload_trie(trie, "cuda")
    assert not att.lexicon_fused(D, T, S, EOS, W, handle)
    step, names = recorded_calls(monkeypatch, lambda: to_np(att.lexicon_search(Hb.cuda(), SOS, EOS, W, handle, S - 1)))
    assert not [n for n in names if n.startswith("mrn_attn_lexicon") or n.startswith("mrn_attn_beam")]
    check_layout(step, B, W, S, words)
    check_self_consistent(att, Hb, step[:6])
    check_reference(name + " stepwise", step, ref)
    for b in np.flatnonzero(decisive(ref[7])):
        assert np.array_equal(fused[0][b], step[0][b]) and np.array_equal(fused[1][b], step[1][b]) and np.array_equal(fused[6][b], step[6][b])
        assert np.all(np.abs(fused[2][b] - step[2][b]) <= 2 * fused[1][b] * TOKEN_BAND)


def test_context_over_the_budget_goes_stepwise(ops, monkeypatch):
    """D = 2304 does not fit the whole-context tile: no lexicon launch, the step loop, still self-consistent and all lexicon words"""
    from mrn_amd.modules import decoding
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    B, T, D, C, S, W = 5, 65, 2304, 203, 6, 4
    sd, Hb = beam_fixture(B, T, D, C, 500, 50.0)
    words = draw_lexicon(C, S, 500, 200, 2, False)
    trie = decoding.build_trie(*as_arrays(words))
    att = module(sd, D, C)
    handle = ops.upload_trie(trie, "cuda")
    assert not ops.attn_lexicon_whole_context(D, T, W) and not att.lexicon_fused(D, T, S, EOS, W, handle)
    got, names = recorded_calls(monkeypatch, lambda: to_np(att.lexicon_search(Hb.cuda(), SOS, EOS, W, handle, S - 1)))
    assert not [n for n in names if n.startswith("mrn_attn_lexicon") or n.startswith("mrn_attn_beam")]
    assert names.count("mrn_embed_gather_f32") == S
    check_layout(got, B, W, S, words)
    check_self_consistent(att, Hb, got[:6])


def test_calls_outside_the_limits_are_errors(ops, monkeypatch):
    """W = 17, S = 513, a trie deeper than S - 1, a null trie array: an error code from the argument checks, which stand before the
    first launch (tests/test_attn_lexicon_cpu.py::test_rule_matches_the_launch_helper); a malformed trie never reaches the library"""
    from mrn_amd.modules import decoding
    B, T, D, C, S, _ = CASES["c97"]
    sd, Hb, _ = case("c97")
    att = module(sd, D, C)
    trie = decoding.build_trie(*as_arrays([(5, 6, 7), (8,), (5, 9)]))
    handle = ops.upload_trie(trie, "cuda")
    with torch.no_grad():
        Hproj = ops.linear(Hb.cuda(), att.attention_cell.i2h.weight)
        args = att.greedy_args()

        def run(S=S, eos=EOS, W=4, hidden=HID, handle=handle):
            return ops.attn_lexicon_decode(Hb.cuda(), Hproj, args[0], sos(SOS), *args[1:9], hidden, S, eos, W, handle, w_inv=args[9])

        assert len(run()) == 7
        for kw, msg in (({"W": 17}, "beam width W=17"), ({"W": 0}, "beam width W=0"), ({"S": 513}, "S=513"), ({"hidden": 128}, "hidden=128"),
                        ({"eos": C}, "eos="), ({"S": 3}, "trie depth=3")):
            with pytest.raises(RuntimeError, match=r"failed \(code -1\).*" + msg):
                run(**kw)
        null = ops.upload_trie(trie, "cuda")
        null.child_tok = torch.empty(0, dtype=torch.int32, device="cuda")          # data_ptr() == 0
        with pytest.raises(RuntimeError, match=r"failed \(code -1\).*null trie operand"):
            run(handle=null)
        with pytest.raises(ValueError, match="upload_trie"):
            run(handle=trie)
        with pytest.raises(ValueError, match="upload_trie"):
            run(handle=None)
        _, names = recorded_calls(monkeypatch, lambda: pytest.raises(ValueError, ops.upload_trie, trie._replace(
            child_node=np.array([1, 2, 3, 9, 5], dtype=np.int32)), "cuda"))
        assert names == []
        with pytest.raises(ValueError, match="longest word"):
            att.lexicon_search(Hb.cuda(), SOS, EOS, 4, handle, 2)
    torch.cuda.synchronize()


# ---- the evaluation forwards and validation() --------------------------------------------------------------------------------------
WORDS = ["beam", "search", "a1", "", "mi355x", "lds", "wave64", "x", "beams", "sea", "lds", "Wave", "a-1", "waves", "b", "m1", "z9q",
         "0", "abcdefghijklmnopqrstuvwxyz"]


@pytest.mark.parametrize("kind", ["mrn", "model"])
def test_validation_decodes_along_the_lexicon(ops, monkeypatch, kind):
    """attn_lexicon: every returned prediction is a lexicon word; the loss is the default run's bit for bit; accuracy, NED and the
    confidences are those of the (routed expert's) reference best entry for decisive samples; device and host scoring agree; one
    lexicon launch per heads group; without the key, or with None, every value is today's.  infer_time, a wall-clock time, is the one
    value of the eight left out"""
    from mrn_amd.modules import decoding
    from mrn_amd.test import validation
    from mrn_amd.tools.utils import AttnLabelConverter
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    monkeypatch.delenv("MRN_VALIDATION_SCORING", raising=False)
    net, plain, image = trba_nets()
    model, choose = (net, "TF") if kind == "mrn" else (plain, "val")
    conv = AttnLabelConverter(CHARACTERS)
    B, W, L = len(LABELS), 4, 25

    def run(**kw):
        def go():
            with torch.no_grad():
                return validation(model, None, [(image, list(LABELS))], conv, trba_opt(NED=True, **kw), val_choose=choose)
        res, names = recorded_calls(monkeypatch, go)
        return res[:6] + res[7:], names

    absent, names0 = run()
    none, _ = run(attn_lexicon=None)
    assert absent == none and not [n for n in names0 if "lexicon" in n or "attn_beam" in n]
    lex, names = run(attn_lexicon=WORDS)
    assert sum(n.startswith("mrn_attn_lexicon_decode") for n in names) == 1 and not [n for n in names if n.startswith("mrn_attn_beam")]
    assert lex[0] == absent[0]                                             # valid_loss: the greedy decoder's logits
    assert run(attn_lexicon=WORDS, attn_decode="greedy")[0] == lex and run(attn_lexicon=WORDS, attn_decode="beam")[0] == lex
    assert run(attn_lexicon=WORDS, lexicon=["zz"])[0] == lex               # opt.lexicon stays the CTC heads'
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "host")
    host, _ = run(attn_lexicon=WORDS)
    monkeypatch.delenv("MRN_VALIDATION_SCORING")
    assert host == lex
    tokens, lengths, kept = decoding.encode_attn_lexicon(conv, WORDS, L)
    assert kept == [w for w in WORDS if w not in ("Wave", "a-1", "abcdefghijklmnopqrstuvwxyz")]
    trie = decoding.build_trie(tokens, lengths)
    # the returned strings are the unpruned decode of all S steps: the word, then [EOS] to the end
    for text in lex[3]:
        assert text[:text.find("[EOS]")] in kept and text.replace("[EOS]", "") == text[:text.find("[EOS]")]
    # the reference: attn_lexicon_host on the features of the expert the routing picks
    handle = ops.upload_trie(trie, "cuda")
    sos_t = torch.full((B,), 2, dtype=torch.long).cuda()
    with torch.no_grad():
        if kind == "mrn":
            out = model(image.cuda(), True, sos_t, False, attn_beam=W, attn_lexicon=handle)
            index = out["index"].view(-1).cpu().numpy()
            experts = list(model.model)
            feats = [e(image.cuda(), sos_t, False)["feature"].cpu() for e in experts]
            with pytest.raises(ValueError, match="attn_beam"):
                model(image.cuda(), True, sos_t, False, attn_lexicon=handle)
        else:
            out = model(image.cuda(), sos_t, False, attn_beam=W, attn_lexicon=handle)
            index, experts = np.zeros(B, dtype=np.int64), [model]
            feats = [out["feature"].cpu()]
            with pytest.raises(ValueError, match="attn_beam"):
                model(image.cuda(), sos_t, False, attn_lexicon=handle)
    refs = [decoding.attn_lexicon_host(e.Prediction.state_dict(), f, 2, 3, W, L, trie, want_margin=True) for e, f in zip(experts, feats)]
    path, prob, word = out["beam_path"].cpu().numpy(), out["beam_prob"].cpu().numpy(), out["beam_word"].cpu().numpy()
    assert path.shape == (B, L + 1) and prob.shape == (B, L + 1) and word.shape == (B,)
    checked = correct = 0
    ned = 0.0
    all_decisive = True
    from mrn_amd.test import edit_distance
    for b in range(B):
        ref = refs[int(index[b])]
        if not decisive(ref[7])[b]:
            all_decisive = False
            continue
        checked += 1
        assert np.array_equal(path[b], ref[4][b]) and word[b] == ref[6][b, 0], b
        best = kept[ref[6][b, 0]] if ref[6][b, 0] >= 0 else ""
        assert lex[3][b].startswith(best + "[EOS]")
        want, n_kept = kept_confidence(conv, ref, b)
        print(f"sample {b}: expert {int(index[b])}, word {best!r}, confidence {lex[4][b]:.6e}, reference {want:.6e}")
        assert abs(lex[4][b] - want) <= want * (np.exp(max(n_kept, 1) * TOKEN_BAND) - 1) + 1e-12, b
        correct += best == LABELS[b]
        if len(best) and len(LABELS[b]):
            ned += 1 - edit_distance(best, LABELS[b]) / max(len(best), len(LABELS[b]))
    print(f"{checked} decisive samples of {B}")
    assert checked >= 1
    if all_decisive:
        assert lex[1] == correct / B * 100 and abs(lex[2] - ned / B * 100) < 1e-9
    # a CRNN head ignores the key; a lexicon none of whose words can be spelled is an error
    with pytest.raises(ValueError, match="attn_lexicon: none of the"):
        run(attn_lexicon=["ÄÖ", "Wave", "abcdefghijklmnopqrstuvwxyz0"])
    with pytest.raises(ValueError, match="attn_lexicon must be a sequence"):
        run(attn_lexicon="beam")


def test_a_ctc_head_ignores_the_key(monkeypatch):
    from tests.test_ctc_beam_gpu import run_validation
    base = run_validation(monkeypatch)
    for keys in ({"attn_lexicon": WORDS}, {"attn_lexicon": None}):
        res = run_validation(monkeypatch, **keys)
        assert res[:6] + res[7:] == base[:6] + base[7:]
