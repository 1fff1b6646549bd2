"""The lexicon protocol on the decoders: Attention.shortlist_search, the CTC heads' pair, the evaluation forwards' attn_shortlist= and
validation()'s opt.lexicon_shortlist.  The shortlist kernel itself is held to the host form in tests/test_shortlist_gpu.py; here every
path must equal the composition of its parts bit for bit (the same kernels on the same operands: no tolerance), and with every word
kept validation() must return what opt.candidates returns with the whole list for every image.

The file's name puts it behind tests/test_bench_gpu.py in the suite, as the beam, lexicon and candidate files' do: that file starts
bench.py from a process that has not touched the GPU yet, and skips otherwise."""
import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import EOS, SOS, beam_fixture
from tests.test_attn_lexicon_cpu import LEXICON_CASES, as_arrays, draw_lexicon
from tests.test_greedy_decode_gpu import decode, module, sos

pytestmark = pytest.mark.gpu
WORDS = ["beam", "search", "a1", "mi355x", "lds", "wave64", "x", "beams", "bean", "sea", "wave", "lds9", "", "mi300x", "y", "wave32"]
LAUNCHES = ("greedy_decode", "shortlist", "score_candidates", "attn_beam", "lexicon_decode")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def recorded_calls(monkeypatch, fn):
    """(fn(), the names of the library calls it made)"""
    from mrn_amd._lib import LIB
    names, real = [], LIB.call
    monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.setattr(LIB, "call", real)


def decoder_launches(names):
    return [m for m in names if any(k in m for k in LAUNCHES)]


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("name", ["c97_w4", "c37_w3"])
def test_shortlist_search_is_the_composition_of_its_parts(ops, monkeypatch, name, x3):
    """the fused greedy decode, lexicon_shortlist_host on its tokens before the first eos, score_candidates on that table"""
    from mrn_amd.modules import decoding
    for key in ("MRN_ATTN_BEAM", "MRN_GREEDY_DECODE"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, W, seed0, scale, n, shortest, empty = LEXICON_CASES[name]
    sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
    tokens, lengths = as_arrays(draw_lexicon(C, S, seed0, n, shortest, empty))
    att = module(sd, D, C)
    handle = ops.upload_words(tokens, lengths, "cuda", 2)
    _, greedy = decode(ops, att, Hb.cuda(), sos(SOS), S, want_tokens=True)
    hyp, hyp_len = decoding.hypothesis_of_path(greedy.cpu().numpy(), EOS)
    for K, max_dist in ((20, None), (7, 6)):
        with torch.no_grad():
            got, names = recorded_calls(monkeypatch, lambda: att.shortlist_search(Hb.cuda(), SOS, EOS, handle, K, max_dist, S - 1, want_logp=True))
        ran = decoder_launches(names)
        assert len(ran) == 3 and "greedy_decode" in ran[0] and ran[1] == "mrn_lexicon_shortlist_i32"
        assert ran[2] == ("mrn_attn_score_candidates_x3_grouped" if x3 else "mrn_attn_score_candidates_grouped_f32")
        cand, dist = decoding.lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, K, max_dist)
        parts = att.score_candidates(Hb.cuda(), SOS, EOS, handle.with_cand(cand, S), S - 1, want_logp=True)
        assert len(got) == 8 and len(parts) == 6
        for g, p in zip(got, parts):
            assert torch.equal(g, p)
        assert np.array_equal(got[6].cpu().numpy(), cand) and np.array_equal(got[7].cpu().numpy(), dist)
        assert got[6].dtype == torch.int32 and tuple(got[6].shape) == (B, K)
        # the greedy tokens handed in: no greedy launch, the same result
        with torch.no_grad():
            again, names = recorded_calls(monkeypatch, lambda: att.shortlist_search(Hb.cuda(), SOS, EOS, handle, K, max_dist, S - 1, want_logp=True,
                                                                                     tokens=greedy))
        assert [m for m in decoder_launches(names) if "greedy" in m] == [] and all(torch.equal(a, g) for a, g in zip(again, got))
    # tokens with an eos in every second row: the hypothesis is what stands before it
    cut = greedy.clone()
    cut[::2, 3] = EOS
    cut[1, 0] = EOS
    hyp, hyp_len = decoding.hypothesis_of_path(cut.cpu().numpy(), EOS)
    assert hyp_len[1] == 0 and hyp_len[0] <= 3
    cand, dist = decoding.lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, 9)
    with torch.no_grad():
        got = att.shortlist_search(Hb.cuda(), SOS, EOS, handle, 9, None, S - 1, tokens=cut)
    assert np.array_equal(got[5].cpu().numpy(), cand) and np.array_equal(got[6].cpu().numpy(), dist)
    with pytest.raises(ValueError, match="upload_words"):
        att.shortlist_search(Hb.cuda(), SOS, EOS, (tokens, lengths), 5, None, S - 1)


def crnn_words(conv, batches):
    chars = conv.character[4:]
    labels = [gt for _, gt_list in batches for gt in gt_list]
    near = [gt[:-1] + chars[(chars.index(gt[-1]) + 3) % len(chars)] for gt in labels] + [gt[:-1] for gt in labels] + [gt + chars[2] for gt in labels[:5]]
    return list(dict.fromkeys(w for w in labels + near + [chars[5] * 3, chars[7] * 9] if w)), labels


def test_the_ctc_pair_is_the_composition_of_its_parts(ops, monkeypatch):
    """arg-max per frame, collapsed; lexicon_shortlist_host on it; ops.ctc_lexicon_decode(cand=) on that table"""
    from mrn_amd.modules import decoding
    from mrn_amd.test import _Lexicon
    from tests.test_ctc_beam_gpu import validation_case
    _, conv, _, opt, batches, logits = validation_case()
    words, _ = crnn_words(conv, batches)
    preds = torch.from_numpy(logits[1]).cuda()
    hyp, hyp_len = decoding.hypothesis_of_frames(logits[1].argmax(axis=2))
    for K, max_dist in ((6, None), (4, 0), (len(words) + 2, 2)):
        lex = _Lexicon(conv, words, 2, (K, max_dist))
        got, names = recorded_calls(monkeypatch, lambda: lex.pair(preds, "CTC"))
        assert [m for m in names if "lexicon" in m] == ["mrn_lexicon_shortlist_i32", "mrn_ctc_lexicon_decode_f32"]
        cand, _ = decoding.lexicon_shortlist_host(hyp, hyp_len, lex.tokens, lex.lengths, K, max_dist)
        dev = [torch.from_numpy(a).cuda() for a in (lex.tokens, lex.lengths, cand)]
        path, prob = ops.ctc_lexicon_decode(preds, dev[0], dev[1], n=2, cand=dev[2])[3:]
        assert torch.equal(got[0], path) and torch.equal(got[1], prob)
        empty = (cand < 0).all(axis=1)
        assert not (max_dist is None and empty.any())
        assert (got[0][torch.from_numpy(empty).cuda()] == 0).all() and (got[1][torch.from_numpy(empty).cuda(), 0] == 0).all()


def test_validation_on_a_crnn(monkeypatch):
    """lexicon + lexicon_shortlist with every word kept returns what candidates returns with the whole lexicon for every image; without
    the option the values and the library calls are the lexicon decoder's"""
    from tests.test_ctc_beam_gpu import run_validation, validation_case
    from tests.test_scoring_gpu import recorded_calls as recorded
    _, conv, _, _, batches, _ = validation_case()
    words, labels = crnn_words(conv, batches)
    values = (0, 1, 2, 3, 4, 5, 7)                                              # all but infer_time, which is a clock reading
    with recorded() as log:
        got = run_validation(monkeypatch, lexicon=words, lexicon_shortlist=len(words), lexicon_top_n=2)
    assert log.count("mrn_lexicon_shortlist_i32") == len(batches) == log.count("mrn_ctc_lexicon_decode_f32")
    whole = run_validation(monkeypatch, candidates={gt: words for gt in labels}, lexicon_top_n=2)
    host_scored = run_validation(monkeypatch, scoring="host", lexicon=words, lexicon_shortlist=len(words) + 5, lexicon_top_n=2)
    for i in values:
        assert got[i] == whole[i] == host_scored[i], i
    with recorded() as log_absent:
        absent = run_validation(monkeypatch, lexicon=words, lexicon_top_n=2)
    with recorded() as log_none:
        none = run_validation(monkeypatch, lexicon=words, lexicon_top_n=2, lexicon_shortlist=None, lexicon_max_distance=None)
    assert log_absent == log_none and "mrn_lexicon_shortlist_i32" not in log_none and log_none.count("mrn_ctc_lexicon_decode_f32") == len(batches)
    for i in values:
        assert absent[i] == none[i], i
    assert absent[0] == got[0]                                                  # valid_loss: the logits do not change
    near = run_validation(monkeypatch, lexicon=words, lexicon_shortlist=3, lexicon_max_distance=0)
    assert near[7] == 16 and set(near[3]) <= set(words) | {""}
    with pytest.raises(ValueError, match="words of lexicon"):
        run_validation(monkeypatch, lexicon_shortlist=3)
    with pytest.raises(ValueError, match="lexicon_shortlist and candidates"):
        run_validation(monkeypatch, lexicon=words, lexicon_shortlist=3, candidates={gt: words for gt in labels})


@pytest.mark.parametrize("kind", ["mrn", "model"])
def test_validation_on_a_trba(ops, monkeypatch, kind):
    """attn_lexicon + lexicon_shortlist with every word kept returns what candidates returns with the whole lexicon for every image: one
    shortlist launch and one scoring launch per batch, no beam; beam_width is not read.  Without the option the values and the library
    calls are the trie beam's"""
    from mrn_amd.test import validation
    from mrn_amd.tools.utils import AttnLabelConverter
    from tests.test_decode_attn_beam_gpu import CHARACTERS, LABELS, trba_nets, trba_opt
    for key in ("MRN_ATTN_BEAM", "MRN_GREEDY_DECODE", "MRN_VALIDATION_SCORING"):
        monkeypatch.delenv(key, raising=False)
    net, plain, image = trba_nets()
    model, choose = (net, "TF") if kind == "mrn" else (plain, "val")
    conv = AttnLabelConverter(CHARACTERS)
    batches = [(image[:5], list(LABELS[:5])), (image[5:], list(LABELS[5:]))]

    def run(**kw):
        def go():
            with torch.no_grad():
                return validation(model, None, batches, conv, trba_opt(NED=True, **kw), val_choose=choose)
        res, names = recorded_calls(monkeypatch, go)
        return res[:6] + res[7:], names

    got, names = run(attn_lexicon=WORDS, lexicon_shortlist=len(WORDS) + 3, lexicon_top_n=2)
    ran = decoder_launches(names)
    assert ran.count("mrn_lexicon_shortlist_i32") == len(batches) and sum("score_candidates" in m for m in ran) == len(batches)
    assert not [m for m in ran if "attn_beam" in m or "lexicon_decode" in m]
    whole, _ = run(candidates={gt: WORDS for gt in LABELS}, lexicon_top_n=2)
    assert got == whole
    other = trba_opt(NED=True, attn_lexicon=WORDS, lexicon_shortlist=len(WORDS), lexicon_top_n=2)
    other.beam_width = 1
    with torch.no_grad():
        res = validation(model, None, batches, conv, other, val_choose=choose)
    assert res[:6] + res[7:] == got
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "host")
    assert run(attn_lexicon=WORDS, lexicon_shortlist=len(WORDS), lexicon_top_n=2)[0] == got
    monkeypatch.delenv("MRN_VALIDATION_SCORING")
    absent, names_absent = run(attn_lexicon=WORDS)
    none, names_none = run(attn_lexicon=WORDS, lexicon_shortlist=None, lexicon_max_distance=None)
    assert absent == none and names_absent == names_none and absent[0] == got[0]
    assert sum("attn_lexicon_decode" in m for m in names_none) == len(batches) and not [m for m in names_none if "shortlist" in m or "score_candidates" in m]
    near, _ = run(attn_lexicon=WORDS, lexicon_shortlist=2, lexicon_max_distance=1)
    assert all(s.replace("[EOS]", "") in WORDS for s in near[3])
    with pytest.raises(ValueError, match="words of attn_lexicon"):
        run(lexicon=WORDS, lexicon_shortlist=3)
    with pytest.raises(ValueError, match="lexicon_shortlist and candidates"):
        run(attn_lexicon=WORDS, lexicon_shortlist=3, candidates={gt: WORDS for gt in LABELS})


def test_mrnnet_shortlists_on_the_routed_experts_hypothesis(ops, monkeypatch):
    """three experts of 30, 36 and 41 classes: the candidate table is the shortlist of the arg-max of the ROUTED logits, one table per
    batch, scored under all experts as attn_candidates= scores it -- so the forward with attn_shortlist equals the forward with
    attn_candidates on the host form's table, bit for bit.  A word with a class the routed expert lacks is a dead slot there"""
    import contextlib
    import io
    from mrn_amd.modules import decoding
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as Wt
    from mrn_amd.tools.utils import AttnLabelConverter
    from tests.test_decode_attn_beam_gpu import CHARACTERS, LABELS, trba_nets, trba_opt
    for key in ("MRN_ATTN_BEAM", "MRN_GREEDY_DECODE"):
        monkeypatch.delenv(key, raising=False)
    opt = trba_opt()
    classes = (30, 36, 5 + len(CHARACTERS))
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(256, c)
            net.build_prediction(opt, c)
    Wt.fill_state_dict(net.state_dict(), seed=13)
    with torch.no_grad():
        for e in net.model:
            e.Prediction.generator.weight.mul_(40.0)
    net = net.cuda().eval()
    _, plain, image = trba_nets()
    conv = AttnLabelConverter(CHARACTERS)
    B, L, K = len(LABELS), 25, 6
    tokens, lengths, kept = decoding.encode_attn_lexicon(conv, WORDS, L)
    assert kept == WORDS and tokens.max() >= classes[1] > classes[0]            # words the first two experts cannot spell
    handle = ops.upload_words(tokens, lengths, "cuda", 2)
    sos_t = torch.full((B,), 2, dtype=torch.long).cuda()
    for model, call in ((net, lambda **kw: net(image.cuda(), True, sos_t, False, **kw)), (net, lambda **kw: net(image.cuda(), False, sos_t, False, **kw)),
                        (plain, lambda **kw: plain(image.cuda(), sos_t, False, **kw))):
        with torch.no_grad():
            base = call()
            out, names = recorded_calls(monkeypatch, lambda: call(attn_shortlist=(handle, K, None)))
            logits = base["logits"] if "logits" in base else base["predict"]
            hyp, hyp_len = decoding.hypothesis_of_path(logits.argmax(dim=2).cpu().numpy(), 3)
            cand, _ = decoding.lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, K)
            ref = call(attn_candidates=handle.with_cand(cand, L + 1))
        ran = decoder_launches(names)
        assert ran.count("mrn_lexicon_shortlist_i32") == 1 and sum("score_candidates" in m for m in ran) >= 1
        assert not [m for m in ran if "attn_beam" in m or "lexicon_decode" in m]
        assert torch.equal(out["logits"] if "logits" in out else out["predict"], logits) and "beam_path" not in base
        for key in ("beam_path", "beam_prob", "beam_word"):
            assert torch.equal(out[key], ref[key]), key
        if base.get("index") is not None:
            assert torch.equal(out["index"], base["index"])
            routed = np.array(classes)[base["index"].view(-1).cpu().numpy()]
            word = out["beam_word"].cpu().numpy()
            for b in range(B):
                assert word[b] == -1 or tokens[word[b], :lengths[word[b]]].max(initial=0) < routed[b], b
    with torch.no_grad():
        with pytest.raises(ValueError, match="pass one"):
            net(image.cuda(), True, sos_t, False, attn_beam=4, attn_shortlist=(handle, K, None))
        with pytest.raises(ValueError, match="attn_shortlist must be"):
            plain(image.cuda(), sos_t, False, attn_shortlist=handle)
