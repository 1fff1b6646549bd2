"""Exact scoring of per-sample candidate words on the attention head in one launch (mrn_attn_score_candidates_*, csrc/attn_decode.hip
attn_score_kernel) against the float64 form mrn_amd/modules/decoding.py::attn_candidates_host, and validation()'s per-image lexicons.

The band is the beam tests': a token's log-probability is held to TOKEN_BAND = 2e-4, a score of L + 1 tokens to (L + 1) * TOKEN_BAND.  A
sample is decisive when the two best scores of the float64 form differ by at least three bands of the longer word; decisive samples must
match it exactly in the best word, its path and (within the band) its probabilities.  tests/test_attn_candidates_cpu.py holds the cases
and checks on the CPU that at most B // 4 samples of a case are not decisive.

The file's name puts it behind tests/test_bench_gpu.py in the suite, as the beam and lexicon files' do: that file starts bench.py from a
process that has not touched the GPU yet, and skips otherwise."""
import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import EOS, SOS, TOKEN_BAND, beam_fixture
from tests.test_attn_candidates_cpu import CAND_CASES, cand_case, decisive_samples
from tests.test_attn_lexicon_cpu import as_arrays, draw_lexicon
from tests.test_greedy_decode_gpu import HID, decode, module, sos

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def to_np(res):
    return tuple(r.cpu().numpy() for r in res)


def recorded_calls(monkeypatch, fn):
    """(fn(), the names of the library calls it made)"""
    from mrn_amd._lib import LIB
    names, real = [], LIB.call
    monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.setattr(LIB, "call", real)


def handle_of(ops, tokens, lengths, cand, S, n):
    return ops.upload_words(tokens, lengths, "cuda", n).with_cand(cand, S)


def check_against_host(name, got, ref, words, cand, S, n):
    """layout, every live element inside its band, dead slots exact, the best entry of decisive samples"""
    index, score, score_all, path, prob, logp = got
    r_index, r_score, r_all, r_path, r_prob, r_logp = ref
    B, K = cand.shape
    assert index.shape == (B, n) and index.dtype == np.int32 and score.shape == (B, n) and score.dtype == np.float32
    assert score_all.shape == (B, K) and score_all.dtype == np.float32 and logp.shape == (B, K, S) and logp.dtype == np.float32
    assert path.shape == (B, S) and path.dtype == np.int64 and prob.shape == (B, S) and prob.dtype == np.float32
    dead = np.isneginf(r_all)
    assert np.array_equal(np.isneginf(score_all), dead) and np.all(np.isfinite(score_all[~dead])) and np.all(logp[dead] == 0)
    worst = 0.0
    for b in range(B):
        for k in np.flatnonzero(~dead[b]):
            L = len(words[cand[b, k]])
            err = abs(score_all[b, k] - r_all[b, k])
            worst = max(worst, err / ((L + 1) * TOKEN_BAND))
            assert err <= (L + 1) * TOKEN_BAND, (name, b, k, err)
            assert np.all(np.abs(logp[b, k, :L + 1] - r_logp[b, k, :L + 1]) <= TOKEN_BAND), (name, b, k)
            assert np.all(logp[b, k, L + 1:] == 0)
        live = int((~dead[b]).sum())
        assert np.all(index[b, min(live, n):] == -1) and np.all(np.isneginf(score[b, min(live, n):]))       # dead slots last
        assert np.all(index[b, :min(live, n)] >= 0) and np.all(np.diff(score[b, :min(live, n)]) <= 0)
        for r in range(min(live, n)):                                           # a ranked entry is one of the row's slots with its score
            assert np.any((cand[b] == index[b, r]) & (score_all[b] == score[b, r])), (name, b, r)
    print(f"{name}: worst score error {worst:.3f} of its band")
    decisive = decisive_samples(words, cand, r_all)
    for b in np.flatnonzero(decisive):
        assert index[b, 0] == r_index[b, 0] and np.array_equal(path[b], r_path[b]), (name, b)
        if r_index[b, 0] < 0:
            assert np.all(prob[b] == 0) and np.all(path[b] == EOS)
            continue
        L = len(words[r_index[b, 0]])
        assert np.all(np.abs(prob[b] - r_prob[b]) <= r_prob[b] * (np.exp(TOKEN_BAND) - 1) + 1e-37), (name, b)
        assert np.all(prob[b, L + 1:] == 1.0)
    print(f"{name}: {int(decisive.sum())} decisive samples of {B}")
    assert decisive.sum() >= B - B // 4


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("name", list(CAND_CASES))
def test_kernel_matches_the_host_form(ops, monkeypatch, name, x3):
    """the fused launch, both forms: the float64 form, duplicates bit-equal, a permuted row the permuted scores bit for bit"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, K, _, _ = CAND_CASES[name]
    sd, Hb, words, tokens, lengths, cand, ref = cand_case(name)
    n = ref[0].shape[1]
    att = module(sd, D, C)
    assert att.score_fused(D, T, S, EOS, n)
    got, names = recorded_calls(monkeypatch, lambda: to_np(att.score_candidates(Hb.cuda(), SOS, EOS, handle_of(ops, tokens, lengths, cand, S, n),
                                                                                S - 1, want_logp=True)))
    assert [m for m in names if "score" in m or "beam" in m] == ["mrn_attn_score_candidates_x3_grouped" if x3 else
                                                                 "mrn_attn_score_candidates_grouped_f32"]
    check_against_host(name, got, ref, words, cand, S, n)
    score_all, logp = got[2], got[5]
    for b in range(B):                                                         # the same word in two slots: the same bits
        for i in range(K):
            for k in range(i + 1, K):
                if cand[b, i] >= 0 and cand[b, k] >= 0 and words[cand[b, i]] == words[cand[b, k]]:
                    assert score_all[b, i] == score_all[b, k] and np.array_equal(logp[b, i], logp[b, k]), (b, i, k)
    perm = np.random.default_rng(3).permutation(K)
    again = to_np(att.score_candidates(Hb.cuda(), SOS, EOS, handle_of(ops, tokens, lengths, np.ascontiguousarray(cand[:, perm]), S, n), S - 1,
                                       want_logp=True))
    assert np.array_equal(again[2], score_all[:, perm]) and np.array_equal(again[5], logp[:, perm])


@pytest.mark.parametrize("x3", [True, False])
def test_a_row_fed_the_greedy_decode_reproduces_the_greedy_logits(ops, monkeypatch, x3):
    """the word of a sample = the first S - 1 tokens of its greedy decode: the row's inputs are the greedy kernel's, so its logits are the
    greedy kernel's bit for bit, and logp is the log-softmax of attn_greedy_decode's logits at the targets (the greedy tokens, then eos)
    up to the float32 rounding of the log-sum-exp.  That bound, for C classes and unit round-off u = 2^-24: the sum of C exponentials
    carries a relative error of at most (C + 2) u (expf to 2 ulp, C - 1 additions), its logarithm that much absolutely, plus one
    rounding each of logf, the addition of the maximum and the subtraction from the target's logit, each at most u times the largest
    of |lse|, |lp| and 1"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, K, seed0, scale = CAND_CASES["k16"]
    sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
    att = module(sd, D, C)
    logits, greedy = decode(ops, att, Hb.cuda(), sos(SOS), S, want_tokens=True)
    greedy = greedy.cpu().numpy()
    tokens = np.ascontiguousarray(greedy[:, :S - 1], dtype=np.int32)
    lengths = np.full(B, S - 1, dtype=np.int32)
    cand = np.full((B, 2), -1, dtype=np.int32)
    cand[:, 1] = np.arange(B)
    got = to_np(att.score_candidates(Hb.cuda(), SOS, EOS, handle_of(ops, tokens, lengths, cand, S, 1), S - 1, want_logp=True))
    x = logits.cpu().numpy().astype(np.float64)
    peak = x.max(axis=2, keepdims=True)
    lse = (peak + np.log(np.exp(x - peak).sum(axis=2, keepdims=True)))[:, :, 0]
    target = np.concatenate([greedy[:, :S - 1], np.full((B, 1), EOS)], axis=1)
    want = np.take_along_axis(x, target[:, :, None], axis=2)[:, :, 0] - lse
    u = 2.0 ** -24
    bound = (C + 2) * u + 3 * u * np.maximum(np.maximum(np.abs(lse), np.abs(want)), 1.0)
    err = np.abs(got[5][:, 1] - want)
    print(f"largest error {err.max():.3e}, {np.max(err / bound):.3f} of its bound")
    assert np.all(err <= bound)
    assert np.all(np.abs(got[2][:, 1] - want.sum(axis=1)) <= bound.sum(axis=1) + S * u * np.abs(want).sum(axis=1))
    assert np.all(np.isneginf(got[2][:, 0])) and np.array_equal(got[0][:, 0], np.arange(B))


def test_fused_and_stepwise_agree(ops, monkeypatch):
    """the teacher-forced decoder on the (sample, slot) rows, in chunks, against the fused launch: within twice the band, the same dead
    slots, no scorer launch"""
    name = "k17"
    B, T, D, C, S, K, _, _ = CAND_CASES[name]
    sd, Hb, words, tokens, lengths, cand, ref = cand_case(name)
    n = ref[0].shape[1]
    att = module(sd, D, C)
    handle = handle_of(ops, tokens, lengths, cand, S, n)
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    fused = to_np(att.score_candidates(Hb.cuda(), SOS, EOS, handle, S - 1, want_logp=True))
    monkeypatch.setenv("MRN_ATTN_BEAM", "stepwise")
    monkeypatch.setattr(type(att), "SCORE_ROWS_BYTES", 1 << 20)                # several chunks of rows, one ending inside a sample
    assert not att.score_fused(D, T, S, EOS, n)
    step, names = recorded_calls(monkeypatch, lambda: to_np(att.score_candidates(Hb.cuda(), SOS, EOS, handle, S - 1, want_logp=True)))
    assert not [m for m in names if m.startswith("mrn_attn_score")] and names.count("mrn_embed_gather_f32") > 1
    check_against_host(name + " stepwise", step, ref, words, cand, S, n)
    dead = np.isneginf(fused[2])
    assert np.array_equal(dead, np.isneginf(step[2]))
    for b in range(B):
        for k in np.flatnonzero(~dead[b]):
            L = len(words[cand[b, k]])
            assert abs(fused[2][b, k] - step[2][b, k]) <= 2 * (L + 1) * TOKEN_BAND, (b, k)
            assert np.all(np.abs(fused[5][b, k] - step[5][b, k]) <= 2 * TOKEN_BAND)


@pytest.mark.parametrize("x3", [True, False])
def test_grouped_equals_single_launches(ops, monkeypatch, x3):
    """three experts of 37 / 97 / 331 classes on their own features, one word table over the 331-class alphabet, one launch: every
    group bit-identical to its single launch; a word with a class an expert lacks is dead for that expert alone"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, S, K, n = 5, 17, 8, 6, 2
    classes = (37, 97, 331)
    sds, atts, Hbs = [], [], []
    for g, C in enumerate(classes):
        sd, Hb = beam_fixture(B, T, 256, C, 700 + 40 * g, 100.0)
        sds.append(sd)
        atts.append(module(sd, 256, C))
        Hbs.append(Hb)
    Hb = torch.stack(Hbs).cuda()
    words = list(dict.fromkeys(draw_lexicon(331, S, 900, 40, 0, True)))
    assert any(max(w, default=0) >= 97 for w in words) and any(37 <= max(w, default=0) < 97 for w in words) and any(max(w, default=0) < 37 for w in words)
    tokens, lengths = as_arrays(words)
    cand = np.stack([np.random.default_rng(b).permutation(len(words))[:K] for b in range(B)]).astype(np.int32)
    cand[0, 2] = -1
    handle = handle_of(ops, tokens, lengths, cand, S, n)
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
        table = (handle.tokens_dev, handle.lengths_dev, handle.cand_dev)
        grouped = ops.attn_score_candidates_grouped(Hb, Hproj, cols[0], sos(SOS), *cols[1:9], HID, S, EOS, *table, n=n, want_logp=True,
                                                    w_inv=cols[9] if x3 else None)
        assert len(grouped) == 6 and grouped[2].shape == (3, B, K) and (cols[9][0] is not None) == x3
        for g, C in enumerate(classes):
            one = ops.attn_score_candidates(Hb[g], Hproj[g], cols[0][g], sos(SOS), *[c[g] for c in cols[1:9]], HID, S, EOS, *table, n=n,
                                            want_logp=True, w_inv=cols[9][g] if x3 else None)
            for x, y in zip(grouped, one):
                assert torch.equal(x[g], y), f"expert {g}"
            lacks = np.array([[w < 0 or max(words[w], default=0) >= C for w in row] for row in cand])
            assert np.array_equal(np.isneginf(one[2].cpu().numpy()), lacks), g
            from mrn_amd.modules import decoding
            ref = decoding.attn_candidates_host(sds[g], Hbs[g], SOS, EOS, tokens, lengths, cand, n, S - 1)
            live = ~lacks
            L1 = np.array([[len(words[w]) + 1 if w >= 0 else 1 for w in row] for row in cand])
            assert np.all(np.abs(one[2].cpu().numpy()[live] - ref[2][live]) <= L1[live] * TOKEN_BAND), g


def test_bad_tables_and_limits_are_refused_before_any_launch(ops, monkeypatch):
    """ValueErrors for the tables (no library call at all), error codes from the argument checks for the limits"""
    B, T, D, C, S, K, _, _ = CAND_CASES["k3"]
    sd, Hb, words, tokens, lengths, cand, ref = cand_case("k3")
    att = module(sd, D, C)
    handle = handle_of(ops, tokens, lengths, cand, S, 1)
    with torch.no_grad():
        Hproj = ops.linear(Hb.cuda(), att.attention_cell.i2h.weight)
        args = att.greedy_args()

        def run(S=S, eos=EOS, hidden=HID, n=1, tokens=handle.tokens_dev, lengths=handle.lengths_dev, cand=handle.cand_dev):
            return ops.attn_score_candidates(Hb.cuda(), Hproj, args[0], sos(SOS), *args[1:9], hidden, S, eos, tokens, lengths, cand, n=n,
                                             w_inv=args[9])

        assert len(run()) == 5
        for kw, msg in (({"S": 513, "lengths": handle.lengths_dev}, "S=513"), ({"hidden": 128}, "hidden=128"), ({"eos": C}, "eos=")):
            with pytest.raises(RuntimeError, match=r"failed \(code -1\).*" + msg):
                run(**kw)
        dev = handle.cand_dev
        bad = (({"cand": torch.full_like(dev, len(words))}, "candidate index"), ({"cand": torch.full_like(dev, -2)}, "candidate index"),
               ({"cand": dev[:, :0].contiguous()}, "K >= 1"), ({"cand": dev[:2].contiguous()}, "cand"),
               ({"lengths": torch.full_like(handle.lengths_dev, S)}, "word length"), ({"tokens": -handle.tokens_dev - 1}, "negative class"),
               ({"cand": dev.long()}, "int32"), ({"cand": dev.cpu()}, "device of the features"), ({"n": 17}, "n=17"), ({"n": 0}, "n=0"))
        for kw, msg in bad:
            _, names = recorded_calls(monkeypatch, lambda: pytest.raises(ValueError, run, **kw).match(msg))
            assert names == [], (kw, names)
        with pytest.raises(ValueError, match="candidate index"):
            handle.with_cand(np.full((B, K), len(words), dtype=np.int32), S)
    torch.cuda.synchronize()


def test_the_lds_rule_on_both_sides_of_its_boundary(ops, monkeypatch):
    """the widest context the scorer's tile takes at T = 17 runs fused and meets the float64 form; 32 columns more go stepwise without
    a scorer launch, and agree with the fused scores of the narrower context's band"""
    from mrn_amd.modules import decoding
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    x3 = ops.DECODER_X3
    B, T, C, S, K = 2, 17, 37, 4, 3
    edge = max(D for D in range(32, 4096, 32) if ops.attn_score_whole_context(D, T, x3))
    lds = 4 * (2 * 16 * 260 + 16 * (edge + 4) + 16 * T + 256) + (1024 if x3 else 0) + 2368
    assert lds <= 160 * 1024 < lds + 4 * 16 * 32 and not ops.attn_score_whole_context(edge + 32, T, x3)
    words = [(5, 6), (7,), (), (8, 9, 10)]
    tokens, lengths = as_arrays(words)
    cand = np.int32([[0, 1, 2], [3, -1, 1]])
    for D, fused in ((edge, True), (edge + 32, False)):
        sd, Hb = beam_fixture(B, T, D, C, 300, 50.0)
        att = module(sd, D, C)
        assert att.score_fused(D, T, S, EOS, 1) == fused
        got, names = recorded_calls(monkeypatch, lambda: to_np(att.score_candidates(Hb.cuda(), SOS, EOS, handle_of(ops, tokens, lengths, cand, S, 1),
                                                                                    S - 1, want_logp=True)))
        assert bool([m for m in names if m.startswith("mrn_attn_score")]) == fused
        ref = decoding.attn_candidates_host(sd, Hb, SOS, EOS, tokens, lengths, cand, 1, S - 1, want_logp=True)
        check_against_host(f"D={D}", got, ref, words, cand, S, 1)


# ---- the evaluation forwards and validation() --------------------------------------------------------------------------------------
def word_lists(labels):
    """every label's list: the label, two neighbours of it, two words shared by all, one the converter cannot spell"""
    return {gt: [gt + "s", gt, gt[:-1] + "9" if gt else "q", "lds", "wave", "Ä" + gt] for gt in labels}


def test_mrnnet_returns_the_routed_experts_pair(ops, monkeypatch):
    """MRNNet's evaluation forward with attn_candidates: all experts in ONE grouped launch, and for every sample the pair and the word of
    the expert the routing picks -- on decisive samples the float64 form's on that expert's features"""
    from mrn_amd.modules import decoding
    from mrn_amd.tools.utils import AttnLabelConverter
    from tests.test_decode_attn_beam_gpu import CHARACTERS, LABELS, trba_nets
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    net, plain, image = trba_nets()
    conv = AttnLabelConverter(CHARACTERS)
    B, L = len(LABELS), 25
    lists = [word_lists(LABELS)[gt] for gt in LABELS]
    table = decoding.CandidateTable(conv, lists, True, L)
    cand = table.rows(lists)
    handle = ops.upload_words(table.tokens, table.lengths, "cuda", 2).with_cand(cand, L + 1)
    sos_t = torch.full((B,), 2, dtype=torch.long).cuda()
    with torch.no_grad():
        out, names = recorded_calls(monkeypatch, lambda: net(image.cuda(), True, sos_t, False, attn_candidates=handle))
        assert sum(m.startswith("mrn_attn_score_candidates") for m in names) == 1 and not [m for m in names if "beam" in m or "lexicon" in m]
        plain_out = net(image.cuda(), True, sos_t, False)
        assert torch.equal(out["logits"], plain_out["logits"]) and torch.equal(out["index"], plain_out["index"])
        with pytest.raises(ValueError, match="attn_beam"):
            net(image.cuda(), True, sos_t, False, attn_beam=4, attn_candidates=handle)
        feats = [e(image.cuda(), sos_t, False)["feature"].cpu() for e in net.model]
        newest = net(image.cuda(), False, sos_t, False, attn_candidates=handle)
        single = plain(image.cuda(), sos_t, False, attn_candidates=handle)
    index = out["index"].view(-1).cpu().numpy()
    path, prob, word = out["beam_path"].cpu().numpy(), out["beam_prob"].cpu().numpy(), out["beam_word"].cpu().numpy()
    assert path.shape == (B, L + 1) and prob.shape == (B, L + 1) and word.shape == (B,)
    assert newest["beam_path"].shape == (B, L + 1) and single["beam_word"].shape == (B,) and "beam_path" not in plain_out
    refs = [decoding.attn_candidates_host(e.Prediction.state_dict(), f, 2, 3, table.tokens, table.lengths, cand, 2, L) for e, f in zip(net.model, feats)]
    spelled = [[table.words[w] if w >= 0 else "" for w in row] for row in cand]
    checked = 0
    for b in range(B):
        ref = refs[int(index[b])]
        if not decisive_samples([tuple(w) for w in table.words], cand[b:b + 1], ref[2][b:b + 1])[0]:
            continue
        checked += 1
        assert word[b] == ref[0][b, 0] and np.array_equal(path[b], ref[3][b]), b
        assert np.all(np.abs(prob[b] - ref[4][b]) <= ref[4][b] * (np.exp(TOKEN_BAND) - 1) + 1e-37), b
    # the first expert has 30 classes: the words it cannot spell are dead for it alone
    C0 = net.model[0].Prediction.num_class
    lacks = np.array([[w < 0 or (table.tokens[w, :table.lengths[w]] >= C0).any() for w in row] for row in cand])
    assert lacks.any() and np.array_equal(np.isneginf(refs[0][2]), lacks) and not np.isneginf(refs[1][2][cand >= 0]).any()
    print(f"{checked} decisive samples of {B}; routing {index.tolist()}; words {[spelled[b][list(cand[b]).index(word[b])] if word[b] >= 0 else None for b in range(B)]}")
    assert checked >= 1


@pytest.mark.parametrize("kind", ["mrn", "model"])
def test_validation_on_a_trba(ops, monkeypatch, kind):
    """opt.candidates on the attention head: every prediction is the word of its own list the float64 form ranks first (decisive
    samples), with that word's confidence; the loss is the default run's; device and host scoring agree; dict and callable agree;
    without the key, or with None, all values are today's, bit for bit.  infer_time, a wall-clock time, is the one value left out"""
    from mrn_amd.modules import decoding
    from mrn_amd.test import validation
    from mrn_amd.tools.utils import AttnLabelConverter
    from tests.test_decode_attn_beam_gpu import CHARACTERS, LABELS, trba_nets, trba_opt
    for key in ("MRN_ATTN_BEAM", "MRN_GREEDY_DECODE", "MRN_VALIDATION_SCORING"):
        monkeypatch.delenv(key, raising=False)
    net, plain, image = trba_nets()
    model, choose = (net, "TF") if kind == "mrn" else (plain, "val")
    conv = AttnLabelConverter(CHARACTERS)
    B, L = len(LABELS), 25
    batches = [(image[:5], list(LABELS[:5])), (image[5:], list(LABELS[5:]))]
    table_of = word_lists(LABELS)

    def run(**kw):
        def go():
            with torch.no_grad():
                return validation(model, None, batches, conv, trba_opt(NED=True, **kw), val_choose=choose)
        res, names = recorded_calls(monkeypatch, go)
        return res[:6] + res[7:], names

    absent, names0 = run()
    none, _ = run(candidates=None)
    assert absent == none and not [m for m in names0 if "score_candidates" in m]
    got, names = run(candidates=table_of, lexicon_top_n=2)
    assert sum(m.startswith("mrn_attn_score_candidates") for m in names) == len(batches) and not [m for m in names if "attn_beam" in m or "lexicon" in m]
    assert got[0] == absent[0]                                                 # valid_loss: the greedy decoder's logits
    assert run(candidates=lambda labels: [table_of[gt] for gt in labels], lexicon_top_n=2)[0] == got
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "host")
    assert run(candidates=table_of, lexicon_top_n=2)[0] == got
    monkeypatch.delenv("MRN_VALIDATION_SCORING")
    with pytest.raises(ValueError, match="candidates and attn_decode='beam'"):
        run(candidates=table_of, attn_decode="beam")
    # the float64 form on the features of the expert the routing picks, last batch (the returned strings are the last batch's)
    img, labels = batches[-1]
    lists = [table_of[gt] for gt in labels]
    table = decoding.CandidateTable(conv, [table_of[gt] for gt in LABELS], True, L)
    assert all(not w.startswith("Ä") for w in table.words)
    cand = table.rows(lists)
    sos_t = torch.full((len(labels),), 2, dtype=torch.long).cuda()
    with torch.no_grad():
        if kind == "mrn":
            index = model(img.cuda(), True, sos_t, False)["index"].view(-1).cpu().numpy()
            experts = list(model.model)
            feats = [e(img.cuda(), sos_t, False)["feature"].cpu() for e in experts]
        else:
            index, experts = np.zeros(len(labels), dtype=np.int64), [model]
            feats = [model(img.cuda(), sos_t, False)["feature"].cpu()]
    refs = [decoding.attn_candidates_host(e.Prediction.state_dict(), f, 2, 3, table.tokens, table.lengths, cand, 2, L, want_logp=True)
            for e, f in zip(experts, feats)]
    checked = 0
    for b in range(len(labels)):
        ref = refs[int(index[b])]
        if not decisive_samples([tuple(w) for w in table.words], cand[b:b + 1], ref[2][b:b + 1])[0]:
            continue
        checked += 1
        best = table.words[ref[0][b, 0]] if ref[0][b, 0] >= 0 else ""
        assert best in lists[b] or ref[0][b, 0] < 0
        assert got[3][b].startswith(best + "[EOS]") and got[3][b].replace("[EOS]", "") == best, (b, got[3][b], best)
        want = float(np.prod(ref[4][b][:len(best)])) if best else 0.0
        assert abs(got[4][b] - want) <= want * (np.exp(max(len(best), 1) * TOKEN_BAND) - 1) + 1e-12, b
    print(f"{checked} decisive samples of {len(labels)} in the last batch")
    assert checked >= 1


def test_validation_on_a_crnn(monkeypatch):
    """opt.candidates on a CTC head: one ops.ctc_lexicon_decode(cand=) call per batch; predictions, accuracy and NED are those of the
    float64 host form's best words through the host string loop, the confidences exp(score) within the CTC lexicon decoder's band
    (tests/test_lexicon_gpu.py); device and host scoring agree; None is the call without the option"""
    import math
    from mrn_amd.modules import decoding
    from mrn_amd.test import _host_scores
    from tests import lexicon_cases as LC
    from tests.test_ctc_beam_gpu import run_validation, validation_case
    from tests.test_scoring_gpu import recorded_calls as recorded
    _, conv, _, opt, batches, logits = validation_case()
    chars = conv.character[4:]
    labels_all = [gt for _, labels in batches for gt in labels]
    lists = {gt: list(dict.fromkeys([gt[:-1] + chars[(chars.index(gt[-1]) + 3) % len(chars)], gt, gt[:-1], chars[5] * 3, "not in the character set"]))
             for gt in labels_all}
    table = decoding.CandidateTable(conv, [lists[gt] for gt in labels_all], False, opt.batch_max_length)
    assert "not in the character set" not in table.words
    T = logits[0].shape[1]
    n_correct, norm_ed, strings, scores = 0, 0.0, None, []
    for (_, labels), lg in zip(batches, logits):
        cand = table.rows([lists[gt] for gt in labels])
        index, score, score_all, path, prob = decoding.ctc_lexicon_host(lg, table.tokens, table.lengths, 2, cand)
        band = LC.ATOL + LC.RTOL * np.abs(score[:, 0])
        assert ((score[:, 0] - score[:, 1]) > 2 * band).all()           # the inputs' own property: float32 cannot swap the top two
        strings = conv.decode(path, [T] * len(path))
        assert strings == [table.words[i] for i in index[:, 0]] and all(w in lists[gt] for w, gt in zip(strings, labels))
        scores = score[:, 0].tolist()
        for term, correct, _ in _host_scores(labels, strings, prob, False, True):
            norm_ed += term if term is not None else 0
            n_correct += bool(correct)
    with recorded() as log:
        got = run_validation(monkeypatch, candidates=lists, lexicon_top_n=2)
    assert log.count("mrn_ctc_lexicon_decode_f32") == len(batches) and log.count("mrn_argmax_prob_f32") == 0
    assert list(got[3]) == strings and got[1] == n_correct / 16 * 100 and got[2] == norm_ed / 16 * 100 and got[7] == 16
    for conf, sc in zip(got[4], scores):
        assert abs(conf - math.exp(sc)) <= math.exp(sc) * math.expm1(2 * (LC.ATOL + LC.RTOL * abs(sc))) + 2e-45
    fn = run_validation(monkeypatch, candidates=lambda labels: [lists[gt] for gt in labels], lexicon_top_n=2)
    host_scored = run_validation(monkeypatch, scoring="host", candidates=lists, lexicon_top_n=2)
    default = run_validation(monkeypatch)
    none = run_validation(monkeypatch, candidates=None)
    for i in (0, 1, 2, 3, 4, 5, 7):                       # all but infer_time, which is a clock reading
        assert got[i] == fn[i] == host_scored[i], i
        assert default[i] == none[i], i
    assert got[0] == default[0]
    with pytest.raises(ValueError, match="candidates and ctc_decode='beam'"):
        run_validation(monkeypatch, candidates=lists, ctc_decode="beam")
    with pytest.raises(ValueError, match="no word list for the label"):
        run_validation(monkeypatch, candidates={labels_all[0]: [labels_all[0]]})
