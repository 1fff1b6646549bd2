"""Beam-search decoding on the attention head in one launch (mrn_attn_beam_decode_*, csrc/attn_decode.hip attn_beam_kernel) against the float64
reference mrn_amd/modules/decoding.py::attn_beam_host.

Bands: logits are held to 1e-4 of the oracle, a chosen token's log-probability (logit - lse) therefore to 2e-4 and a score of n tokens
to n * 2e-4.  A sample is decisive when every gap of the REFERENCE (neighbouring kept candidates, last kept against best dropped, every
step) is at least three times the step's band; decisive samples must match the reference exactly in tokens, lengths and order.  Every
sample, decisive or not, must be self-consistent: its tokens, fed through the teacher-forced decoder, give its log-probabilities and
score back.  tests/test_attn_beam_cpu.py holds the cases and checks on the CPU that at most B // 4 samples of a case are not decisive.

The file's name puts it behind tests/test_bench_gpu.py in the suite: that file starts bench.py as a child process and skips once the
pytest process has initialised the GPU, which every test here does."""
import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import BEAM_CASES, EOS, SOS, TOKEN_BAND, beam_case, beam_fixture, decisive
from tests.test_greedy_decode_gpu import CASES, HID, case, decode, fixture, grouped_fixture, module, sos

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def to_np(res):
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy() for r in res)


def search(att, Hb, W, S, eos=EOS):
    return to_np(att.beam_search(Hb.cuda(), SOS, eos, W, S - 1))


def check_layout(got, B, W, S, eos=EOS):
    """shapes, fills and dead slots as specified; path / prob are entry 0's"""
    tokens, length, score, logp, path, prob = got
    assert tokens.shape == (B, W, S) and tokens.dtype == np.int32 and length.shape == (B, W) and length.dtype == np.int32
    assert score.shape == (B, W) and score.dtype == np.float32 and logp.shape == (B, W, S) and logp.dtype == np.float32
    assert path.shape == (B, S) and path.dtype == np.int64 and prob.shape == (B, S) and prob.dtype == np.float32
    assert np.all(length[:, 0] >= 1)
    for b in range(B):
        for w in range(W):
            n = int(length[b, w])
            if n < 0:
                assert n == -1 and np.isneginf(score[b, w]) and np.all(tokens[b, w] == eos) and np.all(logp[b, w] == 0)
                assert np.all(length[b, w:] == -1)                          # dead slots come last
                continue
            assert 1 <= n <= S and np.isfinite(score[b, w])
            where = np.flatnonzero(tokens[b, w] == eos)
            assert n == (where[0] + 1 if where.size else S)
            assert np.all(tokens[b, w, n:] == eos) and np.all(logp[b, w, n:] == 0)
            assert np.all(tokens[b, w, :n] >= 0)
        live = score[b][length[b] >= 0]
        assert np.all(live[:-1] >= live[1:])                                # descending score
    assert np.array_equal(path, tokens[:, 0].astype(np.int64))
    np.testing.assert_allclose(prob, np.exp(logp[:, 0].astype(np.float64)), rtol=2e-6, atol=0)
    assert np.all(prob[logp[:, 0] == 0] == 1.0)


def check_self_consistent(att, Hb, got, eos=EOS):
    """(2) every live entry of every sample: the teacher-forced decoder on its tokens gives logp and score back"""
    tokens, length, score, logp, _, _ = got
    B, W, S = tokens.shape
    C = att.num_class
    text = np.concatenate([np.full((B, W, 1), SOS, dtype=np.int64), tokens[:, :, :-1].astype(np.int64)], axis=2).reshape(B * W, S)
    with torch.no_grad():
        rows = Hb.cuda().repeat_interleave(W, dim=0)
        logits = att(rows, torch.from_numpy(text).cuda(), True, S - 1)
    lsm = torch.log_softmax(logits.double(), dim=2).cpu().numpy().reshape(B, W, S, C)
    worst_lp = worst_sc = 0.0
    for b in range(B):
        for w in range(W):
            n = int(length[b, w])
            if n < 0:
                continue
            chosen = lsm[b, w, np.arange(n), tokens[b, w, :n]]
            worst_lp = max(worst_lp, np.abs(logp[b, w, :n] - chosen).max())
            worst_sc = max(worst_sc, abs(score[b, w] - chosen.sum()) / n)
    print(f"self-consistency: max |logp - teacher forced| {worst_lp:.3e}, max |score - sum| / tokens {worst_sc:.3e} (band {TOKEN_BAND})")
    for b in range(B):
        for w in range(W):
            n = int(length[b, w])
            if n < 0:
                continue
            chosen = lsm[b, w, np.arange(n), tokens[b, w, :n]]
            assert np.abs(logp[b, w, :n] - chosen).max() <= TOKEN_BAND, (b, w)
            assert abs(score[b, w] - chosen.sum()) <= n * TOKEN_BAND, (b, w)


def check_against_reference(name, got, ref):
    """(1) decisive samples equal the reference in tokens, lengths and order, scores and logp inside the band"""
    tokens, length, score, logp, path, prob = got
    rt, rl, rs, rlp, rpath, rprob, margin = ref
    keep = decisive(margin)
    d_lp = d_sc = 0.0
    for b in np.flatnonzero(keep):
        if np.array_equal(tokens[b], rt[b]) and np.array_equal(length[b], rl[b]):
            live = rl[b] >= 0
            d_lp = max(d_lp, np.abs(logp[b] - rlp[b]).max())
            d_sc = max(d_sc, (np.abs(score[b][live] - rs[b][live]) / rl[b][live]).max())
    print(f"{name}: {int(keep.sum())} decisive samples of {len(keep)}; max |logp - reference| {d_lp:.3e}, max |score - reference| / tokens "
          f"{d_sc:.3e} (band {TOKEN_BAND})")
    for b in np.flatnonzero(keep):
        assert np.array_equal(tokens[b], rt[b]), (name, b)
        assert np.array_equal(length[b], rl[b]), (name, b)
        live = rl[b] >= 0
        assert np.all(np.abs(logp[b] - rlp[b]) <= TOKEN_BAND), (name, b)
        assert np.all(np.abs(score[b][live] - rs[b][live]) <= rl[b][live] * TOKEN_BAND), (name, b)
        assert np.all(np.isneginf(score[b][~live]))
        assert np.array_equal(path[b], rpath[b])
        np.testing.assert_allclose(prob[b], rprob[b], atol=TOKEN_BAND)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("name", list(BEAM_CASES))
def test_kernel_matches_the_reference_and_itself(ops, monkeypatch, name, x3):
    """(1) + (2): the fused launch, both forms"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, W, _, _ = BEAM_CASES[name]
    sd, Hb, ref = beam_case(name)
    att = module(sd, D, C)
    assert att.beam_fused(D, T, S, EOS, W)
    got = search(att, Hb, W, S)
    check_layout(got, B, W, S)
    check_self_consistent(att, Hb, got)
    check_against_reference(name, got, ref)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("name", ["c331", "t65", "d512"])
def test_width_one_is_greedy(ops, monkeypatch, name, x3):
    """(3) the tokens of attn_greedy_decode up to the first eos, exactly: a row's logits are the greedy kernel's"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, _ = CASES[name]
    sd, Hb, _ = case(name)
    att = module(sd, D, C)
    _, tok = decode(ops, att, Hb.cuda(), sos(SOS), S, want_tokens=True)
    tok = tok.cpu().numpy()
    got = search(att, Hb, 1, S)
    check_layout(got, B, 1, S)
    for b in range(B):
        n = int(got[1][b, 0])
        where = np.flatnonzero(tok[b] == EOS)
        assert n == (where[0] + 1 if where.size else S)
        assert np.array_equal(got[0][b, 0, :n], tok[b, :n]), b


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("G", [3, 9])
def test_grouped_equals_single_launches(ops, monkeypatch, G, x3):
    """(4) ragged class counts (97, 331, 203) in one launch, nine experts in two: bit-identical to one launch per expert"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, S, W = 19, 31, 12, 4
    classes, atts, Hb = grouped_fixture(G, B, T, S)
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
        grouped = ops.attn_beam_decode_grouped(Hb, Hproj, cols[0], sos(SOS), *cols[1:9], HID, S, EOS, W, w_inv=cols[9] if x3 else None)
        assert (cols[9][0] is not None) == x3
        for g, a in enumerate(atts):
            one = ops.attn_beam_decode(Hb[g], Hproj[g], cols[0][g], sos(SOS), *[c[g] for c in cols[1:9]], HID, S, EOS, W,
                                       w_inv=cols[9][g] if x3 else None)
            for x, y in zip(grouped, one):
                assert torch.equal(x[g], y), f"expert {g}"
            check_layout(to_np(one), B, W, S)


def test_fused_and_stepwise_agree(ops, monkeypatch):
    """(4) the step loop on the B * W-row batch against the fused launch, on decisive samples; every sample of it self-consistent"""
    name = "c97_w4"
    B, T, D, C, S, W, _, _ = BEAM_CASES[name]
    sd, Hb, ref = beam_case(name)
    att = module(sd, D, C)
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    fused = search(att, Hb, W, S)
    monkeypatch.setenv("MRN_ATTN_BEAM", "stepwise")
    assert not att.beam_fused(D, T, S, EOS, W)
    step = search(att, Hb, W, S)
    check_layout(step, B, W, S)
    check_self_consistent(att, Hb, step)
    check_against_reference(name + " stepwise", step, ref)
    for b in np.flatnonzero(decisive(ref[6])):
        assert np.array_equal(fused[0][b], step[0][b]) and np.array_equal(fused[1][b], step[1][b])
        assert np.all(np.abs(fused[2][b] - step[2][b]) <= 2 * fused[1][b] * TOKEN_BAND)


def test_context_over_the_budget_goes_stepwise(ops, monkeypatch):
    """(4) D = 2304 does not fit the whole-context tile: no beam launch, the step loop, still self-consistent"""
    from mrn_amd._lib import LIB
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    B, T, D, C, S, W = 5, 65, 2304, 203, 6, 4
    sd, Hb = beam_fixture(B, T, D, C, 500, 50.0)
    att = module(sd, D, C)
    assert not ops.attn_beam_whole_context(D, T, W) and not att.beam_fused(D, T, S, EOS, W)
    names, real = [], LIB.call
    monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = search(att, Hb, W, S)
    monkeypatch.setattr(LIB, "call", real)
    assert not [n for n in names if n.startswith("mrn_attn_beam")] and names.count("mrn_embed_gather_f32") == S
    check_layout(got, B, W, S)
    check_self_consistent(att, Hb, got)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("other", [7, 300])
def test_ties_go_to_the_lower_entry_then_the_lower_class(ops, monkeypatch, x3, other):
    """(5) class 5's generator row, bias and embedding copied to a second class (in the same class tile, then in another wave's) and both
    lifted above every other class: all candidates of a step tie, so the survivors are (entry 0, 5), (entry 0, other), (entry 1, 5),
    (entry 1, other) -- entry k of W = 4 ends as 5 ... 5 followed by k's two bits, 0 = class 5, 1 = the other"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, _ = CASES["c331"]
    sd, Hb, _ = case("c331")
    sd = {k: v.clone() for k, v in sd.items()}
    sd["generator.weight"][other] = sd["generator.weight"][5]
    sd["generator.bias"][5] += 30.0
    sd["generator.bias"][other] = sd["generator.bias"][5]
    sd["char_embeddings.weight"][other] = sd["char_embeddings.weight"][5]
    att = module(sd, D, C)
    for W in (1, 2, 4):
        tokens, length, score, logp, path, prob = search(att, Hb, W, S)
        for k in range(W):
            want = [5] * (S - 2) + [other if k & 2 else 5, other if k & 1 else 5]
            assert np.array_equal(tokens[:, k], np.tile(np.int32(want), (B, 1))), (W, k)
        assert np.all(score == score[:, :1]) and np.all(length == S)


@pytest.mark.parametrize("x3", [True, False])
def test_planted_early_eos(ops, monkeypatch, x3):
    """(6) eos lifted above every class: entry 0 is [eos] after the first step and keeps its score and tokens, every other entry ends on
    its second token and the workgroups stop early; the step loop, which runs all S steps, returns the same"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    name = "c97_w4"
    B, T, D, C, S, W, seed0, scale = BEAM_CASES[name]
    sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
    sd["generator.bias"][EOS] += 60.0
    att = module(sd, D, C)
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    fused = search(att, Hb, W, S)
    check_layout(fused, B, W, S)
    tokens, length, score, logp, path, prob = fused
    assert np.all(length[:, 0] == 1) and np.all(length[:, 1:] == 2) and np.all(tokens[:, 1:, 1] == EOS)
    assert np.array_equal(score[:, 0], logp[:, 0, 0])                      # 0 + lp, untouched by the later steps
    assert np.array_equal(score[:, 1:], logp[:, 1:, 0] + logp[:, 1:, 1])
    check_self_consistent(att, Hb, fused)
    monkeypatch.setenv("MRN_ATTN_BEAM", "stepwise")
    step = search(att, Hb, W, S)
    assert np.array_equal(step[1], length)
    from mrn_amd.modules import decoding
    ref = decoding.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1, want_margin=True)
    check_against_reference(name + " eos", fused, ref)
    check_against_reference(name + " eos stepwise", step, ref)


def test_calls_outside_the_limits_are_errors(ops):
    """(7) W = 17, S = 513, hidden != 256 (and an eos that is no class): an error code from the argument checks, which stand before the
    first launch (tests/test_attn_beam_cpu.py::test_rule_matches_the_launch_helper)"""
    B, T, D, C, S, _ = CASES["c97"]
    sd, Hb, _ = case("c97")
    att = module(sd, D, C)
    with torch.no_grad():
        Hproj = ops.linear(Hb.cuda(), att.attention_cell.i2h.weight)
        args = att.greedy_args()

        def run(S=S, eos=EOS, W=4, hidden=HID):
            return ops.attn_beam_decode(Hb.cuda(), Hproj, args[0], sos(SOS), *args[1:9], hidden, S, eos, W, w_inv=args[9])

        run()
        for kw, msg in (({"W": 17}, "beam width W=17"), ({"W": 0}, "beam width W=0"), ({"S": 513}, "S=513"), ({"hidden": 128}, "hidden=128"),
                        ({"eos": C}, "eos=")):
            with pytest.raises(RuntimeError, match=r"failed \(code -1\).*" + msg):
                run(**kw)
    torch.cuda.synchronize()


# ---- the evaluation forwards and validation() --------------------------------------------------------------------------------------
CHARACTERS = "abcdefghijklmnopqrstuvwxyz0123456789"
LABELS = ["beam", "search", "a1", "", "mi355x", "lds", "wave64", "x"]


def trba_opt(**kw):
    import types
    return types.SimpleNamespace(Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM", Prediction="Attn",
                                 num_fiducial=20, imgH=32, imgW=128, input_channel=4, output_channel=512, hidden_size=256,
                                 batch_max_length=25, beam_width=4, **kw)


def trba_nets():
    """(two-expert MRNNet, plain Model) with peaked generators, and the batch"""
    import contextlib
    import io
    from mrn_amd.modules.model import Model, MRNNet
    from mrn_amd.tools import weights as Wt
    opt = trba_opt()
    classes = (30, 5 + len(CHARACTERS))
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(256, c)
            net.build_prediction(opt, c)
        plain = Model(trba_opt(num_class=classes[1]))
        plain.reset_class(plain.opt, "cpu")
    Wt.fill_state_dict(net.state_dict(), seed=11)
    Wt.fill_state_dict(plain.state_dict(), seed=12)
    with torch.no_grad():
        for head in [e.Prediction for e in net.model] + [plain.Prediction]:
            head.generator.weight.mul_(40.0)
    image = torch.from_numpy(Wt.smooth_image("attn_beam", (len(LABELS), 4, 32, 128), 11))
    return net.cuda().eval(), plain.cuda().eval(), image


def kept_confidence(conv, ref, b):
    """what validation()'s unchanged scorer makes of the reference's best entry (test.py:222-226, 262-265): the row is decoded to a
    string, cut at the CHARACTER position of the first "[EOS]" (without one find() gives -1 and the last element goes), and the
    probabilities are cut at that same number -- for a row of ordinary characters the product of the probabilities in front of [EOS],
    exp(score - logp of [EOS]); a predicted [UNK] / [PAD] / [SOS] is several characters long and lets later factors in.  Nothing kept: 0
    -> (confidence, factors)"""
    S = ref[4].shape[1]
    cut = conv.decode(ref[4][b:b + 1], [S])[0].find("[EOS]")
    probs = np.exp(ref[3][b, 0])[:cut]
    return (float(np.prod(probs)) if len(probs) else 0.0), len(probs)


@pytest.mark.parametrize("kind", ["mrn", "model"])
def test_validation_decodes_by_beam_search(ops, monkeypatch, kind):
    """(8) attn_decode="beam": the loss is the greedy run's bit for bit, the confidences are those of the (routed expert's) reference
    best entry for decisive samples, device and host scoring agree, one beam launch per heads group; without the option (or with
    "greedy") every value is the greedy run's.  infer_time, a wall-clock time, is the one value of the eight left out"""
    from mrn_amd._lib import LIB
    from mrn_amd.modules import decoding
    from mrn_amd.test import validation
    from mrn_amd.tools.utils import AttnLabelConverter
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    monkeypatch.delenv("MRN_VALIDATION_SCORING", raising=False)
    net, plain, image = trba_nets()
    model, choose = (net, "TF") if kind == "mrn" else (plain, "val")
    conv = AttnLabelConverter(CHARACTERS)
    assert conv.dict["[EOS]"] == decoding.ATTN_EOS == 3 and conv.dict["[SOS]"] == 2
    B, W, L = len(LABELS), 4, 25
    names, real = [], LIB.call

    def run(**kw):
        names.clear()
        monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        with torch.no_grad():
            res = validation(model, None, [(image, list(LABELS))], conv, trba_opt(**kw), val_choose=choose)
        monkeypatch.setattr(LIB, "call", real)
        return res[:6] + res[7:], sum(n.startswith("mrn_attn_beam_decode") for n in names)

    absent, n0 = run()
    greedy, n1 = run(attn_decode="greedy")
    assert absent == greedy and n0 == n1 == 0
    beam, launches = run(attn_decode="beam")
    assert launches == 1
    assert beam[0] == greedy[0]                                            # valid_loss: the greedy decoder's logits
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "host")
    host, _ = run(attn_decode="beam")
    monkeypatch.delenv("MRN_VALIDATION_SCORING")
    assert host == beam
    # the reference: attn_beam_host on the features of the expert the routing picks
    sos_t = torch.full((B,), 2, dtype=torch.long).cuda()
    with torch.no_grad():
        if kind == "mrn":
            out = model(image.cuda(), True, sos_t, False, attn_beam=W)
            index = out["index"].view(-1).cpu().numpy()
            experts = list(model.model)
            feats = [e(image.cuda(), sos_t, False)["feature"].cpu() for e in experts]
            again = model(image.cuda(), True, sos_t, False)
            assert torch.equal(out["logits"], again["logits"]) and "beam_path" not in again      # one more launch, not a replacement
        else:
            out = model(image.cuda(), sos_t, False, attn_beam=W)
            index, experts = np.zeros(B, dtype=np.int64), [model]
            feats = [out["feature"].cpu()]
    refs = [decoding.attn_beam_host(e.Prediction.state_dict(), f, 2, 3, W, L, want_margin=True) for e, f in zip(experts, feats)]
    path, prob = out["beam_path"].cpu().numpy(), out["beam_prob"].cpu().numpy()
    assert path.shape == (B, L + 1) and prob.shape == (B, L + 1)
    checked = 0
    for b in range(B):
        ref = refs[int(index[b])]
        if not decisive(ref[6])[b]:
            continue
        checked += 1
        assert np.array_equal(path[b], ref[4][b]), b
        want, kept = kept_confidence(conv, ref, b)
        print(f"sample {b}: expert {int(index[b])}, {kept} kept probabilities, confidence {beam[4][b]:.6e}, reference {want:.6e}")
        assert abs(beam[4][b] - want) <= want * (np.exp(max(kept, 1) * TOKEN_BAND) - 1) + 1e-12, b
    print(f"{checked} decisive samples of {B}")
    assert checked >= 1
