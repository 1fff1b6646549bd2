"""Beam search on the attention head fused with a character n-gram model in one launch (mrn_attn_beam_lm_decode_*, csrc/attn_decode.hip
attn_beam_lm_kernel) against the float64 reference mrn_amd/modules/decoding.py::attn_beam_host(lm=).

Bands: those of tests/test_decode_attn_beam_gpu.py for the acoustic outputs (a token's log-probability to TOKEN_BAND = 2e-4, a score of n
tokens to n * TOKEN_BAND).  The fused key of an entry of n tokens, acoustic + alpha * lm + beta * len, is held to
n * TOKEN_BAND * (1 + alpha) + alpha * n * 2^-23 * |lm_ref|: the acoustic band, and the float32 running sum of n model terms against the
reference's own sum.  A sample is decisive when every gap of the REFERENCE (neighbouring kept proposals and last kept against best
dropped by key, and every live unfinished entry's N-th against (N + 1)-th logit, the pruning boundary) is at least three times its
band; decisive samples must match the reference exactly in tokens, lengths and order.  Every sample must be self-consistent (the
teacher-forced decoder gives its log-probabilities and score back).  tests/test_attn_lm_cpu.py holds the cases and checks on the CPU
that at most B // 4 samples of a case are not decisive.

The file's name puts it behind tests/test_bench_gpu.py in the suite, as its siblings' do."""
import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import BEAM_CASES, EOS, SOS, TOKEN_BAND, beam_fixture, decisive
from tests.test_attn_lm_cpu import LM_BONUS, LM_CASES, PLANT, lm_case, planted_case, random_lm
from tests.test_decode_attn_beam_gpu import CHARACTERS, LABELS, check_self_consistent, kept_confidence, to_np, trba_nets, trba_opt
from tests.test_greedy_decode_gpu import CASES, HID, case, grouped_fixture, module, sos

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def search(att, Hb, W, S, handle, alpha, beta, top_n, eos=EOS):
    return to_np(att.beam_search(Hb.cuda(), SOS, eos, W, S - 1, lm=handle, lm_weight=alpha, lm_bonus=beta, top_n=top_n))


def check_layout(got, B, W, S, eos=EOS):
    """shapes, fills and dead slots as specified; entries in descending fused; path / prob are entry 0's"""
    tokens, length, score, logp, path, prob, fused = got
    assert tokens.shape == (B, W, S) and tokens.dtype == np.int32 and length.shape == (B, W) and length.dtype == np.int32
    assert score.shape == (B, W) and score.dtype == np.float32 and logp.shape == (B, W, S) and logp.dtype == np.float32
    assert path.shape == (B, S) and path.dtype == np.int64 and prob.shape == (B, S) and prob.dtype == np.float32
    assert fused.shape == (B, W) and fused.dtype == np.float32
    assert np.all(length[:, 0] >= 1)
    for b in range(B):
        for w in range(W):
            n = int(length[b, w])
            if n < 0:
                assert n == -1 and np.isneginf(score[b, w]) and np.isneginf(fused[b, w])
                assert np.all(tokens[b, w] == eos) and np.all(logp[b, w] == 0)
                assert np.all(length[b, w:] == -1)                          # dead slots come last
                continue
            assert 1 <= n <= S and np.isfinite(score[b, w]) and np.isfinite(fused[b, w])
            where = np.flatnonzero(tokens[b, w] == eos)
            assert n == (where[0] + 1 if where.size else S)
            assert np.all(tokens[b, w, n:] == eos) and np.all(logp[b, w, n:] == 0)
            assert np.all(tokens[b, w, :n] >= 0)
        live = fused[b][length[b] >= 0]
        assert np.all(live[:-1] >= live[1:])                                # descending fused key
    assert np.array_equal(path, tokens[:, 0].astype(np.int64))
    np.testing.assert_allclose(prob, np.exp(logp[:, 0].astype(np.float64)), rtol=2e-6, atol=0)
    assert np.all(prob[logp[:, 0] == 0] == 1.0)


def model_sum(lm, row, n, eos):
    """the reference's LM sum of an entry: its n tokens walked through the model, float64"""
    a = b = 0
    total = 0.0
    for k in map(int, row[:n]):
        total += lm.logp(a, b, 0) if k == eos else lm.unk_logp if k == 0 else lm.logp(a, b, k)
        a, b = b, (0 if k == eos else k)
    return total


def check_against_reference(name, got, ref, lm, alpha, eos=EOS):
    """decisive samples equal the reference in tokens, lengths and order; score and logp inside the acoustic bands, fused inside its own"""
    tokens, length, score, logp, path, prob, fused = got
    rt, rl, rs, rlp, rpath, rprob, rfused, margin = ref
    keep = decisive(margin)
    d_lp = d_sc = d_key = 0.0
    for b in np.flatnonzero(keep):
        if np.array_equal(tokens[b], rt[b]) and np.array_equal(length[b], rl[b]):
            live = rl[b] >= 0
            d_lp = max(d_lp, np.abs(logp[b] - rlp[b]).max())
            d_sc = max(d_sc, (np.abs(score[b][live] - rs[b][live]) / rl[b][live]).max())
            d_key = max(d_key, (np.abs(fused[b][live] - rfused[b][live]) / rl[b][live]).max())
    print(f"{name}: {int(keep.sum())} decisive samples of {len(keep)}; max |logp - reference| {d_lp:.3e}, max |score - reference| / tokens "
          f"{d_sc:.3e}, max |fused - reference| / tokens {d_key:.3e} (band {TOKEN_BAND} and {TOKEN_BAND * (1 + alpha):.1e} + the model's)")
    for b in np.flatnonzero(keep):
        assert np.array_equal(tokens[b], rt[b]), (name, b)
        assert np.array_equal(length[b], rl[b]), (name, b)
        live = rl[b] >= 0
        assert np.all(np.abs(logp[b] - rlp[b]) <= TOKEN_BAND), (name, b)
        assert np.all(np.abs(score[b][live] - rs[b][live]) <= rl[b][live] * TOKEN_BAND), (name, b)
        assert np.all(np.isneginf(score[b][~live])) and np.all(np.isneginf(fused[b][~live]))
        for w in np.flatnonzero(live):
            n = int(rl[b, w])
            band = n * TOKEN_BAND * (1 + alpha) + alpha * n * 2.0 ** -23 * abs(model_sum(lm, rt[b, w], n, eos))
            assert abs(fused[b, w] - rfused[b, w]) <= band, (name, b, w)
        assert np.array_equal(path[b], rpath[b])
        np.testing.assert_allclose(prob[b], rprob[b], atol=TOKEN_BAND)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("name", list(LM_CASES))
def test_kernel_matches_the_reference_and_itself(ops, monkeypatch, name, x3):
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, W, _, _ = BEAM_CASES[name]
    _, _, order, top_n, C_lm, _, alpha = LM_CASES[name]
    sd, Hb, lm, ref = lm_case(name)
    att = module(sd, D, C)
    handle = ops.upload_char_lm(lm, "cuda")
    assert att.beam_lm_fused(D, T, S, EOS, W, handle, top_n)
    got = search(att, Hb, W, S, handle, alpha, LM_BONUS, top_n)
    check_layout(got, B, W, S)
    check_self_consistent(att, Hb, got[:6])
    check_against_reference(name, got, ref, lm, alpha)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("name,top_n", [("c97_w4", 15), ("c37_w3", 3), ("d512_w16", 1)])
def test_zero_weights_are_the_plain_launch_bit_for_bit(ops, monkeypatch, name, top_n, x3):
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, W, _, _ = BEAM_CASES[name]
    sd, Hb, lm, _ = lm_case(name)
    att = module(sd, D, C)
    handle = ops.upload_char_lm(lm, "cuda")
    plain = att.beam_search(Hb.cuda(), SOS, EOS, W, S - 1)
    fused = att.beam_search(Hb.cuda(), SOS, EOS, W, S - 1, lm=handle, lm_weight=0.0, lm_bonus=0.0, top_n=top_n)
    assert len(plain) == 6 and len(fused) == 7
    for i, (x, y) in enumerate(zip(plain, fused)):
        assert x.dtype == y.dtype and torch.equal(x, y), i
    assert torch.equal(fused[6], plain[2])


def test_top_n_above_sixteen_is_the_launch_at_sixteen(ops, monkeypatch):
    """N = min(16, max(W, top_n)): beam_top_n = 40 is the same search as 16 and takes the launch, not the host form"""
    from mrn_amd._lib import LIB
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    name = "c37_w3"
    B, T, D, C, S, W, _, _ = BEAM_CASES[name]
    alpha = LM_CASES[name][6]
    sd, Hb, lm, _ = lm_case(name)
    att = module(sd, D, C)
    handle = ops.upload_char_lm(lm, "cuda")
    assert att.beam_lm_fused(D, T, S, EOS, W, handle, 40)
    names, real = [], LIB.call
    monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    wide = att.beam_search(Hb.cuda(), SOS, EOS, W, S - 1, lm=handle, lm_weight=alpha, lm_bonus=LM_BONUS, top_n=40)
    monkeypatch.setattr(LIB, "call", real)
    assert sum(n.startswith("mrn_attn_beam_lm_decode") for n in names) == 1
    at16 = att.beam_search(Hb.cuda(), SOS, EOS, W, S - 1, lm=handle, lm_weight=alpha, lm_bonus=LM_BONUS, top_n=16)
    for x, y in zip(wide, at16):
        assert torch.equal(x, y)


@pytest.mark.parametrize("x3", [True, False])
def test_planted_preference_flips_the_best_entry(ops, monkeypatch, x3):
    """the case of tests/test_attn_lm_cpu.py: two classes delta = 1e-3 apart, the bigram model prefers the second"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    p = PLANT
    sd, Hb, lm, lp_second = planted_case()
    att = module({k: v.float() for k, v in sd.items()}, p["D"], p["C"])
    handle = ops.upload_char_lm(lm, "cuda")
    plain = to_np(att.beam_search(Hb.cuda(), SOS, EOS, 1, 0))
    fused = search(att, Hb, 1, 1, handle, p["alpha"], p["beta"], 2)
    check_layout(fused, 1, 1, 1)
    assert plain[0][0, 0, 0] == p["first"] and fused[0][0, 0, 0] == p["second"]
    want = lp_second + p["alpha"] * lm.logp(0, 0, p["second"]) + p["beta"]
    print(f"fused {fused[6][0, 0]:.6f}, by hand {want:.6f}; score {fused[2][0, 0]:.6f}, reference {lp_second:.6f}")
    assert abs(fused[2][0, 0] - lp_second) <= TOKEN_BAND
    assert abs(fused[6][0, 0] - want) <= TOKEN_BAND * (1 + p["alpha"]) + p["alpha"] * 2.0 ** -23 * abs(lm.logp(0, 0, p["second"]))


@pytest.mark.parametrize("x3", [True, False])
def test_planted_early_eos(ops, monkeypatch, x3):
    """eos lifted above every class: entries finish on their first or second token, a finished entry keeps its key (which holds the
    end-of-text term) and the workgroups stop early"""
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    from mrn_amd.modules import decoding
    name = "c97_w4"
    B, T, D, C, S, W, _, _ = BEAM_CASES[name]
    seed0, scale, order, top_n, C_lm, _, alpha = LM_CASES[name]
    sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
    sd["generator.bias"][EOS] += 60.0
    lm = lm_case(name)[2]
    att = module(sd, D, C)
    got = search(att, Hb, W, S, ops.upload_char_lm(lm, "cuda"), alpha, LM_BONUS, top_n)
    check_layout(got, B, W, S)
    assert np.all(got[1] <= 2) and np.all(got[1][:, 0] == 1)
    check_self_consistent(att, Hb, got[:6])
    ref = decoding.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1, want_margin=True, lm=lm, lm_weight=alpha, lm_bonus=LM_BONUS, top_n=top_n)
    assert decisive(ref[7]).sum() >= 1
    check_against_reference(name + " eos", got, ref, lm, alpha)


@pytest.mark.parametrize("x3", [True, False])
def test_grouped_equals_single_launches(ops, monkeypatch, x3):
    """G = 3 with class counts 97, 331, 203 and one model over 97 classes: bit-identical to one launch per expert"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    G, B, T, S, W = 3, 19, 31, 12, 4
    classes, atts, Hb = grouped_fixture(G, B, T, S)
    assert len(set(classes)) == 3
    handle = ops.upload_char_lm(random_lm(97, 3, 5), "cuda")
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
        grouped = ops.attn_beam_lm_decode_grouped(Hb, Hproj, cols[0], sos(SOS), *cols[1:9], HID, S, EOS, W, handle, 0.3, LM_BONUS, 15,
                                                  w_inv=cols[9] if x3 else None)
        assert len(grouped) == 7 and (cols[9][0] is not None) == x3
        for g, a in enumerate(atts):
            one = ops.attn_beam_lm_decode(Hb[g], Hproj[g], cols[0][g], sos(SOS), *[c[g] for c in cols[1:9]], HID, S, EOS, W, handle, 0.3,
                                          LM_BONUS, 15, w_inv=cols[9][g] if x3 else None)
            for x, y in zip(grouped, one):
                assert torch.equal(x[g], y), f"expert {g}"
            check_layout(to_np(one), B, W, S)


def test_calls_outside_the_limits_are_errors(ops):
    """top_n = 0 or 17, alpha < 0, a NaN beta and a table whose size is no power of two: an error from the argument checks, which stand
    before the first launch (tests/test_attn_lm_cpu.py::test_rule_matches_the_launch_helper)"""
    import copy
    B, T, D, C, S, _ = CASES["c97"]
    sd, Hb, _ = case("c97")
    att = module(sd, D, C)
    handle = ops.upload_char_lm(random_lm(C, 3, 0), "cuda")
    with torch.no_grad():
        Hproj = ops.linear(Hb.cuda(), att.attention_cell.i2h.weight)
        args = att.greedy_args()

        def run(lm=handle, alpha=0.5, beta=0.0, top_n=15, raw=False):
            if raw:                     # past the Python check of the weights: the entry point's own
                return ops._attn_beam_grouped(Hb.cuda().unsqueeze(0), Hproj.unsqueeze(0), [args[0]], sos(SOS), *[[a] for a in args[1:9]], HID, S,
                                              EOS, 4, None if args[9] is None else [args[9]], None, fusion=(lm, alpha, beta, top_n))
            return ops.attn_beam_lm_decode(Hb.cuda(), Hproj, args[0], sos(SOS), *args[1:9], HID, S, EOS, 4, lm, alpha, beta, top_n, w_inv=args[9])

        assert len(run()) == 7 and len(run(raw=True)) == 7
        odd = copy.copy(handle)
        odd.size = handle.size - 2
        for kw, msg in (({"top_n": 0}, "top_n=0"), ({"top_n": 17}, "top_n=17"), ({"alpha": -0.5, "raw": True}, "alpha -0.5"),
                        ({"beta": float("nan"), "raw": True}, "beta nan"), ({"lm": odd}, "not a power of two")):
            with pytest.raises(RuntimeError, match=r"failed \(code -1\).*" + msg):
                run(**kw)
        for kw in ({"alpha": -0.5}, {"beta": float("nan")}, {"alpha": float("inf")}):
            with pytest.raises(ValueError, match="lm_weight|lm_bonus"):
                run(**kw)
        with pytest.raises(ValueError, match="upload_char_lm"):
            run(lm=None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("how", ["budget", "stepwise"])
def test_what_the_launch_does_not_take_goes_to_the_host_form(ops, monkeypatch, how):
    """a context beyond the LDS budget (D = 2304) and MRN_ATTN_BEAM=stepwise: no launch with a model, the float64 host form's outputs"""
    from mrn_amd._lib import LIB
    from mrn_amd.modules import decoding
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    if how == "budget":
        B, T, D, C, S, W, top_n, alpha = 5, 65, 2304, 203, 6, 4, 15, 0.2
        sd, Hb = beam_fixture(B, T, D, C, 500, 50.0)
        lm = random_lm(C, 3, 3)
        assert not ops.attn_beam_lm_whole_context(D, T, W)
    else:
        name = "c37_w3"
        B, T, D, C, S, W, _, _ = BEAM_CASES[name]
        _, _, _, top_n, _, _, alpha = LM_CASES[name]
        sd, Hb, lm, _ = lm_case(name)
        monkeypatch.setenv("MRN_ATTN_BEAM", "stepwise")
    att = module(sd, D, C)
    handle = ops.upload_char_lm(lm, "cuda")
    assert not att.beam_lm_fused(D, T, S, EOS, W, handle, top_n)
    names, real = [], LIB.call
    monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    res = att.beam_search(Hb.cuda(), SOS, EOS, W, S - 1, lm=handle, lm_weight=alpha, lm_bonus=LM_BONUS, top_n=top_n)
    monkeypatch.setattr(LIB, "call", real)
    assert not [n for n in names if n.startswith("mrn_attn_beam")] and all(r.is_cuda for r in res)
    got = to_np(res)
    check_layout(got, B, W, S)
    ref = decoding.attn_beam_host(att.state_dict(), Hb, SOS, EOS, W, S - 1, want_margin=True, lm=lm, lm_weight=alpha, lm_bonus=LM_BONUS,
                                  top_n=top_n)
    keep = decisive(ref[7])
    print(f"{how}: {int(keep.sum())} decisive samples of {B}")
    assert keep.sum() >= 1
    check_against_reference(how, got, ref, lm, alpha)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("other", [7, 300])
def test_ties_go_to_the_lower_entry_then_the_lower_class(ops, monkeypatch, x3, other):
    """the tie case of tests/test_decode_attn_beam_gpu.py (class 5 copied to a second class, both lifted above every other) with a bigram
    table of identical values: the keys of a step's proposals are equal too, so entry k of W = 4 ends as 5 ... 5 followed by k's two
    bits, 0 = class 5, 1 = the other"""
    from mrn_amd.modules.char_lm import CharLM
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
    pairs = {(a, b): (-1.0, 0.0) for a in (0, 5, other) for b in (5, other)}
    lm = CharLM(2, np.full(C, -3.0), np.zeros(C), -3.0, bigrams=pairs)
    handle = ops.upload_char_lm(lm, "cuda")
    for W in (1, 2, 4):
        tokens, length, score, logp, path, prob, fused = search(att, Hb, W, S, handle, 0.5, 0.25, 15)
        for k in range(W):
            want = [5] * (S - 2) + [other if k & 2 else 5, other if k & 1 else 5]
            assert np.array_equal(tokens[:, k], np.tile(np.int32(want), (B, 1))), (W, k)
        assert np.all(score == score[:, :1]) and np.all(fused == fused[:, :1]) and np.all(length == S)
        np.testing.assert_allclose(fused, score + 0.5 * (-1.0 * S) + 0.25 * S, rtol=0, atol=1e-4)


# ---- the evaluation forwards and validation() --------------------------------------------------------------------------------------
TEXTS = ["beam", "search", "a1", "mi355x", "lds", "wave64", "x", "seam", "beach", "wave", "lexicon", "a12", "x1", "mi300", "search1"]


@pytest.mark.parametrize("kind", ["mrn", "model"])
def test_validation_fuses_the_model(ops, monkeypatch, kind):
    """attn_decode="beam" with attn_lm on a batch every sample of which is decisive (width 2, lm_weight 0.3, lm_bonus 0.1: asserted):
    one launch with the model per heads group and none without; the loss is the greedy run's bit for bit; accuracy, normalised edit
    distance, strings, labels and the number of samples are those the unchanged scorer's host form makes of the (routed expert's)
    host-form best entries, the confidences within the band of their kept tokens; device and host scoring agree.  With the option absent
    or None every value is the plain beam run's, and without attn_decode="beam" the option is an error.  infer_time, a wall-clock
    time, is the one value of the eight left out"""
    from mrn_amd._lib import LIB
    from mrn_amd.modules import decoding
    from mrn_amd.modules.char_lm import build_char_lm
    from mrn_amd.test import _host_scores, validation
    from mrn_amd.tools.utils import AttnLabelConverter
    for key in ("MRN_ATTN_BEAM", "MRN_GREEDY_DECODE", "MRN_VALIDATION_SCORING"):
        monkeypatch.delenv(key, raising=False)
    net, plain, image = trba_nets()
    model, choose = (net, "TF") if kind == "mrn" else (plain, "val")
    conv = AttnLabelConverter(CHARACTERS)
    lm = build_char_lm(conv, TEXTS, order=3)
    assert lm.C_lm == len(conv.character) and lm.dropped == 0
    B, W, L, alpha, beta, top_n = len(LABELS), 2, 25, 0.3, 0.1, 15
    names, real = [], LIB.call

    def run(**kw):
        names.clear()
        opt = trba_opt(NED=True, **kw)
        opt.beam_width = W
        monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        try:
            with torch.no_grad():
                res = validation(model, None, [(image, list(LABELS))], conv, opt, val_choose=choose)
        finally:
            monkeypatch.setattr(LIB, "call", real)
        return res[:6] + res[7:], sum(n.startswith("mrn_attn_beam_lm_decode") for n in names), sum(n.startswith("mrn_attn_beam_decode") for n in names)

    greedy, n0, m0 = run()
    beam, n1, m1 = run(attn_decode="beam")
    off, n2, m2 = run(attn_decode="beam", attn_lm=None, lm_weight=alpha, lm_bonus=beta)
    assert off == beam and (n0, m0, n1, m1, n2, m2) == (0, 0, 0, 1, 0, 1)
    with pytest.raises(ValueError, match="attn_decode='beam'"):
        run(attn_lm=lm)
    fused, launches, plain_launches = run(attn_decode="beam", attn_lm=lm, lm_weight=alpha, lm_bonus=beta)
    assert launches == 1 and plain_launches == 0
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "host")
    host, _, _ = run(attn_decode="beam", attn_lm=lm, lm_weight=alpha, lm_bonus=beta)
    monkeypatch.delenv("MRN_VALIDATION_SCORING")
    assert host == fused
    # the reference: attn_beam_host(lm=) on the features of the expert the routing picks
    handle = ops.upload_char_lm(lm, "cuda")
    sos_t = torch.full((B,), 2, dtype=torch.long).cuda()
    with torch.no_grad():
        if kind == "mrn":
            out = model(image.cuda(), True, sos_t, False, attn_beam=W, attn_lm=(handle, alpha, beta, top_n))
            index = out["index"].view(-1).cpu().numpy()
            experts = list(model.model)
            feats = [e(image.cuda(), sos_t, False)["feature"].cpu() for e in experts]
        else:
            out = model(image.cuda(), sos_t, False, attn_beam=W, attn_lm=(handle, alpha, beta, top_n))
            index, experts = np.zeros(B, dtype=np.int64), [model]
            feats = [out["feature"].cpu()]
    refs = [decoding.attn_beam_host(e.Prediction.state_dict(), f, 2, 3, W, L, want_margin=True, lm=lm, lm_weight=alpha, lm_bonus=beta,
                                    top_n=top_n) for e, f in zip(experts, feats)]
    margins = np.array([refs[int(index[b])][7][b] for b in range(B)])
    print(f"margins of the routed experts' references: {np.array2string(margins, precision=3)} (decisive from {3 * TOKEN_BAND})")
    assert decisive(margins).all()                                         # a decisive batch
    path, prob = out["beam_path"].cpu().numpy(), out["beam_prob"].cpu().numpy()
    assert path.shape == (B, L + 1) and prob.shape == (B, L + 1) and "beam_word" not in out
    rows = np.stack([refs[int(index[b])][4][b] for b in range(B)])
    probs = np.stack([refs[int(index[b])][5][b] for b in range(B)])
    assert np.array_equal(path, rows)
    # the eight values the unchanged scorer makes of those best entries
    strings = conv.decode(rows, [L + 1] * B)
    scored = _host_scores(list(LABELS), strings, probs, True, True)
    terms = [t for t, _, _ in scored if t is not None]
    valid_loss, accuracy, ned, preds_str, confidence, labels, n_data = fused
    assert valid_loss == greedy[0]                                         # the greedy decoder's logits
    assert accuracy == sum(bool(ok) for _, ok, _ in scored) / B * 100
    assert abs(ned - sum(terms) / B * 100) < 1e-9
    assert preds_str == strings and labels == list(LABELS) and n_data == B
    for b in range(B):
        want, kept = kept_confidence(conv, refs[int(index[b])], b)
        assert abs(want - scored[b][2]) <= 1e-5 * want                       # (the scorer's float32 running product)
        print(f"sample {b}: expert {int(index[b])}, {kept} kept probabilities, confidence {confidence[b]:.6e}, reference {want:.6e}")
        assert abs(confidence[b] - want) <= want * (np.exp(max(kept, 1) * TOKEN_BAND) - 1) + 1e-12, b
