"""Host side of language-model fusion in the attention head's beam search (no kernel is launched): the C ABI of include/mrn_attn_lm.h,
the options, the float64 host form attn_beam_host(lm=) against the plain one and against hand-computed keys, the LDS rule, and the
reference cases tests/test_decode_attn_lm_gpu.py decodes: how many of their samples are decisive is a property of the reference alone.

The cases stand on the fixtures of tests/test_attn_beam_cpu.py (beam_fixture and the shapes of BEAM_CASES).  Fixture seed, generator
scale, model seed and lm_weight are chosen so that at most B // 4 samples are non-decisive under the extended margin (key gaps and the
pruning boundary); a model is lm_from_rows on seeded random rows over the classes 4 ... C_lm - 1."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import BEAM_CASES, EOS, SOS, TOKEN_BAND, beam_fixture, decisive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_ENTRY = ("mrn_attn_beam_lm_decode_grouped_f32", "mrn_attn_beam_lm_decode_x3_grouped")
LM_BONUS = 0.05
# name (the shapes of BEAM_CASES[name]): (fixture seed0, generator weight scale, order, top_n, C_lm, model seed, lm_weight)
LM_CASES = {
    "c97_w4": (200, 100.0, 3, 15, 97, 1, 0.2),
    "c331_w8": (512, 400.0, 2, 15, 331, 1, 0.3),                 # ragged last class tile; B ends inside a workgroup
    "c37_w3": (300, 50.0, 3, 5, 37, 2, 0.2),                     # W does not divide 16; N = 5
    "d512_w16": (1001, 400.0, 1, 15, 1045, 1, 0.2),              # order 1, N = 16
    "t127_c5374_w8": (100, 50.0, 3, 15, 2091, 1, 0.2),           # C_lm < C: classes outside the model
}
_REF = {}


def random_lm(C_lm, order, seed, n=300):
    """lm_from_rows on n seeded random rows of 1 ... 11 classes out of 4 ... C_lm - 1"""
    from mrn_amd.modules.char_lm import lm_from_rows
    rng = np.random.default_rng(seed)
    rows = [rng.integers(4, C_lm, size=int(rng.integers(1, 12))).tolist() for _ in range(n)]
    return lm_from_rows(rows, C_lm, order)


def lm_case(name):
    """(sd, Hb, model, reference outputs of attn_beam_host(lm=) with the margin) of a case, computed once and shared (never modified)"""
    if name not in _REF:
        from mrn_amd.modules import decoding
        B, T, D, C, S, W, _, _ = BEAM_CASES[name]
        seed0, scale, order, top_n, C_lm, lm_seed, alpha = LM_CASES[name]
        sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
        lm = random_lm(C_lm, order, lm_seed)
        ref = decoding.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1, want_margin=True, lm=lm, lm_weight=alpha, lm_bonus=LM_BONUS, top_n=top_n)
        _REF[name] = (sd, Hb, lm, ref)
    return _REF[name]


PLANT = dict(B=1, T=31, D=256, C=97, seed0=200, scale=100.0, first=40, second=11, delta=1e-3, alpha=0.2, beta=0.05)


def planted_case():
    """one sample, one step (S = 1), width 1: the logits of classes `first` and `second` are lifted 10 above every other class and set
    delta = 1e-3 apart (five times a token's band), and a bigram model has seen `second` at the start of a text fifty times as often
    -> (sd, Hb, model, the log-probability of `second` under the planted head)"""
    from mrn_amd.modules import decoding
    from mrn_amd.modules.char_lm import lm_from_rows
    p = PLANT
    sd, Hb = beam_fixture(p["B"], p["T"], p["D"], p["C"], p["seed0"], p["scale"])
    sd = {k: v.double() for k, v in sd.items()}
    tokens, _, score, _, _, _ = decoding.attn_beam_host(sd, Hb, SOS, EOS, p["C"], 0)           # every class of the one step
    lp = np.empty(p["C"])
    lp[tokens[0, :, 0]] = score[0]
    sd["generator.bias"][p["first"]] += lp.max() + 10.0 - lp[p["first"]]
    sd["generator.bias"][p["second"]] += lp.max() + 10.0 - p["delta"] - lp[p["second"]]
    lm = lm_from_rows([[p["second"], 20]] * 50 + [[p["first"], 20]] + [[30, 31, 32]] * 5, p["C"], 2)
    tokens, _, score, _, _, _ = decoding.attn_beam_host(sd, Hb, SOS, EOS, 2, 0)
    assert tokens[0, :, 0].tolist() == [p["first"], p["second"]] and abs(score[0, 0] - score[0, 1] - p["delta"]) < 1e-9
    return sd, Hb, lm, float(score[0, 1])


def test_entry_points_are_declared_bound_exported_and_cited():
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.ATTN_LM_HEADER_PATH)
    assert tuple(protos) == LM_ENTRY
    others = [_lib.HEADER_PATH, _lib.DECODE_HEADER_PATH, _lib.ATTN_BEAM_HEADER_PATH, _lib.LEXICON_HEADER_PATH, _lib.ATTN_LEXICON_HEADER_PATH,
              _lib.ATTN_SCORE_HEADER_PATH, _lib.SHORTLIST_HEADER_PATH, _lib.HERDING_HEADER_PATH, _lib.CTC_LM_HEADER_PATH]
    for path in others:
        assert not set(protos) & set(_lib.parse_header(path)), path
    dll = ctypes.CDLL(_lib.LIB_PATH)
    loaded = _lib.LIB.load()
    header = open(_lib.ATTN_LM_HEADER_PATH).read()
    beam = _lib.parse_header(_lib.ATTN_BEAM_HEADER_PATH)
    ctc = _lib.parse_header(_lib.CTC_LM_HEADER_PATH)["mrn_ctc_beam_lm_decode_f32"]
    model = ctc[2][ctc[2].index("lm_keys"):ctc[2].index("fused")]
    assert model == ["lm_keys", "lm_vals", "lm_mask", "lm_max_probe", "uni_logp", "uni_bow", "C_lm", "unk_logp", "order", "alpha", "beta"]
    for name, plain in zip(LM_ENTRY, ("mrn_attn_beam_decode_grouped_f32", "mrn_attn_beam_decode_x3_grouped")):
        ret, argtypes, argnames = protos[name]
        assert hasattr(dll, name) and name in _lib.LIB._protos
        bound = getattr(loaded, name)
        assert bound.restype is ctypes.c_int and len(bound.argtypes) == len(argnames)
        assert ret == "int" and argnames[-2:] == ["hidden", "stream"]
        base = beam[plain][2]
        cut, out = base.index("W") + 1, base.index("groups")
        # the operands of the plain entry point, then top_n and the model's operands, then its outputs and fused
        assert argnames == base[:cut] + ["top_n"] + model + base[cut:out] + ["fused"] + base[out:]
        assert [argtypes[argnames.index(a)] for a in model] == [ctc[1][ctc[2].index(a)] for a in model]
        assert ("w_inv" in argnames) == ("x3" in name)
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "modules/prediction.py:70-86" in comment, name
        for limit in ("1 <= W <= 16", "1 <= top_n <= 16", "1 <= S <= 512", "2 <= num_class <= 65535", "hidden = 256",
                      "multiple of " + ("32" if "x3" in name else "16")):
            assert limit in comment, (name, limit)
    first = header[:header.index("int " + LM_ENTRY[0] + "(")]
    for limit in ("1 <= C_lm <= 65535", "power of two <= 2^26", "0 <= lm_max_probe <= lm_mask + 1", "1 <= order <= 3", "alpha >= 0",
                  "alpha, beta and unk_logp finite"):
        assert limit in first, limit
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`include/mrn_attn_lm.h`" in readme and "mrn_attn_beam_lm_decode_grouped_f32" in readme
    # the hash stays stated in one device file, and char_lm.py names it
    csrc = os.path.join(ROOT, "mrn_amd", "csrc")
    stated = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".cpp")) and "0xBF58476D1CE4E5B9" in open(os.path.join(csrc, f)).read()]
    assert stated == ["char_lm.hpp"]
    from mrn_amd.modules import char_lm
    assert "mrn_amd/csrc/char_lm.hpp (lm_mix)" in char_lm.__doc__ and "ctc_beam.hip" not in char_lm.__doc__


def test_rule_matches_the_launch_helper():
    """ops.attn_beam_lm_whole_context restates the launch's LDS sum in csrc/attn_decode.hip (the beam's plus LM_LDS_MORE), every limit is
    checked before the first launch, and the three kernels share one body"""
    from mrn_amd import ops
    src = open(os.path.join(ROOT, "mrn_amd", "csrc", "attn_decode.hip")).read()
    consts = dict(re.findall(r"(?m)^constexpr int (\w+) = ([^;]+);", src))
    assert re.sub(r"\s+", " ", consts["LM_LDS_MORE"]).strip() == "4 * (8 * BT + 2 * BT * BT)"
    assert ops.ATTN_BEAM_LM_LDS_EXTRA == ops.ATTN_BEAM_LDS_EXTRA + 4 * (8 * 16 + 2 * 16 * 16) == 3584 + 2560
    launch = re.sub(r"\s+", " ", src[src.index("static int beam_launch("):src.index("static int beam_grouped(")])
    assert "+ (lm ? LM_LDS_MORE : 0)" in launch and "CTX_CHUNK" not in launch
    body = re.sub(r"\s+", " ", src[src.index("static int beam_grouped("):src.index("MRN_EXPORT int mrn_attn_beam_decode_grouped_f32")])
    for check in ("attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA + LM_LDS_MORE) <= 160 * 1024", "m.top_n >= 1 && m.top_n <= BT",
                  "m.order >= 1 && m.order <= 3", "m.C_lm >= 1 && m.C_lm <= CHAR_LM_MAX_C", "((m.mask + 1) & m.mask) == 0",
                  "(int64_t)m.max_probe <= m.mask + 1", "isfinite(m.alpha) && m.alpha >= 0.f && isfinite(m.beta)",
                  "o.num_class[g] <= CHAR_LM_MAX_C"):
        assert check in body and body.index(check) < body.index("beam_launch("), check
    assert src.count("void attn_beam_body(") == 1 and src.count("attn_beam_body<X3, false, true>(grp") == 1
    for T in (17, 65, 129):
        for x3 in (True, False):
            for D in list(range(32, 2600, 32)) + [48, 264]:
                for W in (0, 1, 3, 16, 17):
                    lds = 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + (1024 if x3 else 0) + 3584 + 2560
                    want = lds <= 160 * 1024 and 1 <= W <= 16 and D % (32 if x3 else 16) == 0
                    assert ops.attn_beam_lm_whole_context(D, T, W, x3) == want, (D, T, W, x3)
    assert ops.attn_beam_lm_whole_context(1792, 65, 8, True) and not ops.attn_beam_lm_whole_context(2304, 65, 8, True)


def test_options():
    from mrn_amd.modules import decoding as D
    lm = random_lm(40, 2, 0, n=20)
    off = (None, 0.5, 0.0, 15)
    assert D.attn_lm_options(SimpleNamespace(), True) == off
    assert D.attn_lm_options(SimpleNamespace(attn_lm=None, attn_decode="beam"), True) == off
    assert D.attn_lm_options(SimpleNamespace(attn_lm=lm, attn_decode="beam"), True) == (lm, 0.5, 0.0, 15)
    opt = SimpleNamespace(attn_lm=lm, attn_decode="beam", lm_weight=0.25, lm_bonus=-1, beam_top_n=np.int64(7))
    assert D.attn_lm_options(opt, True) == (lm, 0.25, -1.0, 7)
    # CTC heads ignore the option, whatever stands beside it; the attention head ignores ctc_lm
    assert D.attn_lm_options(SimpleNamespace(attn_lm=lm), False) == off
    assert D.attn_lm_options(SimpleNamespace(attn_lm="no model", lexicon=["a"], candidates={}), False) == off
    assert D.lm_options(SimpleNamespace(ctc_lm=lm), True) == (None, 0.5, 0.0)
    with pytest.raises(ValueError, match="attn_lm must be a CharLM"):
        D.attn_lm_options(SimpleNamespace(attn_lm="no model", attn_decode="beam"), True)
    for opt in (SimpleNamespace(attn_lm=lm), SimpleNamespace(attn_lm=lm, attn_decode="greedy")):
        with pytest.raises(ValueError, match="attn_decode='beam'"):
            D.attn_lm_options(opt, True)
    for key, value in (("attn_lexicon", ["word"]), ("candidates", {}), ("lexicon_shortlist", 4)):
        with pytest.raises(ValueError, match="attn_lm and " + key):
            D.attn_lm_options(SimpleNamespace(attn_lm=lm, attn_decode="beam", **{key: value}), True)
    for bad in (dict(lm_weight=-0.1), dict(lm_weight=float("nan")), dict(lm_bonus=float("inf")), dict(lm_weight="1")):
        with pytest.raises(ValueError, match="lm_weight|lm_bonus"):
            D.attn_lm_options(SimpleNamespace(attn_lm=lm, attn_decode="beam", **bad), True)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="beam_top_n"):
            D.attn_lm_options(SimpleNamespace(attn_lm=lm, attn_decode="beam", beam_top_n=bad), True)
    # the evaluation forwards' keyword
    handle = SimpleNamespace(lm=lm, keys=None)
    req = D.attn_search_request("Attn", False, attn_beam=4, attn_lm=(handle, 0.5, 0, 15))
    assert req is None                                                     # grad is enabled here: nothing is decoded a second time
    with torch.no_grad():
        req = D.attn_search_request("Attn", False, attn_beam=4, attn_lm=(handle, 0.5, 0, 15))
        assert req == D.AttnFusedSearch(4, (handle, 0.5, 0.0, 15)) and req != D.AttnFusedSearch(4, (handle, 0.25, 0.0, 15))
        assert isinstance(req, D.AttnSearch) and req.kind == "beam" and req.width == 4 and req.lm == (handle, 0.5, 0.0, 15) and not req.has_word
        assert D.attn_search_request("Attn", False, attn_beam=4) == D.AttnSearch("beam", width=4) and D.AttnSearch("beam", width=4).lm is None
        assert D.attn_search_request("CTC", False, attn_beam=4, attn_lm=(handle, 0.5, 0, 15)) is None
        with pytest.raises(ValueError, match="attn_beam=<width>"):
            D.attn_search_request("Attn", False, attn_lm=(handle, 0.5, 0, 15))
        for kw in (dict(attn_lexicon=object()), dict(attn_candidates=object()), dict(attn_shortlist=(object(), 2, None))):
            with pytest.raises(ValueError, match="closed-vocabulary"):
                D.attn_search_request("Attn", False, attn_beam=4, attn_lm=(handle, 0.5, 0, 15), **kw)
        for bad in (handle, (handle, 0.5, 0), (lm, 0.5, 0, 15), (handle, -1, 0, 15), (handle, 0.5, 0, 0)):
            with pytest.raises(ValueError):
                D.attn_search_request("Attn", False, attn_beam=4, attn_lm=bad)
    assert D.attn_lm_proposals(4, 15) == 15 and D.attn_lm_proposals(8, 5) == 8 and D.attn_lm_proposals(3, 40) == 16
    assert D.attn_lm_proposals(16, 1) == 16 and D.attn_lm_proposals(20, 15) == 20


@pytest.mark.parametrize("name,top_n", [("c37_w3", 3), ("c37_w3", 5), ("c37_w3", 16), ("c97_w4", 4), ("c97_w4", 15)])
def test_zero_weights_are_the_plain_search(name, top_n):
    """lm=None is attn_beam_host; alpha = beta = 0 at any top_n >= W gives its six outputs element for element, and fused = score"""
    from mrn_amd.modules import decoding as D
    B, T, Dm, C, S, W, _, _ = BEAM_CASES[name]
    sd, Hb, lm, _ = lm_case(name)
    plain = D.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1)
    assert len(plain) == 6
    same = D.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1, lm=None, lm_weight=0.7, lm_bonus=0.3, top_n=top_n)
    zero = D.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1, lm=lm, lm_weight=0.0, lm_bonus=0.0, top_n=top_n)
    assert len(same) == 6 and len(zero) == 7
    for a, b, c in zip(plain, same, zero):
        assert a.dtype == b.dtype == c.dtype and np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(zero[6], plain[2])


def test_planted_preference_flips_the_best_entry():
    from mrn_amd.modules import decoding as D
    p = PLANT
    sd, Hb, lm, lp_second = planted_case()
    plain = D.attn_beam_host(sd, Hb, SOS, EOS, 1, 0)
    fused = D.attn_beam_host(sd, Hb, SOS, EOS, 1, 0, lm=lm, lm_weight=p["alpha"], lm_bonus=p["beta"], top_n=2)
    assert plain[0][0, 0, 0] == p["first"] and fused[0][0, 0, 0] == p["second"]
    gain = p["alpha"] * (lm.logp(0, 0, p["second"]) - lm.logp(0, 0, p["first"]))
    print(f"delta {p['delta']:.1e} (band {TOKEN_BAND:.1e}), the model's preference is worth {gain:.3f}")
    assert p["delta"] >= 3 * TOKEN_BAND and gain > 100 * p["delta"]
    assert abs(fused[2][0, 0] - lp_second) < 1e-12                         # score stays acoustic (rows of another batch: the last bits)
    want = lp_second + p["alpha"] * lm.logp(0, 0, p["second"]) + p["beta"] * 1
    assert abs(fused[6][0, 0] - want) < 1e-12
    assert fused[4][0, 0] == p["second"] and abs(fused[5][0, 0] - np.exp(lp_second)) < 1e-6


def test_unk_and_eos_terms_and_the_context():
    """C = 8, two steps, every hypothesis kept (W = 64 >= 1 + 7 * 8): fused - score of every entry is the hand-computed model part.
    Class 0 scores unk_logp flat and reads as begin of text to its successor; eos scores logp(a, b, 0), adds no length and ends the
    entry, whose key the second step leaves alone"""
    from mrn_amd.modules import decoding as D
    from mrn_amd.modules.char_lm import lm_from_rows
    C, W, alpha, beta = 8, 64, 0.3, 0.07
    sd, Hb = beam_fixture(2, 5, 16, C, 900, 10.0)
    lm = lm_from_rows([[4, 5, 6], [4, 5], [6, 7, 4], [5, 5, 6, 4], [7]], C, 3)
    tokens, length, score, logp, path, prob, fused = D.attn_beam_host(sd, Hb, SOS, EOS, W, 1, lm=lm, lm_weight=alpha, lm_bonus=beta, top_n=8)
    seen = set()
    for b in range(2):
        assert np.all(length[b, :57] >= 1) and np.all(length[b, 57:] == -1) and np.all(np.isneginf(fused[b, 57:]))
        assert np.all(fused[b, :56] >= fused[b, 1:57])                     # descending fused
        for w in range(57):
            k1, k2 = map(int, tokens[b, w])
            seen.add((k1, k2))
            if k1 == EOS:
                assert k2 == EOS and length[b, w] == 1
                model, chars = lm.logp(0, 0, 0), 0
            else:
                first = lm.unk_logp if k1 == 0 else lm.logp(0, 0, k1)
                ctx = (0, k1)                                              # a predicted 0 is begin of text to its successor
                second = lm.logp(*ctx, 0) if k2 == EOS else lm.unk_logp if k2 == 0 else lm.logp(*ctx, k2)
                model, chars = first + second, 1 + (k2 != EOS)
            assert abs(fused[b, w] - (score[b, w] + alpha * model + beta * chars)) < 1e-12, (b, w, k1, k2)
            assert abs(score[b, w] - logp[b, w].sum()) < 1e-12
    assert len(seen) == 57 and (0, 0) in seen and (0, 4) in seen and (4, 0) in seen and (4, EOS) in seen
    assert lm.unk_logp != lm.logp(0, 0, 0) and lm.logp(0, 4, 5) != lm.logp(0, 0, 5)


def test_reference_cases_are_decisive_enough():
    """at most B // 4 samples of a GPU case may be left to the self-consistency check alone under the extended margin (key gaps and the
    pruning boundary); fixture seed, generator scale, model seed and lm_weight are chosen so that the reference meets that"""
    from mrn_amd.modules import decoding as D
    assert set(LM_CASES) == set(BEAM_CASES)
    for name, (B, T, Dm, C, S, W, _, _) in BEAM_CASES.items():
        seed0, scale, order, top_n, C_lm, lm_seed, alpha = LM_CASES[name]
        sd, Hb, lm, ref = lm_case(name)
        tokens, length, score, logp, path, prob, fused, margin = ref
        plain = D.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1)
        moved = int((tokens != plain[0]).any(axis=(1, 2)).sum())
        loose = int((~decisive(margin)).sum())
        print(f"{name}: {loose} of {B} samples are not decisive (cap {B // 4}); smallest margin {margin.min():.3e}; the model changes the "
              f"entries of {moved} samples")
        assert loose <= B // 4, name
        assert lm.order == order and lm.C_lm == C_lm and D.attn_lm_proposals(W, top_n) == min(16, max(W, top_n))
        assert tokens.shape == (B, W, S) and fused.shape == (B, W) and np.all(length[:, 0] >= 1) and moved >= 1
        live = length >= 0
        assert np.all(np.isneginf(fused[~live])) and np.all(np.isfinite(fused[live]))
        assert np.all(np.where(live[:, 1:], fused[:, :-1] >= fused[:, 1:], True))
    assert LM_CASES["t127_c5374_w8"][4] < BEAM_CASES["t127_c5374_w8"][3] and int(lm_case("t127_c5374_w8")[3][0].max()) >= 2091
