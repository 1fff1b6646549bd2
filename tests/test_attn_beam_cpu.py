"""Host side of beam-search decoding on the attention head (no kernel is launched): the options, the float64 reference attn_beam_host
against the oracle (greedy at width 1, an exhaustive search on a tiny head), the C ABI of include/mrn_attn_beam.h, the LDS rule, and
the reference cases tests/test_decode_attn_beam_gpu.py decodes: how many of their samples are decisive is a property of the reference alone."""
import ctypes
import itertools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAM = ("mrn_attn_beam_decode_grouped_f32", "mrn_attn_beam_decode_x3_grouped")
SOS, EOS = 2, 1
TOKEN_BAND = 2e-4        # logits are held to 1e-4 of the oracle, so a chosen token's log-probability (logit - lse) to 2e-4
# name: (B, T, D, C, S, W, seed0, generator weight scale).  The scale makes the distributions peaked: the gaps between candidates grow
# with it, and so does the number of decisive samples
BEAM_CASES = {
    "c97_w4": (19, 31, 256, 97, 12, 4, 200, 100.0),
    "c331_w8": (19, 31, 256, 331, 12, 8, 500, 400.0),              # ragged last class tile; B ends inside a workgroup (2 samples each)
    "d512_w16": (5, 17, 512, 1045, 8, 16, 1000, 400.0),             # one sample per workgroup
    "c37_w3": (7, 31, 256, 37, 12, 3, 300, 50.0),                 # W does not divide 16: five samples and an unused row per workgroup
    "t127_c5374_w8": (3, 127, 256, 5374, 4, 8, 100, 50.0),
}
_REF = {}


def beam_fixture(B, T, D, C, seed0, scale):
    """(state dict, Hb) of tests/test_greedy_decode_gpu.py::fixture with the generator weight scaled"""
    from tests.test_greedy_decode_gpu import fixture
    sd, Hb = fixture(B, T, D, C, seed0)
    sd["generator.weight"] = sd["generator.weight"] * scale
    return sd, Hb


def beam_case(name):
    """(sd, Hb, reference outputs of attn_beam_host with the margin) of a case, computed once and shared (never modified)"""
    if name not in _REF:
        from mrn_amd.modules import decoding
        B, T, D, C, S, W, seed0, scale = BEAM_CASES[name]
        sd, Hb = beam_fixture(B, T, D, C, seed0, scale)
        _REF[name] = (sd, Hb, decoding.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1, want_margin=True))
    return _REF[name]


def decisive(margin):
    """samples whose every gap (neighbouring kept candidates, last kept against best dropped) is at least 3 x the step's band: the
    margin is the smallest gap divided by the step's token count, the band of a score of n tokens n * TOKEN_BAND"""
    return np.asarray(margin) >= 3 * TOKEN_BAND


def test_attention_decode_options():
    from mrn_amd.modules import decoding as D
    assert D.ATTN_DECODERS == ("greedy", "beam")
    assert D.attn_decode_options(SimpleNamespace()) == ("greedy", 8)
    assert D.attn_decode_options(SimpleNamespace(attn_decode="beam")) == ("beam", 8)
    assert D.attn_decode_options(SimpleNamespace(attn_decode="beam", beam_width=3)) == ("beam", 3)
    assert D.attn_decode_options(SimpleNamespace(attn_decode="greedy", beam_width=np.int64(5))) == ("greedy", 5)
    for bad in ("Beam", "", None, "prefix"):
        with pytest.raises(ValueError, match="attn_decode"):
            D.attn_decode_options(SimpleNamespace(attn_decode=bad))
    for bad in (0, -1, 2.0, True, "8"):
        with pytest.raises(ValueError, match="beam_width"):
            D.attn_decode_options(SimpleNamespace(attn_decode="beam", beam_width=bad))
    # the CTC options do not read the new key
    assert D.decode_options(SimpleNamespace(attn_decode="beam")) == ("greedy", 8, 15)


def test_switch_parsing(monkeypatch):
    from mrn_amd import ops
    monkeypatch.delenv("MRN_ATTN_BEAM", raising=False)
    assert ops.attn_beam_mode() == "fused"
    for value, mode in (("", "fused"), ("fused", "fused"), ("stepwise", "stepwise")):
        monkeypatch.setenv("MRN_ATTN_BEAM", value)                        # read per call
        assert ops.attn_beam_mode() == mode
    for bad in ("0", "step", "Fused"):
        monkeypatch.setenv("MRN_ATTN_BEAM", bad)
        with pytest.raises(ValueError, match="MRN_ATTN_BEAM"):
            ops.attn_beam_mode()


def test_width_one_is_greedy_decoding():
    """attn_beam_host at W = 1 against the oracle's greedy loop, on a case whose oracle top-1 / top-2 gap is at least 3e-4"""
    from mrn_amd.modules import decoding as D
    from oracle import mrn_oracle as O
    from tests.test_greedy_decode_gpu import CASES, fixture
    B, T, Dm, C, S, seed0 = CASES["c97"]
    sd, Hb = fixture(B, T, Dm, C, seed0)
    osd = {"P." + k: v for k, v in sd.items()}
    ref = O.attention_forward(osd, "P.", Hb, torch.LongTensor(B).fill_(SOS), False, S - 1, sd["generator.weight"], sd["generator.bias"])
    top = ref.topk(2, dim=2).values
    assert (top[..., 0] - top[..., 1]).min().item() >= 3e-4
    greedy = ref.argmax(2).numpy()
    tokens, length, score, logp, path, prob = D.attn_beam_host(sd, Hb, SOS, EOS, 1, S - 1)
    assert tokens.shape == (B, 1, S) and tokens.dtype == np.int32 and length.shape == (B, 1) and path.dtype == np.int64
    lsm = torch.log_softmax(ref.double(), dim=2).numpy()
    for b in range(B):
        n = int(length[b, 0])
        first = np.flatnonzero(greedy[b] == EOS)
        assert n == (first[0] + 1 if first.size else S)
        assert np.array_equal(tokens[b, 0, :n], greedy[b, :n]) and np.all(tokens[b, 0, n:] == EOS)
        assert np.array_equal(path[b], tokens[b, 0])
        chosen = lsm[b, np.arange(n), greedy[b, :n]]
        np.testing.assert_allclose(logp[b, 0, :n], chosen, atol=2e-4)      # (the oracle runs in float32)
        assert np.all(logp[b, 0, n:] == 0) and np.all(prob[b, n:] == 1.0)
        assert abs(score[b, 0] - chosen.sum()) <= n * 2e-4


def test_wide_beam_on_a_tiny_head_is_an_exhaustive_search():
    """C = 5, S = 3, W = 100 > 85 hypotheses: every sequence is scored by the teacher-forced oracle in float64, sequences that agree up
    to their first eos are one hypothesis, and attn_beam_host returns exactly those, in descending score"""
    from mrn_amd.modules import decoding as D
    from mrn_amd.modules.prediction import Attention
    from oracle import mrn_oracle as O
    from tests.test_greedy_decode_gpu import rnd
    B, T, Dm, C, S, W = 2, 5, 16, 5, 3, 100
    att = Attention(Dm, 256, C, nn.Linear(256, C))
    sd = {k: rnd(*v.shape, seed=900 + i, scale=0.08).double() for i, (k, v) in enumerate(att.state_dict().items())}
    sd["char_embeddings.weight"] = rnd(C, 256, seed=937).double()
    sd["generator.weight"] = sd["generator.weight"] * 10
    Hb = rnd(B, T, Dm, seed=901).double()
    osd = {"P." + k: v for k, v in sd.items()}
    seqs = list(itertools.product(range(C), repeat=S))
    text = torch.tensor([[SOS] + list(q[:-1]) for q in seqs], dtype=torch.int64)
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)             # the oracle's zero state follows the default dtype
    try:
        lsm = []
        for b in range(B):
            logits = O.attention_forward(osd, "P.", Hb[b:b + 1].expand(len(seqs), T, Dm), text, True, S - 1, sd["generator.weight"],
                                         sd["generator.bias"])
            assert logits.dtype == torch.float64
            lsm.append(torch.log_softmax(logits, dim=2).numpy())
    finally:
        torch.set_default_dtype(default)
    tokens, length, score, logp, path, prob = D.attn_beam_host(sd, Hb, SOS, EOS, W, S - 1)
    for b in range(B):
        hyps = {}
        for n, q in enumerate(seqs):
            cut = q.index(EOS) + 1 if EOS in q else S
            key = tuple(q[:cut]) + (EOS,) * (S - cut)
            total = sum(lsm[b][n, s, q[s]] for s in range(cut))
            assert key not in hyps or abs(hyps[key] - total) < 1e-12
            hyps[key] = total
        assert len(hyps) == 85
        ranked = sorted(hyps.items(), key=lambda kv: -kv[1])
        assert (length[b] >= 0).sum() == 85 and np.all(length[b, 85:] == -1) and np.all(np.isneginf(score[b, 85:]))
        assert np.all(tokens[b, 85:] == EOS) and np.all(logp[b, 85:] == 0)
        for w, (key, total) in enumerate(ranked):
            assert tuple(tokens[b, w]) == key, (b, w)
            assert abs(score[b, w] - total) < 1e-9
            cut = key.index(EOS) + 1 if EOS in key else S
            assert length[b, w] == cut and abs(logp[b, w, :cut].sum() - total) < 1e-9
        assert np.array_equal(path[b], tokens[b, 0])
        np.testing.assert_allclose(prob[b], np.exp(logp[b, 0]), rtol=1e-6)


def test_reference_cases_are_decisive_enough():
    """at most B // 4 samples of a GPU case may be left to the self-consistency check alone; seeds and generator scale are chosen so
    that the reference meets that"""
    for name, (B, T, D, C, S, W, _, _) in BEAM_CASES.items():
        tokens, length, score, logp, path, prob, margin = beam_case(name)[2]
        loose = int((~decisive(margin)).sum())
        print(f"{name}: {loose} of {B} samples are not decisive (cap {B // 4}); smallest margin {margin.min():.3e}")
        assert loose <= B // 4, name
        assert tokens.shape == (B, W, S) and np.all(length[:, 0] >= 1)


def test_entry_points_are_declared_bound_exported_and_cited():
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.ATTN_BEAM_HEADER_PATH)
    assert tuple(protos) == BEAM
    assert not set(protos) & (set(_lib.parse_header()) | set(_lib.parse_header(_lib.DECODE_HEADER_PATH)))
    dll = ctypes.CDLL(_lib.LIB_PATH)
    loaded = _lib.LIB.load()
    header = open(_lib.ATTN_BEAM_HEADER_PATH).read()
    greedy = _lib.parse_header()["mrn_attn_greedy_decode_x3_grouped"][2]
    for name in BEAM:
        ret, argtypes, argnames = protos[name]
        assert hasattr(dll, name) and name in _lib.LIB._protos
        bound = getattr(loaded, name)
        assert bound.restype is ctypes.c_int and len(bound.argtypes) == len(argnames)
        assert ret == "int" and argnames[-2:] == ["hidden", "stream"]
        for a in ("eos", "W", "scratch", "tokens", "length", "score", "logp", "path", "prob", "groups"):
            assert a in argnames, (name, a)
        operands = [a for a in greedy[:greedy.index("num_class") + 1] if "x3" in name or a != "w_inv"]
        assert argnames[:len(operands)] == operands                # the operands of the grouped greedy entry points, in their order
        assert ("w_inv" in argnames) == ("x3" in name)
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "modules/prediction.py:70-86" in comment, name
        for limit in ("1 <= W <= 16", "1 <= S <= 512", "num_class >= 2", "hidden = 256", "multiple of " + ("32" if "x3" in name else "16")):
            assert limit in comment, (name, limit)
    # the other two headers keep their counts
    assert len(_lib.parse_header()) == 156 and len(_lib.parse_header(_lib.DECODE_HEADER_PATH)) == 1


def test_rule_matches_the_launch_helper():
    """ops.attn_beam_whole_context restates the beam launch's LDS sum in csrc/attn_decode.hip (the tile of attn_tile_lds, the three decoder
    kernels' one definition, at dc = D plus BEAM_LDS_EXTRA) and the limits beam_grouped checks before any launch"""
    from mrn_amd import ops
    src = open(os.path.join(ROOT, "mrn_amd", "csrc", "attn_decode.hip")).read()
    flat = re.sub(r"\s+", " ", src[src.index("static size_t attn_tile_lds("):src.index("static dim3 attn_grid(")])
    assert "(bool x3, int dc, int T, size_t extra)" in flat
    assert "sizeof(float) * (2 * BT * HLD + BT * (dc + 4) + BT * T + HID) + (x3 ? 1024 : 0) + extra" in flat
    launch = re.sub(r"\s+", " ", src[src.index("static int beam_launch("):src.index("static int beam_grouped(")])
    assert "lds = attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA)" in launch and "CTX_CHUNK" not in launch
    body = re.sub(r"\s+", " ", src[src.index("static int beam_grouped("):src.index("MRN_EXPORT int mrn_attn_beam_decode_grouped_f32")])
    fits = "attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA) <= 160 * 1024"
    assert fits in body and "W >= 1 && W <= BT" in body and "S >= 1 && S <= 512" in body
    assert body.index(fits) < body.index("beam_launch(")      # refused before the first launch
    consts = dict(re.findall(r"(?m)^constexpr int (\w+) = ([^;]+);", src))
    assert re.sub(r"\s+", " ", consts["BEAM_LDS_EXTRA"]).strip() == "4 * (8 * BT + 3 * BT * BT)"
    assert ops.ATTN_BEAM_LDS_EXTRA == 4 * (8 * 16 + 3 * 16 * 16) == 3584
    for T in (17, 65, 129):
        for x3 in (True, False):
            for D in list(range(32, 2600, 32)) + [48, 264]:
                for W in (0, 1, 3, 16, 17):
                    lds = 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + (1024 if x3 else 0) + 3584
                    want = lds <= 160 * 1024 and 1 <= W <= 16 and D % (32 if x3 else 16) == 0
                    assert ops.attn_beam_whole_context(D, T, W, x3) == want, (D, T, W, x3)
    assert ops.attn_beam_whole_context(1792, 65, 8, True) and not ops.attn_beam_whole_context(2304, 65, 8, True)
    assert src.index("void attn_greedy_kernel(") < src.index("void embed_gather_kernel(") < src.index("void attn_beam_kernel(")
    assert src.count("template <bool X3>\n__global__ __launch_bounds__(NTH) void attn_beam_kernel(const BeamGroup grp)") == 1


def test_config_loader_passes_the_key_through(tmp_path):
    from mrn_amd.tiny_train import load_config
    cfg = tmp_path / "cfg.py"
    cfg.write_text('common = dict(Prediction="Attn")\nmodel = dict(attn_decode="beam", beam_width=4)\n')
    opt = load_config(str(cfg))
    from mrn_amd.modules import decoding as D
    assert D.attn_decode_options(opt) == ("beam", 4)
