"""Greedy decoding on the attention head in one launch (mrn_attn_greedy_decode*, csrc/attn_decode.hip attn_greedy_kernel) against the CPU oracle's
step loop (reference modules/prediction.py:70-86), and the fused launch against itself across its forms.

Greedy feedback turns a flipped near-tie into a different sequence, so every oracle comparison first asserts that the ORACLE's smallest
top-1 / top-2 logit gap over all (sample, step) pairs is at least 3e-4 -- three times the 1e-4 band the logits are held to -- and then
demands every index equal and every logit inside the band, nothing left out."""
import contextlib
import io
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

HID = 256
MIN_GAP = 3e-4
# B, T, D, C, S, seed0
CASES = {
    "c331": (19, 31, 256, 331, 12, 3300),          # 21 class tiles: several passes per wave, the last tile ragged; B ends inside a workgroup
    "c203": (19, 31, 256, 203, 12, 1200),
    "c97": (19, 31, 256, 97, 12, 600),
    "t65": (19, 65, 256, 331, 26, 1500),
    "wide2304": (5, 65, 2304, 203, 6, 500),        # the WIDE form: three context chunks (1024, 1024, 256)
    "d512": (37, 17, 512, 1045, 8, 600),
    "t127_c5374": (3, 127, 256, 5374, 4, 500),
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def fixture(B, T, D, C, seed0):
    """(state dict, Hb) built like tests/test_kernels_gpu.py::test_attention_decoder"""
    from mrn_amd.modules.prediction import Attention
    att = Attention(D, HID, C, nn.Linear(HID, C))
    sd = {k: rnd(*v.shape, seed=seed0 + i, scale=0.08) for i, (k, v) in enumerate(att.state_dict().items())}
    sd["char_embeddings.weight"] = rnd(C, 256, seed=seed0 + 37)
    return sd, rnd(B, T, D, seed=seed0 + 1)


def module(sd, D, C):
    from mrn_amd.modules.prediction import Attention
    att = Attention(D, HID, C, nn.Linear(HID, C))
    att.load_state_dict(sd)
    return att.cuda()


_REF = {}


def case(name):
    """(sd, Hb, oracle logits) of a case, computed once and shared (never modified)"""
    if name not in _REF:
        from oracle import mrn_oracle as O
        B, T, D, C, S, seed0 = CASES[name]
        sd, Hb = fixture(B, T, D, C, seed0)
        osd = {"P." + k: v for k, v in sd.items()}
        ref = O.attention_forward(osd, "P.", Hb, torch.LongTensor(B).fill_(2), False, S - 1, sd["generator.weight"], sd["generator.bias"])
        _REF[name] = (sd, Hb, ref)
    return _REF[name]


def check_against_oracle(name, out):
    ref = case(name)[2]
    top = ref.topk(2, dim=2).values
    gap = (top[..., 0] - top[..., 1]).min().item()
    print(f"{name}: oracle top-1 / top-2 gap {gap:.3e}")
    assert gap >= MIN_GAP, f"{name}: the oracle's own top-1 / top-2 gap {gap:.3e} is below {MIN_GAP}"
    print(f"{name}: max |logits - oracle| {(out.cpu() - ref).abs().max().item():.3e}")
    assert np.array_equal(out.argmax(2).cpu().numpy(), ref.argmax(2).numpy())
    assert_close("greedy logits " + name, out, ref, atol=1e-4)


def forward(name):
    B, T, D, C, S, _ = CASES[name]
    sd, Hb, _ = case(name)
    att = module(sd, D, C)
    with torch.no_grad():
        return att(Hb.cuda(), torch.LongTensor(B).fill_(2).cuda(), False, S - 1)


def decode(ops, att, Hb, start, S, **kw):
    """ops.attn_greedy_decode on a module's operands"""
    with torch.no_grad():
        Hproj = ops.linear(Hb, att.attention_cell.i2h.weight)
        etab, w_h2h, b_h2h, w_score, w_ih, w_hh, b_hh, w_gen, b_gen, w_inv = att.greedy_args()
        return ops.attn_greedy_decode(Hb, Hproj, etab, start, w_h2h, b_h2h, w_score, w_ih, w_hh, b_hh, w_gen, b_gen, HID, S, w_inv=w_inv, **kw)


def sos(v=2):
    return torch.tensor([v], dtype=torch.int64).cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_single_expert_matches_the_oracle(ops, monkeypatch, name):
    """the default (split-fp16 x3) form through Attention.forward(is_train=False); D = 2304 takes the WIDE form"""
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    monkeypatch.delenv("MRN_ATTN_CTX_CHUNK", raising=False)
    B, T, D, C, S, _ = CASES[name]
    assert ops.attn_greedy_whole_context(D, T) == (D != 2304)
    check_against_oracle(name, forward(name))


@pytest.mark.parametrize("name", ["c331", "wide2304"])
def test_exact_fp32_form_matches_the_oracle(ops, monkeypatch, name):
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", False)
    check_against_oracle(name, forward(name))


@pytest.mark.parametrize("x3", [True, False])
def test_chunked_context_equals_the_whole_context_bit_for_bit(ops, monkeypatch, x3):
    """MRN_ATTN_CTX_CHUNK=1 takes the WIDE form at D = 256 (one chunk of 256 columns): the same sums in the same order"""
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    monkeypatch.delenv("MRN_ATTN_CTX_CHUNK", raising=False)
    whole = forward("c331")
    monkeypatch.setenv("MRN_ATTN_CTX_CHUNK", "1")
    chunked = forward("c331")
    assert torch.equal(whole, chunked)
    if x3:
        check_against_oracle("c331", chunked)


def test_tokens_out_and_unknown_start_token(ops):
    B, T, D, C, S, _ = CASES["c331"]
    sd, Hb, _ = case("c331")
    att = module(sd, D, C)
    out, tok = decode(ops, att, Hb.cuda(), sos(2), S, want_tokens=True)
    assert tok.dtype == torch.int64 and tuple(tok.shape) == (B, S)
    assert torch.equal(tok, out.argmax(2))
    check_against_oracle("c331", out)
    zero, tok0 = decode(ops, att, Hb.cuda(), sos(0), S, want_tokens=True)
    unknown, toku = decode(ops, att, Hb.cuda(), sos(C + 1), S, want_tokens=True)      # cut_unknown: decodes like token 0
    assert torch.equal(zero, unknown) and torch.equal(tok0, toku)
    assert not torch.equal(zero, out)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("other", [7, 300])
def test_ties_go_to_the_lowest_index(ops, monkeypatch, x3, other):
    """class 5's generator row and bias copied to a second class -- in the same 16-class tile (7), then in a tile another wave owns
    (300: tile 18, wave 2) -- and both lifted above every other class: every step must return 5, as torch.max / mrn_argmax_f32 do"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, _ = CASES["c331"]
    sd, Hb, _ = case("c331")
    sd = {k: v.clone() for k, v in sd.items()}
    sd["generator.weight"][other] = sd["generator.weight"][5]
    sd["generator.bias"][5] += 1.0
    sd["generator.bias"][other] = sd["generator.bias"][5]
    att = module(sd, D, C)
    out, tok = decode(ops, att, Hb.cuda(), sos(2), S, want_tokens=True)
    assert torch.equal(out[:, :, 5], out[:, :, other])
    assert torch.equal(tok, torch.full_like(tok, 5))
    assert torch.equal(ops.argmax_lastdim(out.contiguous()), tok)


def grouped_fixture(G, B, T, S):
    classes = [(97, 331, 203)[g % 3] for g in range(G)]
    atts, Hbs = [], []
    for g, C in enumerate(classes):
        sd, Hb = fixture(B, T, 256, C, 7000 + 100 * g)
        atts.append(module(sd, 256, C))
        Hbs.append(Hb)
    return classes, atts, torch.stack(Hbs).cuda()


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("G", [3, 9])
def test_grouped_equals_single_launches(ops, monkeypatch, G, x3):
    """ragged class counts (97, 331, 203) in one launch; nine experts take two launches (MAX_GROUPS = 8).  Bit-identical to one
    launch per expert, logits in padded-row views whose strides differ with the class count"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, S = 19, 31, 12
    classes, atts, Hb = grouped_fixture(G, B, T, S)
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
        outs = [ops.padded_rows(B, S, C, Hb.device) for C in classes]
        _, tokens = ops.attn_greedy_decode_grouped(Hb, Hproj, cols[0], sos(2), *cols[1:9], HID, S, outs, want_tokens=True,
                                                   w_inv=cols[9] if x3 else None)
    assert (cols[9][0] is not None) == x3
    for g, a in enumerate(atts):
        one, tok = decode(ops, a, Hb[g], sos(2), S, want_tokens=True)
        assert torch.equal(outs[g], one), f"expert {g}"
        assert torch.equal(tokens[g], tok), f"expert {g}"


@pytest.mark.parametrize("x3", [True, False])
def test_samples_per_workgroup_do_not_change_a_row(ops, monkeypatch, x3):
    """MRN_GREEDY_VB = 2 (ten workgroups, the last one half full) against 16 (two workgroups): a row's arithmetic does not depend on its
    position in the MFMA tile"""
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    B, T, D, C, S, _ = CASES["c331"]
    sd, Hb, _ = case("c331")
    att = module(sd, D, C)
    res = {}
    for vb in ("2", "16"):
        monkeypatch.setenv("MRN_GREEDY_VB", vb)
        res[vb] = decode(ops, att, Hb.cuda(), sos(2), S, want_tokens=True)
    assert torch.equal(res["2"][0], res["16"][0]) and torch.equal(res["2"][1], res["16"][1])
    if x3:
        check_against_oracle("c331", res["2"][0])


def test_strided_output_leaves_the_padding_alone(ops):
    B, T, D, C, S, _ = CASES["c203"]
    sd, Hb, _ = case("c203")
    att = module(sd, D, C)
    ld = (C + 3) // 4 * 4 + 8
    buf = torch.full((B + 1, S + 2, ld), 12345.0).cuda()
    view = buf[:B, 1:S + 1, :C]                          # free batch and step strides, padded rows
    got = decode(ops, att, Hb.cuda(), sos(2), S, out=view)
    assert got.data_ptr() == view.data_ptr()
    check_against_oracle("c203", view)
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:B, 1:S + 1, :C] = False
    assert torch.equal(buf[keep], torch.full_like(buf[keep], 12345.0))
    pad = ops.padded_rows(B, S, C, buf.device)
    decode(ops, att, Hb.cuda(), sos(2), S, out=pad)
    assert torch.equal(pad, view)


def test_validation_forward_issues_one_greedy_launch(ops, monkeypatch):
    """cross=True, is_train=False on three TRBA experts: ONE mrn_attn_greedy_decode* call and none of the step loop's calls; under
    MRN_GREEDY_DECODE=stepwise the old calls instead; the same routing index both ways"""
    from mrn_amd._lib import LIB
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as W
    opt = types.SimpleNamespace(Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM", Prediction="Attn",
                                num_fiducial=20, imgH=32, imgW=128, input_channel=4, output_channel=512, hidden_size=256,
                                batch_max_length=25)
    classes = (30, 45, 61)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(256, c)
            net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed=11)
    net = net.cuda().eval()
    B = 4
    image = torch.from_numpy(W.smooth_image("greedy_wiring", (B, 4, 32, 128), 11)).cuda()
    start = torch.LongTensor(B).fill_(2).cuda()
    counts = {}
    real = LIB.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(LIB, "call", counting)

    def run(mode):
        counts.clear()
        if mode is None:
            monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
        else:
            monkeypatch.setenv("MRN_GREEDY_DECODE", mode)
        with torch.no_grad():
            out = net(image, True, start, False)
        torch.cuda.synchronize()
        return out, dict(counts)

    def total(c, prefix):
        return sum(v for k, v in c.items() if k.startswith(prefix))

    fused, cf = run(None)
    assert total(cf, "mrn_attn_greedy_decode") == 1, cf
    assert total(cf, "mrn_attn_decoder_fwd") == 0 and cf.get("mrn_embed_gather_f32", 0) == 0 and cf.get("mrn_argmax_f32", 0) == 0, cf
    step, cs = run("stepwise")
    S = opt.batch_max_length + 1
    assert total(cs, "mrn_attn_greedy_decode") == 0, cs
    assert total(cs, "mrn_attn_decoder_fwd") == 3 * S and cs["mrn_embed_gather_f32"] == 3 * S and cs["mrn_argmax_f32"] == 3 * S, cs
    assert torch.equal(fused["index"], step["index"])
    assert tuple(fused["logits"].shape) == tuple(step["logits"].shape)
