"""Hidden sizes 128 / 256 / 512 on the CPU: the pure-Python predicate and message behind the HIP path's refusals, the fragment-major
packers' index formulas at 128 and 512, and the CPU oracle at Cfg(hidden_size=...) against the reference's own outputs
(tests/golden/hidden.npz, written by tests/golden/make_golden_hidden.py) -- what makes the oracle the yardstick of
tests/test_hidden_gpu.py.  Bands of the oracle cases: those of tests/test_width_cpu.py for the same quantities."""
import numpy as np
import pytest
import torch

from mrn_amd.modules import hidden_size as HS
from mrn_amd.modules.hidden_size import hidden_supported, unsupported_hidden_message
from tests.helpers import assert_close, assert_sub_close, drop_masks, load_golden

STAGES = {"crnn": ("None", "VGG", "BiLSTM", "CTC"), "svtr": ("None", "SVTR", "None", "CTC")}
CLASSES = (40, 70)
HIDDEN_CASES = (("crnn", 128, 128, 4, 71), ("crnn", 512, 128, 4, 72), ("svtr", 128, 256, 2, 73))      # kind, hidden, imgW, B, seed


def test_supported_set_and_predicate_grid():
    assert HS.SUPPORTED_HIDDEN == (128, 256, 512)
    for seq in ("BiLSTM", "None", None):
        for h in (128, 256, 512):
            assert hidden_supported(seq, "CTC", h), (seq, h)
            assert hidden_supported(seq, "Attn", h) == (h == 256), (seq, h)
        for h in (64, 192, 384, 1024):
            assert not hidden_supported(seq, "CTC", h), (seq, h)
            assert not hidden_supported(seq, "Attn", h), (seq, h)


def test_message_names_the_set_and_the_attention_head():
    msg = unsupported_hidden_message("BiLSTM", "Attn", 128)
    assert "[128, 256, 512]" in msg and "attention head runs 256 only" in msg and "hidden_size=128" in msg and "Prediction=Attn" in msg
    msg = unsupported_hidden_message("BiLSTM", "CTC", 192)
    assert "[128, 256, 512]" in msg and "hidden_size=192" in msg
    HS.check_hidden("BiLSTM", "CTC", 512)
    HS.check_hidden("None", "CTC", 128)
    HS.check_hidden("BiLSTM", "Attn", 256)
    for seq, pred, h in (("BiLSTM", "Attn", 128), ("BiLSTM", "Attn", 512), ("BiLSTM", "CTC", 192), ("None", "CTC", 64)):
        with pytest.raises(NotImplementedError, match=r"\[128, 256, 512\].*attention head runs 256 only"):
            HS.check_hidden(seq, pred, h)


def test_models_refuse_before_anything_is_built():
    import contextlib
    import io
    import types
    from mrn_amd.modules.model import DERNet, MRNNet
    for stages, h in ((("TPS", "ResNet", "BiLSTM", "Attn"), 128), (("None", "VGG", "BiLSTM", "CTC"), 192)):
        o = types.SimpleNamespace(num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=h, batch_max_length=25)
        o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = stages
        for cls in (MRNNet, DERNet):
            with contextlib.redirect_stdout(io.StringIO()), pytest.raises(NotImplementedError, match=r"\[128, 256, 512\]"):
                net = cls(o)                                  # (DERNet builds its first extractor here, MRNNet in update_fc)
                net.update_fc(h, 41)


# ---- the packers' documented index formulas ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [128, 512])
@pytest.mark.parametrize("transposed", [False, True])
def test_pack_fragment_major_round_trip(hidden, transposed):
    """packed[w][g][q][lane = gg*16 + n][r] = W[g*hidden + 16w + n][16q + 4gg + r]: W_hh [4H, H] (four gate groups) and W_hh^T [H, 4H]
    (one group) of an LSTM layer, unpacked element by element through the formula"""
    from mrn_amd import ops
    g = torch.Generator().manual_seed(hidden)
    w = torch.randn(4 * hidden, hidden, generator=g)
    if transposed:
        w = w.t().contiguous()
    G, K = w.shape[0] // hidden, w.shape[1]
    p = ops.pack_fragment_major(w, hidden)
    assert p.shape == (hidden // 16, G, K // 16, 4, 16, 4) and p.is_contiguous()
    back = torch.empty_like(w)
    wi, gi, qi, gg, n, r = torch.meshgrid(*[torch.arange(s) for s in p.shape], indexing="ij")
    back[gi * hidden + 16 * wi + n, 16 * qi + 4 * gg + r] = p
    assert torch.equal(back, w)
    flat = p.reshape(hidden // 16, G, K // 16, 64, 4)                     # (the lane axis as the kernels index it)
    assert torch.equal(flat[hidden // 16 - 1, G - 1, 2, 37], w[(G - 1) * hidden + hidden - 16 + 5, 32 + 8:32 + 12])


@pytest.mark.parametrize("hidden", [128, 512])
def test_pack_fragment_major_keeps_its_256_layout(hidden):
    """the 256 layout is the slice of the generic one: packing at 256 is unchanged, and a wider matrix's tiles follow in order"""
    from mrn_amd import ops
    w = torch.randn(4 * 256, 256, generator=torch.Generator().manual_seed(1))
    v = w.reshape(4, 16, 16, 16, 4, 4).permute(1, 0, 3, 4, 2, 5).contiguous()
    assert torch.equal(ops.pack_fragment_major(w), v) and torch.equal(ops.pack_fragment_major(w, 256), v)
    with pytest.raises(AssertionError):
        ops.pack_fragment_major(torch.zeros(4 * hidden + 8, hidden), hidden)


# ---- the CPU oracle against the reference's outputs at other hidden sizes (tests/golden/make_golden_hidden.py) --------------------
def hidden_state_dict(g, p, seed):
    from mrn_amd.tools import weights as W
    sd = {}
    for k, shp in zip(g[p + "sd_keys"], g[p + "sd_shapes"]):
        k = str(k)
        shape = tuple(int(v) for v in str(shp).split(",")) if str(shp) else ()
        sd[k] = torch.from_numpy(np.array(W.det_param(W.canonical_key(k), shape, seed)))
    return sd


def hidden_targets(kind, hidden, imgW, B, seed):
    """the generator's inputs (make_golden_hidden.py: targets)"""
    from mrn_amd.tools import weights as W
    image = torch.from_numpy(W.smooth_image(f"hidden:{kind}:{hidden}", (B, 4, 32, imgW), seed))
    lens = torch.from_numpy(W.randint(f"hidden:len:{kind}:{hidden}", (B,), 1, 26, seed)).int()
    labels = torch.from_numpy(W.randint(f"hidden:ctc:{kind}:{hidden}", (B, 25), 4, CLASSES[-1], seed))
    labels[torch.arange(25)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


def hidden_masks(kind, hidden, B, seed, tag, n=1):
    """the DropPath draws the generator injected (SVTR only)"""
    return drop_masks(B, seed, f"hidden{hidden}:{tag}", n) if kind == "svtr" else None


@pytest.mark.parametrize("kind,hidden,imgW,B,seed", HIDDEN_CASES)
def test_oracle_matches_reference_at_hidden(kind, hidden, imgW, B, seed):
    from oracle import mrn_oracle as O
    g = load_golden("hidden")
    p = f"{kind}{hidden}/"
    cfg = O.Cfg(*STAGES[kind], imgH=32, imgW=imgW, hidden_size=hidden)
    sd = hidden_state_dict(g, p, seed)
    image, tgt, lens = hidden_targets(kind, hidden, imgW, B, seed)
    shapes = dict(zip(map(str, g[p + "sd_keys"]), map(str, g[p + "sd_shapes"])))
    assert shapes["model.1.fc.weight"] == f"70,{hidden}" and shapes["channel_route.weight"] == f"2,{2 * hidden}"
    assert shapes["dm_router.0.proj_1.weight"] == f"{2 * hidden},{hidden}"
    if kind == "crnn":
        assert shapes["model.0.model.SequenceModeling.0.rnn.weight_hh_l0"] == f"{4 * hidden},{hidden}"
    else:
        assert shapes["model.0.model.SequenceModeling.0.weight"] == f"{hidden},512"
    with torch.no_grad():
        m = hidden_masks(kind, hidden, B, seed, "e0")
        feat = O.model_forward(sd, "model.0.", cfg, image, None, True, training=True, masks=m[0] if m else None)["feature"]
        assert feat.shape == (B, 31 if kind == "crnn" else 64, hidden)
        assert_sub_close(g, p + "e0/feature", feat, atol=2e-5)
    # loop A: the newest expert's logits, loss and parameter gradients
    sd = hidden_state_dict(g, p, seed)
    names = [str(k)[len(p + "stepA/grad/"):] for k in g.files if k.startswith(p + "stepA/grad/") and k.endswith("/sub")]
    names = [n[:-len("/sub")] for n in names]
    assert len(names) == 4
    params = [sd[n].requires_grad_(True) for n in names]
    m = hidden_masks(kind, hidden, B, seed, "stepA")
    out = O.mrn_forward(sd, cfg, 2, image, False, None, True, training=True, masks=[None, m[0]] if m else None)["logits"]
    loss = O.ctc_loss(out, tgt, lens)
    grads = torch.autograd.grad(loss, params)
    assert_sub_close(g, p + "stepA/logits", out, atol=2e-5)
    assert abs(loss.item() - float(g[p + "stepA/loss"])) <= 1e-5 * max(1.0, abs(float(g[p + "stepA/loss"])))
    for n, gr in zip(names, grads):
        assert_sub_close(g, p + "stepA/grad/" + n, gr, atol=1e-6, rtol=2e-3)
    # loop B forward: routing weights and fused logits
    sd = hidden_state_dict(g, p, seed)
    with torch.no_grad():
        ob = O.mrn_forward(sd, cfg, 2, image, True, None, True, training=True, masks=hidden_masks(kind, hidden, B, seed, "stepB", 2))
    assert_close("routing weights", ob["index"], g[p + "stepB/weights"], atol=1e-5)
    assert_sub_close(g, p + "stepB/logits", ob["logits"], atol=2e-5)
    # eval: hard routing and argmax, bit-exact
    sd = hidden_state_dict(g, p, seed)
    with torch.no_grad():
        oe = O.mrn_forward(sd, cfg, 2, image, True, None, False, training=False)
    assert np.array_equal(oe["index"].numpy(), g[p + "eval/index"])
    assert_sub_close(g, p + "eval/logits", oe["logits"], atol=2e-5)
    assert np.array_equal(oe["logits"].max(2)[1].numpy(), g[p + "eval/argmax"])
