"""Input widths 128 ... 512 on the CPU: the pure-Python predicate, frame count and per-call pixel budget behind the HIP path's
refusals, and the CPU oracle against the reference's own outputs at 32 x 128, 32 x 512, 48 x 320 and 64 x 192
(tests/golden/width.npz, written by tests/golden/make_golden_width.py) -- what makes the oracle the yardstick of
tests/test_width_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mrn_amd.modules import geometry as Geo
from mrn_amd.modules.geometry import frames, geometry_supported, unsupported_geometry_message
from tests.helpers import assert_close, assert_sub_close, load_golden

WIDTHS = (128, 192, 256, 320, 384, 448, 512)
HEIGHTS = (32, 48, 64)


def test_supported_widths_for_vgg_and_resnet():
    assert Geo.SUPPORTED_WIDTHS == WIDTHS and Geo.SUPPORTED_WIDTH == 256
    for feat, trans in (("VGG", "None"), ("ResNet", "TPS"), ("ResNet", "None"), ("VGG", "TPS")):
        for h in HEIGHTS:
            for w in WIDTHS:
                assert geometry_supported(feat, h, w, trans), (feat, trans, h, w)


def test_other_extractors_stay_at_32x256():
    for feat in ("SVTR", "RCNN"):
        for h in HEIGHTS:
            for w in WIDTHS:
                assert geometry_supported(feat, h, w) == ((h, w) == (32, 256)), (feat, h, w)


def test_widths_outside_the_set():
    for feat in ("VGG", "ResNet", "SVTR", "RCNN"):
        for trans in ("None", "TPS"):
            for h in HEIGHTS:
                for w in (64, 96, 100, 576):
                    assert not geometry_supported(feat, h, w, trans), (feat, trans, h, w)


def test_frames_follow_the_width():
    for w in WIDTHS:
        assert frames("VGG", w) == w // 4 - 1 and frames("ResNet", w) == w // 4 + 1
    assert (frames("VGG", 256), frames("SVTR", 256), frames("ResNet", 256)) == (63, 64, 65)
    g = load_golden("width")
    for kind, feat in (("trba", "ResNet"), ("crnn", "VGG")):
        for h, w in GEOMETRIES:
            assert frames(feat, w) == int(g[f"{kind}{h}x{w}/featmap_shape"][3]), (kind, h, w)


def test_pixel_budget_edge():
    assert Geo.MAX_CALL_PIXELS == 256 * 64 * 256 == 4194304
    assert Geo.call_in_budget(256, 32, 512) and Geo.call_in_budget(256, 64, 256) and Geo.call_in_budget(128, 64, 512)
    assert not Geo.call_in_budget(129, 64, 512) and not Geo.call_in_budget(256, 64, 512) and not Geo.call_in_budget(257, 64, 256)
    Geo.check_call("TPS", "ResNet", 128, 64, 512)
    with pytest.raises(NotImplementedError, match="4194304") as e:
        Geo.check_call("TPS", "ResNet", 129, 64, 512)
    assert "B = 129 at 64 x 512" in str(e.value)


def test_refusals_name_the_set_and_the_budget():
    msg = unsupported_geometry_message("TPS", "ResNet", 32, 100, 1)
    assert "imgH in {32, 48, 64} at imgW = 256" in msg and "VGG / ResNet" in msg and "32 x 100" in msg
    assert "{128, 192, 256, 320, 384, 448, 512}" in msg and "4194304" in msg
    msg = Geo.over_budget_message(256, 64, 512)
    assert "4194304" in msg and "B = 256 at 64 x 512" in msg
    for feat, h, w in (("VGG", 32, 100), ("ResNet", 32, 576), ("SVTR", 32, 128)):
        with pytest.raises(NotImplementedError, match=r"\{128, 192, 256, 320, 384, 448, 512\}"):
            Geo.check_call("None", feat, 2, h, w)


# ---- the CPU oracle against the reference's outputs at other widths (tests/golden/make_golden_width.py) ----------------------
WIDTH_CASES = {"trba": (("TPS", "ResNet", "BiLSTM", "Attn"), (41, 71), 61), "crnn": (("None", "VGG", "BiLSTM", "CTC"), (40, 70), 62)}
GEOMETRIES = ((32, 128), (32, 512), (48, 320), (64, 192))


def _width_state_dict(g, p, seed):
    from mrn_amd.tools import weights as W
    sd = {}
    for k, shp in zip(g[p + "sd_keys"], g[p + "sd_shapes"]):
        k = str(k)
        shape = tuple(int(v) for v in str(shp).split(",")) if str(shp) else ()
        sd[k] = torch.from_numpy(np.array(W.det_param(W.canonical_key(k), shape, seed)))
    return sd


def _width_targets(kind, imgH, imgW, classes, seed, B=4):
    """the generator's inputs (make_golden_width.py: targets)"""
    from mrn_amd.tools import weights as W
    image = torch.from_numpy(W.smooth_image(f"width:{kind}:{imgH}x{imgW}", (B, 4, imgH, imgW), seed))
    if kind == "trba":
        text = torch.from_numpy(W.randint(f"width:text:{imgH}x{imgW}", (B, 27), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None
    lens = torch.from_numpy(W.randint(f"width:len:{imgH}x{imgW}", (B,), 1, 26, seed)).int()
    labels = torch.from_numpy(W.randint(f"width:ctc:{imgH}x{imgW}", (B, 25), 4, classes[-1], seed))
    labels[torch.arange(25)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


@pytest.mark.parametrize("kind", ["trba", "crnn"])
@pytest.mark.parametrize("imgH,imgW", GEOMETRIES)
def test_oracle_matches_reference_at_width(kind, imgH, imgW):
    from oracle import mrn_oracle as O
    g = load_golden("width")
    p = f"{kind}{imgH}x{imgW}/"
    stages, classes, seed = WIDTH_CASES[kind]
    cfg = O.Cfg(*stages, imgH=imgH, imgW=imgW)
    sd = _width_state_dict(g, p, seed)
    image, tgt, lens = _width_targets(kind, imgH, imgW, classes, seed)
    attn = kind == "trba"
    text = tgt[:, :-1] if attn else None
    assert int(g[p + "featmap_shape"][2]) == {32: 1, 48: 2, 64: 3}[imgH]
    assert int(g[p + "featmap_shape"][3]) == frames(stages[1], imgW)
    with torch.no_grad():
        x = image
        if attn:
            inv, ph = O.tps_constants(20, (imgH, imgW))
            assert_close("inv_delta_C", inv, g[p + "tps/inv_delta_C"], atol=1e-6, rtol=1e-6)
            assert_sub_close(g, p + "tps/P_hat", ph, atol=1e-6, rtol=1e-6)
            x = O.tps_forward(_width_state_dict(g, p, seed), "model.0.model.Transformation.", image, True)
            assert_sub_close(g, p + "tps_out", x, atol=1e-5)
        fwd = O.resnet_forward if attn else O.vgg_forward
        fm = fwd(_width_state_dict(g, p, seed), "model.0.model.FeatureExtraction.", x, True)
        v = fm.permute(0, 3, 1, 2)
        v = F.adaptive_avg_pool2d(v, (v.shape[2], 1)).squeeze(3)           # (as oracle.extractor_forward pools)
        assert_sub_close(g, p + "visual", v, atol=2e-5)
    # loop A: the newest expert's logits, loss and parameter gradients
    names = [str(k)[len(p + "stepA/grad/"):] for k in g.files if k.startswith(p + "stepA/grad/") and k.endswith("/sub")]
    names = [n[:-len("/sub")] for n in names]
    params = [sd[n].requires_grad_(True) for n in names]
    out = O.mrn_forward(sd, cfg, 2, image, False, text, True, training=True)["logits"]
    loss = O.attn_ce_loss(out, tgt) if attn else O.ctc_loss(out, tgt, lens)
    grads = torch.autograd.grad(loss, params)
    assert_sub_close(g, p + "stepA/logits", out, atol=2e-5)
    assert abs(loss.item() - float(g[p + "stepA/loss"])) <= 1e-5 * max(1.0, abs(float(g[p + "stepA/loss"])))
    for n, gr in zip(names, grads):
        assert_sub_close(g, p + "stepA/grad/" + n, gr, atol=1e-6, rtol=2e-3)
    # loop B forward: routing weights and fused logits
    sd = _width_state_dict(g, p, seed)
    with torch.no_grad():
        ob = O.mrn_forward(sd, cfg, 2, image, True, text, True, training=True)
    assert_close("routing weights", ob["index"], g[p + "stepB/weights"], atol=1e-5)
    assert_sub_close(g, p + "stepB/logits", ob["logits"], atol=2e-5)
    # eval: hard routing and greedy indices, bit-exact
    sd = _width_state_dict(g, p, seed)
    with torch.no_grad():
        oe = O.mrn_forward(sd, cfg, 2, image, True, torch.LongTensor(4).fill_(2) if attn else None, False, training=False)
    assert np.array_equal(oe["index"].numpy(), g[p + "eval/index"])
    assert_sub_close(g, p + "eval/logits", oe["logits"], atol=2e-5)
    assert np.array_equal(oe["logits"].max(2)[1].numpy(), g[p + "eval/argmax"])
