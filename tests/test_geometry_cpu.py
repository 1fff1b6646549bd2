"""48- and 64-pixel input heights on the CPU: the pure-Python predicate behind the HIP path's refusals, and the CPU oracle against
the reference's own outputs at those heights (tests/golden/geometry.npz, written by tests/golden/make_golden_geom.py) -- what makes
the oracle the yardstick of tests/test_geometry_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mrn_amd.modules.geometry import geometry_supported, unsupported_geometry_message
from tests.helpers import assert_close, assert_sub_close, load_golden


def test_supported_heights_for_vgg_and_resnet():
    for feat, trans in (("VGG", "None"), ("ResNet", "TPS"), ("ResNet", "None"), ("VGG", "TPS")):
        for h in (32, 48, 64):
            assert geometry_supported(feat, h, 256, trans), (feat, trans, h)


def test_unsupported_geometries():
    assert not geometry_supported("ResNet", 40, 256, "TPS")
    assert not geometry_supported("VGG", 40, 256)
    assert not geometry_supported("ResNet", 96, 256, "TPS")
    assert not geometry_supported("VGG", 128, 256)
    assert not geometry_supported("SVTR", 64, 256)
    assert not geometry_supported("SVTR", 48, 256)
    assert not geometry_supported("ResNet", 48, 100)
    assert geometry_supported("SVTR", 32, 256)          # every extractor at the configs' 32 x 256


def test_refusal_names_the_supported_set():
    msg = unsupported_geometry_message("TPS", "ResNet", 96, 256, 5)
    assert "imgH in {32, 48, 64} at imgW = 256" in msg and "VGG / ResNet" in msg and "96 x 256" in msg


# ---- the CPU oracle against the reference's outputs at imgH = 48 / 64 (tests/golden/make_golden_geom.py) ----------------------
GEOM_CASES = {"trba": (("TPS", "ResNet", "BiLSTM", "Attn"), (41, 71), 51), "crnn": (("None", "VGG", "BiLSTM", "CTC"), (40, 70), 52)}


def _geom_state_dict(g, p, seed):
    from mrn_amd.tools import weights as W
    sd = {}
    for k, shp in zip(g[p + "sd_keys"], g[p + "sd_shapes"]):
        k = str(k)
        shape = tuple(int(v) for v in str(shp).split(",")) if str(shp) else ()
        sd[k] = torch.from_numpy(np.array(W.det_param(W.canonical_key(k), shape, seed)))
    return sd


def _geom_targets(kind, imgH, classes, seed, B=4):
    """the generator's inputs (make_golden_geom.py: targets)"""
    from mrn_amd.tools import weights as W
    image = torch.from_numpy(W.smooth_image(f"geom:{kind}:{imgH}", (B, 4, imgH, 256), seed))
    if kind == "trba":
        text = torch.from_numpy(W.randint(f"geom:text:{imgH}", (B, 27), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None
    lens = torch.from_numpy(W.randint(f"geom:len:{imgH}", (B,), 1, 26, seed)).int()
    labels = torch.from_numpy(W.randint(f"geom:ctc:{imgH}", (B, 25), 4, classes[-1], seed))
    labels[torch.arange(25)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


@pytest.mark.parametrize("kind", ["trba", "crnn"])
@pytest.mark.parametrize("imgH", [48, 64])
def test_oracle_matches_reference_at_height(kind, imgH):
    from oracle import mrn_oracle as O
    g = load_golden("geometry")
    p = f"{kind}{imgH}/"
    stages, classes, seed = GEOM_CASES[kind]
    cfg = O.Cfg(*stages, imgH=imgH)
    sd = _geom_state_dict(g, p, seed)
    image, tgt, lens = _geom_targets(kind, imgH, classes, seed)
    attn = kind == "trba"
    text = tgt[:, :-1] if attn else None
    assert int(g[p + "featmap_shape"][2]) == {48: 2, 64: 3}[imgH]          # the final map really has 2 / 3 rows
    with torch.no_grad():
        x = image
        if attn:
            inv, ph = O.tps_constants(20, (imgH, 256))
            assert_close("inv_delta_C", inv, g[p + "tps/inv_delta_C"], atol=1e-6, rtol=1e-6)
            assert_sub_close(g, p + "tps/P_hat", ph, atol=1e-6, rtol=1e-6)
            x = O.tps_forward(_geom_state_dict(g, p, seed), "model.0.model.Transformation.", image, True)
            assert_sub_close(g, p + "tps_out", x, atol=1e-5)
        fwd = O.resnet_forward if attn else O.vgg_forward
        fm = fwd(_geom_state_dict(g, p, seed), "model.0.model.FeatureExtraction.", x, True)
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
    sd = _geom_state_dict(g, p, seed)
    with torch.no_grad():
        ob = O.mrn_forward(sd, cfg, 2, image, True, text, True, training=True)
    assert_close("routing weights", ob["index"], g[p + "stepB/weights"], atol=1e-5)
    assert_sub_close(g, p + "stepB/logits", ob["logits"], atol=2e-5)
    # eval: hard routing and greedy indices, bit-exact
    sd = _geom_state_dict(g, p, seed)
    with torch.no_grad():
        oe = O.mrn_forward(sd, cfg, 2, image, True, torch.LongTensor(4).fill_(2) if attn else None, False, training=False)
    assert np.array_equal(oe["index"].numpy(), g[p + "eval/index"])
    assert_sub_close(g, p + "eval/logits", oe["logits"], atol=2e-5)
    assert np.array_equal(oe["logits"].max(2)[1].numpy(), g[p + "eval/argmax"])
