"""48- and 64-pixel input heights on the GPU: the height-mean kernels against torch, the CRNN / TRBA MRN stacks against the CPU
oracle at imgH = 48 / 64 (forward, loop A, loop B, DER, reduced mode), the largest supported batch, the refusal of heights
outside the supported set, and the training driver end to end.  Inputs are built here (tests/helpers.det_inputs is 32 x 256)."""
import contextlib
import io
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import assert_close, oracle_dtype

pytestmark = pytest.mark.gpu

CLASSES = {"crnn": (40, 70, 97), "trba": (41, 71, 98)}
CFG = {"crnn": ("None", "VGG", "BiLSTM", "CTC"), "trba": ("TPS", "ResNet", "BiLSTM", "Attn")}


def make_opt(kind, imgH):
    o = types.SimpleNamespace(num_fiducial=20, imgH=imgH, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=25)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = CFG[kind]
    return o


def build_mrn(kind, imgH, classes, seed):
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as W
    opt = make_opt(kind, imgH)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed=seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return opt, net.cuda(), sd


def inputs(kind, imgH, B, classes, seed):
    from mrn_amd.tools import weights as W
    image = torch.from_numpy(W.smooth_image(f"geom_{kind}_{imgH}", (B, 4, imgH, 256), seed))
    if kind == "trba":
        text = torch.from_numpy(W.randint(f"geom_text_{imgH}", (B, 27), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None
    lens = torch.from_numpy(W.randint(f"geom_len_{imgH}", (B,), 1, 26, seed)).int()
    labels = torch.from_numpy(W.randint(f"geom_ctc_{imgH}", (B, 25), 4, classes[-1], seed))
    labels[torch.arange(25)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


def _grad_check(name, mine, ref, rel_l2=2e-3, rel_max=2e-3):
    a = mine.detach().cpu().double().numpy()
    b = ref.detach().double().numpy()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(np.abs(b).max(), 1e-12)
    l2 = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)
    mx = np.abs(a - b).max() / scale
    assert l2 <= rel_l2 and mx <= rel_max, f"{name}: rel L2 {l2:.2e}, rel max {mx:.2e} (|g|max {scale:.2e})"


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [2, 3, 5])
@pytest.mark.parametrize("W", [63, 65])
@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("affine", [False, True])
def test_height_mean_kernel_vs_torch(H, W, C, affine):
    from mrn_amd import ops
    g = torch.Generator().manual_seed(H * 1000 + W + C)
    B = 3
    x = torch.randn(B, H, W, C, generator=g)
    sc = torch.rand(C, generator=g) + 0.5 if affine else None
    sh = torch.randn(C, generator=g) if affine else None
    t = torch.relu(x * sc + sh) if affine else x
    ref = F.adaptive_avg_pool2d(t.permute(0, 3, 1, 2).permute(0, 3, 1, 2), (None, 1)).squeeze(3)     # NCHW -> the reference's permute + pool
    xd = x.cuda()
    if affine:
        out, hl = ops.height_mean_grouped(xd.view(1, B, H, W, C), sc.cuda().view(1, C), sh.cuda().view(1, C), relu=True, want_hl=True)
    else:
        out, hl = ops.height_mean_grouped(xd.view(1, B, H, W, C), want_hl=True)
    out = out.view(B, W, C)
    assert_close("height mean", out, ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(hl, ops.split_hl32(out))                 # the HL32 result is the split of the fp32 one
    if not affine:
        assert torch.equal(ops.height_mean(xd), out)
    # backward: dx = dy / H on every row, as autograd of adaptive_avg_pool2d
    dy = torch.randn(B, W, C, generator=g)
    xr = x.clone().requires_grad_(True)
    F.adaptive_avg_pool2d(xr.permute(0, 3, 1, 2).permute(0, 3, 1, 2), (None, 1)).squeeze(3).backward(dy)
    dx = ops.height_mean_bwd(dy.cuda(), H)
    assert torch.equal(dx.cpu(), xr.grad)


def test_height_mean_grouped_per_expert_tables():
    from mrn_amd import ops
    g = torch.Generator().manual_seed(9)
    G, B, H, W, C = 4, 5, 3, 65, 512
    x = torch.randn(G, B, H, W, C, generator=g)
    sc = torch.randn(G, C, generator=g)
    sh = torch.randn(G, C, generator=g)
    ref = torch.relu(x * sc[:, None, None, None, :] + sh[:, None, None, None, :]).mean(2)
    out, hl = ops.height_mean_grouped(x.cuda(), sc.cuda(), sh.cuda(), relu=True, want_hl=True)
    assert_close("grouped height mean", out, ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(hl, ops.split_hl32(out))
    only_hl = ops.height_mean_grouped(x.cuda(), sc.cuda(), sh.cuda(), relu=True, want_f32=False, want_hl=True)
    assert only_hl[0] is None and torch.equal(only_hl[1], hl)


# ---- 2. MRN forward (train + eval) against the oracle ----------------------------------------------------------------------
def _mrn_forward_case(kind, imgH, B=32, seed=5):
    from mrn_amd import functional as Fn
    from oracle import mrn_oracle as O
    classes = CLASSES[kind]
    I = len(classes)
    opt, net, sd = build_mrn(kind, imgH, classes, seed)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.")
    image, tgt, lens = inputs(kind, imgH, B, classes, seed)
    domain = torch.from_numpy(np.arange(B) % 2)
    cfg = O.Cfg(*CFG[kind], imgH=imgH)
    attn = kind == "trba"
    text_in = tgt[:, :-1] if attn else None
    names = [n for n in sd if not n.startswith("model.") and sd[n].is_floating_point()]
    sd32 = {k: v.clone() for k, v in sd.items()}
    for n in names:
        sd32[n].requires_grad_(True)
    out32 = O.mrn_forward(sd32, cfg, I, image, True, text_in, True, training=True)
    clf32 = O.attn_ce_loss(out32["logits"], tgt) if attn else O.ctc_loss(out32["logits"], tgt, lens)
    loss32 = 15 * clf32 + F.cross_entropy(out32["index"], domain)
    g32 = torch.autograd.grad(loss32, [sd32[n] for n in names])
    with oracle_dtype(torch.float64) as od, torch.no_grad():
        out64 = O.mrn_forward(od.cast(sd), cfg, I, image.double(), True, text_in, True, training=True)
    w32, l32 = out32["index"].detach(), out32["logits"].detach()
    band_w = float((w32.double() - out64["index"]).abs().max())
    band_l = float((l32.double() - out64["logits"]).abs().max())
    with torch.no_grad():
        handle = net.experts_prefetch(image.cuda(), None if text_in is None else text_in.cuda(), True)
    assert handle is not None
    out = net(image.cuda(), True, None if text_in is None else text_in.cuda(), True, experts=handle)
    if attn:
        clf = Fn.cross_entropy(out["logits"], tgt[:, 1:].cuda(), 1)
    else:
        clf = Fn.ctc_loss(out["logits"], tgt.cuda(), lens.cuda())
    loss = 15 * clf + Fn.cross_entropy(out["index"], domain.cuda(), -100)
    loss.backward()
    w, lg = out["index"].detach().cpu(), out["logits"].detach().cpu()
    scale_l = float(l32.abs().max())
    ew, el = float((w - w32).abs().max()), float((lg - l32).abs().max())
    assert ew <= max(1e-4, 3 * band_w), (ew, band_w)
    assert el <= max(1e-4 * max(1.0, scale_l), 3 * band_l), (el, band_l, scale_l)
    assert abs(float(loss.detach()) - float(loss32.detach())) <= 1e-4 * max(1.0, abs(float(loss32.detach())))
    top2 = out64["index"].sort(1, descending=True)[0]
    clear = (top2[:, 0] - top2[:, 1]) > 10 * max(band_w, 1e-5)
    assert int(clear.sum()) >= B // 2
    assert torch.equal(w.argmax(1)[clear], w32.argmax(1)[clear])
    mine = dict(net.named_parameters())
    for n, gr in zip(names, g32):
        if n == "route.bias":
            continue          # shift-invariant under softmax: its gradient is round-off noise
        tol = max(2e-3, 30 * band_w)
        _grad_check(n, mine[n].grad, gr, rel_l2=tol, rel_max=5 * tol)
    # eval routing + greedy indices, bit-exact where the float64 margin clears the band
    sos = torch.LongTensor(B).fill_(2) if attn else None
    with torch.no_grad():
        oe32 = O.mrn_forward({k: v.detach() for k, v in sd32.items()}, cfg, I, image, True, sos, False, training=False)
    with oracle_dtype(torch.float64) as od, torch.no_grad():
        oe64 = O.mrn_forward(od.cast({k: v.detach() for k, v in sd32.items()}), cfg, I, image.double(), True, sos, False,
                             training=False)
    net.eval()
    with torch.no_grad():
        oe = net(image.cuda(), True, None if sos is None else sos.cuda(), False)
    am, am32 = oe["logits"].max(2)[1].cpu(), oe32["logits"].max(2)[1]
    if attn:
        same = oe["index"].cpu() == oe32["index"]            # greedy decoding feeds its argmax back: compare where routing agrees
        assert float(same.float().mean()) >= 0.9
        assert float((am[same] == am32[same]).float().mean()) >= 0.99
    else:
        assert torch.equal(oe["index"].cpu(), oe32["index"]), (oe["index"].cpu(), oe32["index"])
        l2 = oe64["logits"].topk(2, dim=2)[0]
        clear_l = (l2[..., 0] - l2[..., 1]) > 2e-4 * max(1.0, float(oe64["logits"].abs().max()))
        assert torch.equal(am[clear_l], am32[clear_l])
    del net


@pytest.mark.parametrize("kind", ["crnn", "trba"])
@pytest.mark.parametrize("imgH", [48, 64])
def test_mrn3_batch32_vs_oracle(kind, imgH):
    _mrn_forward_case(kind, imgH)


@pytest.mark.parametrize("kind", ["crnn", "trba"])
@pytest.mark.parametrize("imgH", [48, 64])
def test_mrn2_vs_reference_fixture(kind, imgH):
    """the reference's own outputs (tests/golden/geometry.npz, B = 4, two experts): pooled visual feature, loop-B routing weights
    and fused logits, loop-A logits, eval routing and greedy indices.  Band: 1e-4, or for TRBA -- whose TPS grid is an
    ill-conditioned fp32 sum, and B = 4 train-mode BatchNorm amplifies it -- 3x the distance of the reference's fp32 result from
    float64 arithmetic on the same quantity (as test_model_gpu.py::test_trba_noise_inside_reference_band)"""
    from mrn_amd.modules.model import MRNNet
    from oracle import mrn_oracle as O
    from tests.helpers import load_golden, sub
    from tests.test_geometry_cpu import GEOM_CASES, _geom_state_dict, _geom_targets
    g = load_golden("geometry")
    p = f"{kind}{imgH}/"
    stages, classes, seed = GEOM_CASES[kind]
    attn = kind == "trba"
    opt = make_opt(kind, imgH)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
    image, tgt, _ = _geom_targets(kind, imgH, classes, seed)
    text = tgt[:, :-1] if attn else None
    ref64 = {}
    if attn:
        cfg = O.Cfg(*stages, imgH=imgH)
        with oracle_dtype(torch.float64) as od, torch.no_grad():
            sd = od.cast(_geom_state_dict(g, p, seed))
            fm = O.resnet_forward(sd, "model.0.model.FeatureExtraction.",
                                  O.tps_forward(sd, "model.0.model.Transformation.", image.double(), True), True)
            ref64["visual"] = fm.permute(0, 2, 3, 1).mean(1)
            ob = O.mrn_forward(od.cast(_geom_state_dict(g, p, seed)), cfg, 2, image.double(), True, text, True, training=True)
            ref64["stepB/weights"], ref64["stepB/logits"] = ob["index"], ob["logits"]
            ref64["stepA/logits"] = O.mrn_forward(od.cast(_geom_state_dict(g, p, seed)), cfg, 2, image.double(), False, text, True,
                                                  training=True)["logits"]

    def check(name, t, full=False):
        mine = (t.detach().cpu().double().numpy() if full else sub(t)[0].astype(np.float64))
        ref = g[p + name] if full else g[p + name + "/sub"].astype(np.float64)
        tol = 1e-4 + 1e-4 * np.abs(ref).max()
        if name in ref64:
            r64 = ref64[name].numpy() if full else sub(ref64[name])[0].astype(np.float64)
            tol = max(tol, 3 * np.abs(ref - r64).max())
        err = np.abs(mine - ref).max()
        assert err <= tol, f"{name}: max abs err {err:.3e} > tol {tol:.3e}"

    net.load_state_dict(_geom_state_dict(g, p, seed), strict=True)
    net = net.cuda().train()
    with torch.no_grad():
        check("visual", net.model[0].model.visual(image.cuda()))
        net.load_state_dict(_geom_state_dict(g, p, seed), strict=True)
        out = net(image.cuda(), True, None if text is None else text.cuda(), True)
        check("stepB/weights", out["index"], full=True)
        check("stepB/logits", out["logits"])
        assert np.array_equal(out["index"].cpu().numpy().argmax(1), g[p + "stepB/weights"].argmax(1))
        net.load_state_dict(_geom_state_dict(g, p, seed), strict=True)
        check("stepA/logits", net(image.cuda(), False, None if text is None else text.cuda())["logits"])
        net.load_state_dict(_geom_state_dict(g, p, seed), strict=True)
        net.eval()
        oe = net(image.cuda(), True, torch.LongTensor(4).fill_(2).cuda() if attn else None, False)
    assert np.array_equal(oe["index"].cpu().numpy(), g[p + "eval/index"])
    if not attn:
        check("eval/logits", oe["logits"])
    assert float((oe["logits"].max(2)[1].cpu().numpy() == g[p + "eval/argmax"]).mean()) >= 0.99


# ---- 3. loop A: an expert's parameter gradients at imgH = 64 -------------------------------------------------------------
def test_loop_a_crnn_gradients_vs_oracle_64():
    from mrn_amd import functional as Fn
    from oracle import mrn_oracle as O
    opt, net, sd = build_mrn("crnn", 64, (40,), 11)
    image, labels, lens = inputs("crnn", 64, 3, (40,), 11)
    names = [n for n, p in net.named_parameters() if n.startswith("model.0.")]
    params = [sd[n].requires_grad_(True) for n in names]
    cfg = O.Cfg(*CFG["crnn"], imgH=64)
    ref_out = O.model_forward(sd, "model.0.", cfg, image, None, True, training=True)["predict"]
    ref_loss = O.ctc_loss(ref_out, labels, lens)
    ref_grads = torch.autograd.grad(ref_loss, params)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = n.startswith("model.0.")
    preds = net.model[0](image.cuda(), None, True)["predict"]
    loss = Fn.ctc_loss(preds, labels.cuda(), lens.cuda())
    assert_close("loop A logits", preds, ref_out, atol=1e-4)
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * max(1.0, abs(ref_loss.item()))
    loss.backward()
    mine = dict(net.named_parameters())
    for n, rg in zip(names, ref_grads):
        if rg.abs().max() < 1e-9:
            continue
        _grad_check(n, mine[n].grad, rg)


def _oracle_trba_grads(sd0, image, labels_index, dtype):
    from oracle import mrn_oracle as O
    sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    names = [k for k in sd if k.startswith("model.0.") and sd[k].is_floating_point() and "running" not in k
             and "generator" not in k]
    params = [sd[n].requires_grad_(True) for n in names]
    for k in list(sd):               # Prediction.generator.* aliases fc.*
        if k.startswith("model.0.Prediction.generator."):
            sd[k] = sd[k.replace("Prediction.generator.", "fc.")]
    cfg = O.Cfg(*CFG["trba"], imgH=64)
    old = O.tps_constants
    O.tps_constants = lambda *a: tuple(t.to(dtype) for t in old(*a))
    try:
        torch.set_default_dtype(dtype)
        out = O.model_forward(sd, "model.0.", cfg, image.to(dtype), labels_index[:, :-1], True, training=True)["predict"]
        loss = O.attn_ce_loss(out, labels_index)
        grads = torch.autograd.grad(loss, params, allow_unused=True)
    finally:
        torch.set_default_dtype(torch.float32)
        O.tps_constants = old
    return names, grads, out.detach(), loss.detach()


def test_loop_a_trba_gradients_vs_oracle_64():
    """as test_model_gpu.py::test_loop_a_trba_gradients_vs_oracle (B = 3): judged against the float64 oracle, at least as close
    to it as 3x the reference's own fp32 arithmetic, floor 2e-3"""
    from mrn_amd import functional as Fn
    opt, net, sd = build_mrn("trba", 64, (41,), 12)
    image, text, _ = inputs("trba", 64, 3, (41,), 12)
    names, g32, out32, loss32 = _oracle_trba_grads(sd, image, text, torch.float32)
    _, g64, _, _ = _oracle_trba_grads(sd, image, text, torch.float64)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = n.startswith("model.0.")
    preds = net.model[0](image.cuda(), text[:, :-1].cuda(), True)["predict"]
    loss = Fn.cross_entropy(preds, text[:, 1:].cuda(), 1)
    assert_close("loop A logits", preds, out32, atol=1e-4)
    assert abs(loss.item() - loss32.item()) < 1e-4 * max(1.0, abs(loss32.item()))
    loss.backward()
    mine = dict(net.named_parameters())

    def rel(a, b):
        return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)

    for n, a32, a64 in zip(names, g32, g64):
        if a64 is None or a64.abs().max() < 1e-12:
            continue
        e_ref = rel(a32.double().numpy(), a64.numpy())
        e_hip = rel(mine[n].grad.detach().cpu().double().numpy(), a64.numpy())
        assert e_hip <= max(3.0 * e_ref, 2e-3), f"{n}: HIP vs f64 {e_hip:.2e}, torch-f32 vs f64 {e_ref:.2e}"


# ---- 4. loop B: two router steps at imgH = 48 ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["crnn", "trba"])
def test_loop_b_two_steps_vs_oracle_48(kind):
    from mrn_amd import functional as Fn
    from mrn_amd.optim import FlatAdam
    from oracle import mrn_oracle as O
    classes = CLASSES[kind]
    I, B = len(classes), 8
    opt, net, sd = build_mrn(kind, 48, classes, 13)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.")
    tr_names = [n for n, p in net.named_parameters() if p.requires_grad]
    adam = FlatAdam([p for n, p in net.named_parameters() if p.requires_grad], lr=5e-4)
    cfg = O.Cfg(*CFG[kind], imgH=48)
    attn = kind == "trba"
    sd_ref = {k: v.clone() for k, v in sd.items()}
    state = [{"m": torch.zeros_like(sd_ref[n]), "v": torch.zeros_like(sd_ref[n])} for n in tr_names]
    for step in (1, 2):
        image, tgt, lens = inputs(kind, 48, B, classes, 100 + step)
        domain = torch.from_numpy(np.arange(B) % I)
        text_in = tgt[:, :-1] if attn else None
        params = [sd_ref[n].requires_grad_(True) for n in tr_names]
        o = O.mrn_forward(sd_ref, cfg, I, image, True, text_in, True, training=True)
        clf = O.attn_ce_loss(o["logits"], tgt) if attn else O.ctc_loss(o["logits"], tgt, lens)
        ref_loss = 15 * clf + F.cross_entropy(o["index"], domain)
        ref_grads = torch.autograd.grad(ref_loss, params)
        for p in params:
            p.requires_grad_(False)
        before = {n: sd_ref[n].clone() for n in tr_names}
        with torch.no_grad():
            O.clip_and_adam(params, ref_grads, state, 5e-4, step)
        adam.zero_grad()                                    # (the parameters' .grad are views of the optimiser's flat buffer)
        out = net(image.cuda(), True, None if text_in is None else text_in.cuda(), True)
        if attn:
            c = Fn.cross_entropy(out["logits"], tgt[:, 1:].cuda(), 1)
        else:
            c = Fn.ctc_loss(out["logits"], tgt.cuda(), lens.cuda())
        loss = 15 * c + Fn.cross_entropy(out["index"], domain.cuda(), -100)
        assert abs(loss.item() - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item())) * (3 if attn else 1), (loss.item(), ref_loss.item())
        loss.backward()
        mine = dict(net.named_parameters())
        for n, gr in zip(tr_names, ref_grads):
            if n == "route.bias":
                continue
            _grad_check(f"step {step} {n}", mine[n].grad, gr, rel_l2=2e-3 if not attn else 5e-3, rel_max=1e-2 if not attn else 2.5e-2)
        mine_before = {n: mine[n].detach().cpu().clone() for n in tr_names}
        adam.step(lr=5e-4, max_norm=5.0)
        for n, gr in zip(tr_names, ref_grads):
            if n == "route.bias":
                continue          # (a round-off gradient's Adam step has a random sign)
            d_ref = sd_ref[n] - before[n]
            d_mine = mine[n].detach().cpu() - mine_before[n]
            rel = float((d_mine - d_ref).norm() / d_ref.norm().clamp_min(1e-30))
            assert rel <= 5e-2, (step, n, rel)


# ---- 5. DER: one step at imgH = 48 ------------------------------------------------------------------------------------------
def test_dernet_step_vs_oracle_48():
    from mrn_amd import functional as Fn
    from mrn_amd.modules.model import DERNet
    from mrn_amd.tools import weights as W
    from oracle import mrn_oracle as O
    opt = make_opt("crnn", 48)
    classes = (40, 70)
    B = 8
    with contextlib.redirect_stdout(io.StringIO()):
        net = DERNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
            net.build_aux_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed=17)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().train()
    net.model[0].eval()                                         # DER's model_eval_and_train: the old extractor in eval mode, frozen
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.0.")
    image, labels, lens = inputs("crnn", 48, B, classes, 17)
    cfg = O.Cfg(*CFG["crnn"], imgH=48)
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    params = [sd[n].requires_grad_(True) for n in names]
    ref = O.dernet_forward(sd, cfg, len(classes), image, None, True, training=True)
    ref_loss = O.ctc_loss(ref["logits"], labels, lens)
    ref_grads = torch.autograd.grad(ref_loss, params, allow_unused=True)      # (the attention heads are unused by CTC)
    out = net(image.cuda())
    assert_close("DER features", out["features"], ref["features"], atol=1e-4)
    assert_close("DER logits", out["logits"], ref["logits"], atol=1e-4)
    assert_close("DER aux logits", out["aux_logits"], ref["aux_logits"], atol=1e-4)
    loss = Fn.ctc_loss(out["logits"], labels.cuda(), lens.cuda())
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * max(1.0, abs(ref_loss.item()))
    loss.backward()
    mine = dict(net.named_parameters())
    for n, rg in zip(names, ref_grads):
        if rg is None or rg.abs().max() < 1e-9:
            continue
        _grad_check(n, mine[n].grad, rg, rel_l2=2e-3, rel_max=1e-2)


# ---- 6. reduced mode at imgH = 48 (6-row maps: no plain-fp16 Winograd form there) -----------------------------------------
@pytest.mark.parametrize("kind", ["crnn", "trba"])
def test_reduced_mode_loop_b_48(kind):
    from mrn_amd import ops
    classes = CLASSES[kind]
    B = 8
    opt, net, sd = build_mrn(kind, 48, classes, 19)
    net.train()
    image, tgt, _ = inputs(kind, 48, B, classes, 19)
    text_in = tgt[:, :-1].cuda() if kind == "trba" else None
    with torch.no_grad():
        ref = net(image.cuda(), True, text_in, True)
    saved = ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS
    try:
        ops.X3_PRODUCTS = ops.TRAIN_PRODUCTS = 1            # bench.py --precision fp16
        net.load_state_dict(sd, strict=True)                # (the same running statistics before the step)
        with torch.no_grad():
            out = net(image.cuda(), True, text_in, True)
        torch.cuda.synchronize()
    finally:
        ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS = saved
    w, w0 = out["index"].cpu(), ref["index"].cpu()
    lg, lg0 = out["logits"].cpu(), ref["logits"].cpu()
    err_w = float((w - w0).abs().max())
    err_l = float((lg - lg0).abs().max()) / max(float(lg0.abs().max()), 1e-6)
    assert torch.isfinite(lg).all()
    assert err_w <= 2e-2 and err_l <= 5e-2, (err_w, err_l)
    assert err_w > 1e-7 or err_l > 1e-7                     # the reduced arithmetic really ran


# ---- 7. the largest supported size -------------------------------------------------------------------------------------------
def test_full_size_trba6_loop_b_64():
    from mrn_amd import functional as Fn
    from mrn_amd.modules.expert_group import BackboneGroup
    from mrn_amd.tools import weights as W
    classes = (41, 51, 61, 71, 81, 98)
    B = 256
    opt, net, sd = build_mrn("trba", 64, classes, 23)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.")
    image = torch.from_numpy(W.uniform("geom_full", (B, 4, 64, 256), -1.0, 1.0, 23)).cuda()
    text = torch.from_numpy(W.randint("geom_full_text", (B, 27), 4, classes[-1], 23)).cuda()
    text[:, 0] = 2
    domain = torch.arange(B, device="cuda") % len(classes)
    out = net(image, True, text[:, :-1], True)
    loss = 15 * Fn.cross_entropy(out["logits"], text[:, 1:], 1) + Fn.cross_entropy(out["index"], domain, -100)
    loss.backward()
    assert torch.isfinite(loss).item()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
    net.eval()
    grp = BackboneGroup([m.model for m in net.model])
    with torch.no_grad():
        full = grp.visual_all(image)                        # [6, 256, 65, 512]
        part = grp.visual_all(image[:8].contiguous())
    assert full.shape == (6, B, 65, 512)
    assert_close("first 8 rows of B = 256 vs B = 8", full[:, :8], part, atol=1e-4)
    assert torch.isfinite(full).all()


# ---- 8. heights outside the supported set -------------------------------------------------------------------------------------
def test_unsupported_height_is_refused():
    from mrn_amd.modules.model import Model
    opt = make_opt("trba", 96)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Model(opt)
        net.update_fc(opt.hidden_size, 41)
        net.build_prediction(opt, 41)
    net = net.cuda().eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"imgH in \{32, 48, 64\} at imgW = 256"):
        net.model.visual(torch.zeros(2, 4, 96, 256, device="cuda"))
    _, mrn, _ = build_mrn("trba", 96, (41, 51), 3)
    mrn.eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"imgH in \{32, 48, 64\} at imgW = 256"):
        mrn(torch.zeros(2, 4, 96, 256, device="cuda"), True, torch.LongTensor(2).fill_(2).cuda(), False)


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------
def test_tiny_train_one_task_at_64(tmp_path):
    from torch.utils.data import ConcatDataset
    from mrn_amd import tiny_train
    from mrn_amd.data.data_manage import Dataset_Manager, Val_Dataset
    from mrn_amd.data.dataset import ArrayDataset
    from tests.helpers import fake_text_samples
    os.chdir(tmp_path)
    opt = types.SimpleNamespace(
        exp_name="t", il="mrn", memory="random", memory_num=20, batch_max_length=25, imgH=64, imgW=256, manual_seed=111,
        start_task=0, num_fiducial=20, input_channel=4, output_channel=512, hidden_size=256, schedule="super",
        optimizer="adam", lr=0.0005, batch_size=6, num_iter=4, val_interval=2, grad_clip=5, lan_list=["A"], NED=True,
        workers=0, select_data=["rootA"], valid_datas=["valA"], Aug="None")
    opt.Transformation, opt.FeatureExtraction, opt.SequenceModeling, opt.Prediction = CFG["crnn"]

    def open_fake(path, o, mode="train"):
        images, labels = fake_text_samples(path)
        return ArrayDataset(images, labels, o, mode)

    np.random.seed(3)
    torch.manual_seed(3)
    dm = Dataset_Manager(opt, open_dataset=open_fake)
    valid = Val_Dataset(["valA/A"], opt, open_tree=lambda root, o, mode: (ConcatDataset([open_fake(root, o, mode)]), "log"))
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        learner, best, ned = tiny_train.train(opt, io.StringIO(), data=(dm, valid, lambda t: "abcdefghijklmnopqrstuvwxyz",
                                                                         lambda t: [valid.create_dataset("valA/A")]))
    assert len(best) == 1 and len(ned) == 1
    assert 0.0 <= float(best[0]) <= 100.0
    assert "Incremental Accuracy" in sink.getvalue()
    assert all(torch.isfinite(p).all() for p in learner.model.parameters())


def test_checkpoint_round_trip_at_64(tmp_path):
    opt, net, sd = build_mrn("crnn", 64, CLASSES["crnn"], 29)
    image, _, _ = inputs("crnn", 64, 4, CLASSES["crnn"], 29)
    net.eval()
    with torch.no_grad():
        a = net(image.cuda(), True, None, False)["logits"].cpu()
    path = os.path.join(str(tmp_path), "geom64.pth")
    torch.save(net.state_dict(), path)
    _, net2, _ = build_mrn("crnn", 64, CLASSES["crnn"], 30)
    net2.load_state_dict(torch.load(path), strict=True)
    net2.eval()
    with torch.no_grad():
        b = net2(image.cuda(), True, None, False)["logits"].cpu()
    assert torch.equal(a, b)
