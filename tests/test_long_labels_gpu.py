"""Labels longer than 31 characters on the GPU: the long CTC kernel (mrn_ctc_loss_fwd_long_f32 / bwd) against torch's CTC loss
and against the 64-state kernel, the unchanged short path, the CRNN / SVTR stacks against the CPU oracle at batch_max_length
48 / 63 / 40, the attention decoder backward beyond the deferred sums' old LDS staging (S >= 127 steps), validation and the
training driver at 48, and the refusal beyond 255."""
import contextlib
import io
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import assert_close, drop_masks
from tests.test_geometry_gpu import _grad_check
from tests.test_model_gpu import set_drop_masks_from

pytestmark = pytest.mark.gpu

CFG = {"crnn": ("None", "VGG", "BiLSTM", "CTC"), "svtr": ("None", "SVTR", "None", "CTC"), "trba": ("TPS", "ResNet", "BiLSTM", "Attn")}
CLASSES = {"crnn": (40, 70, 97), "svtr": (40, 70, 97), "trba": (41, 71, 98)}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _p(t):
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def ctc_targets(lengths, W, C, seed, repeat_rows=()):
    """padded [B, W] int64 targets (classes 2..C-1, pad 1) and int32 lengths; rows in repeat_rows are one class repeated"""
    B = len(lengths)
    g = torch.Generator().manual_seed(seed)
    tg = torch.randint(2, C, (B, W), generator=g)
    tl = torch.tensor(lengths, dtype=torch.int32)
    for b in repeat_rows:
        tg[b, :] = 7
    for b in range(B):
        L = int(tl[b])
        if b not in repeat_rows and L >= 6:
            tg[b, 1:4] = tg[b, 0]                # a run of repeated labels: needs blanks between them
        tg[b, L:] = 1
    return tg, tl


def torch_ctc(logits, targets, tl, upstream=15.0):
    """F.ctc_loss on the CPU in float64 (mean, zero_infinity) -> (loss, d loss*upstream / d logits) as float64"""
    B, T, C = logits.shape
    x = logits.double().clone().requires_grad_(True)
    lp = x.log_softmax(2).permute(1, 0, 2)
    ref = F.ctc_loss(lp, targets, torch.full((B,), T, dtype=torch.int32), tl, blank=0, reduction="mean", zero_infinity=True)
    (upstream * ref).backward()
    return ref.detach(), x.grad


def direct_ctc(logits, targets, tl, long_kernel, upstream=15.0):
    """one direct call of the fwd / bwd entry points (long or 64-state), max_target_len = the padded width"""
    from mrn_amd import ops
    from mrn_amd._lib import call
    B, T, C = logits.shape
    W = targets.shape[1]
    d = ops.padded_rows(B, T, C, "cuda")
    d.copy_(logits)
    tg, tlc = targets.cuda().contiguous(), tl.cuda().to(torch.int32).contiguous()
    lse = torch.empty(B * T, device="cuda")
    nll = torch.empty(B, device="cuda")
    loss = torch.empty(1, device="cuda")
    up = torch.tensor([upstream], device="cuda")
    dl = torch.empty_strided(d.shape, d.stride(), device="cuda")
    if long_kernel:
        occ = torch.empty(call("mrn_ctc_occ_floats_long", B, T, W), device="cuda")
        call("mrn_ctc_loss_fwd_long_f32", _p(d), d.stride(1), _p(tg), W, _p(tlc), W, _p(lse), _p(nll), _p(occ), _p(loss), B, T, C, 0,
             _stream())
        call("mrn_ctc_loss_bwd_long_f32", _p(d), d.stride(1), _p(lse), _p(occ), _p(tg), W, _p(tlc), W, _p(nll), _p(up), _p(dl),
             dl.stride(1), B, T, C, 0, _stream())
    else:
        occ = torch.empty(call("mrn_ctc_occ_floats", B, T), device="cuda")
        call("mrn_ctc_loss_fwd_f32", _p(d), d.stride(1), _p(tg), W, _p(tlc), W, _p(lse), _p(nll), _p(occ), _p(loss), B, T, C, 0,
             _stream())
        call("mrn_ctc_loss_bwd_f32", _p(d), d.stride(1), _p(lse), _p(occ), _p(tg), W, _p(tlc), _p(nll), _p(up), _p(dl), dl.stride(1),
             B, T, C, 0, _stream())
    torch.cuda.synchronize()
    return loss.cpu(), nll.cpu(), dl.cpu()


# ---- 1. the long kernel against torch ------------------------------------------------------------------------------------------
# (T, W, lengths, repeat rows): every K (W 40 -> 2, 64 / 100 -> 4, 255 -> 8), empty targets, runs of repeats, and infeasible rows
# (L > T; a repeated class needing 2L - 1 > T frames) whose loss and gradient are 0
LONG_CASES = [
    (63, 40, [32, 40, 0, 5, 31, 33, 17, 40, 1, 36], (7,)),
    (64, 64, [64, 63, 32, 0, 40, 50, 2, 64, 33], (8,)),
    (65, 100, [100, 64, 63, 40, 32, 0, 65, 99, 12], (3,)),
    (64, 255, [255, 100, 64, 63, 40, 32, 0, 30, 60], (4,)),
    (300, 255, [255, 200, 100, 64, 63, 32, 0, 150, 140], (7,)),
]


@pytest.mark.parametrize("T,W,lengths,repeat_rows", LONG_CASES)
def test_long_ctc_vs_torch(T, W, lengths, repeat_rows):
    from mrn_amd import ops
    C = 97
    logits = rnd(len(lengths), T, C, seed=T + W, scale=3.0)
    tg, tl = ctc_targets(lengths, W, C, seed=W, repeat_rows=repeat_rows)
    ref, gref = torch_ctc(logits, tg, tl)
    d = ops.padded_rows(len(lengths), T, C, "cuda")
    d.copy_(logits)
    loss, ctx = ops.ctc_loss_fwd(d, tg.cuda(), tl.cuda())
    dl = ops.ctc_loss_bwd(ctx, torch.tensor([15.0], device="cuda"))
    assert_close("long ctc loss", loss, ref.view(1), atol=1e-5, rtol=1e-5)
    assert_close("long ctc grad", dl, gref, atol=2e-6, rtol=1e-4)
    nll = ctx[4].cpu()
    for b, L in enumerate(lengths):
        frames = L + int((tg[b, 1:L] == tg[b, :L - 1]).sum()) if L > 1 else L     # a repeat needs a blank between
        if frames > T:
            assert torch.isinf(nll[b]), (b, L)
            assert float(dl[b].abs().max()) == 0.0, (b, L)
        else:
            assert torch.isfinite(nll[b]), (b, L)


@pytest.mark.parametrize("T", [63, 64])
def test_long_ctc_vs_torch_full_batch(T, W=63):
    """B = 256 and C ~ 5000 (the bench's summed class counts), lengths 0..63 at W = 63"""
    from mrn_amd import ops
    B, C = 256, 4998
    g = torch.Generator().manual_seed(T)
    lengths = torch.randint(0, W + 1, (B,), generator=g).tolist()
    lengths[:4] = [0, W, 32, 1]
    logits = rnd(B, T, C, seed=3 * T, scale=3.0)
    tg, tl = ctc_targets(lengths, W, C, seed=T, repeat_rows=(5,))
    ref, gref = torch_ctc(logits, tg, tl)
    d = ops.padded_rows(B, T, C, "cuda")
    d.copy_(logits)
    loss, ctx = ops.ctc_loss_fwd(d, tg.cuda(), tl.cuda())
    dl = ops.ctc_loss_bwd(ctx, torch.tensor([15.0], device="cuda"))
    assert_close("long ctc loss B=256", loss, ref.view(1), atol=1e-5, rtol=1e-5)
    assert_close("long ctc grad B=256", dl, gref, atol=2e-6, rtol=1e-4)


# ---- 2. the long kernel against the 64-state kernel at L <= 31 ----------------------------------------------------------------
@pytest.mark.parametrize("T,W", [(63, 25), (64, 31), (26, 25)])
def test_long_kernel_matches_short_kernel(T, W):
    B, C = 24, 97
    lengths = [(7 * b) % (W + 1) for b in range(B)]
    lengths[:3] = [0, W, 1]
    logits = rnd(B, T, C, seed=T * W, scale=2.0)
    tg, tl = ctc_targets(lengths, W, C, seed=W + T, repeat_rows=(3,))
    l_short, nll_short, g_short = direct_ctc(logits, tg, tl, long_kernel=False)
    l_long, nll_long, g_long = direct_ctc(logits, tg, tl, long_kernel=True)
    fin = torch.isfinite(nll_short)
    assert torch.equal(fin, torch.isfinite(nll_long))
    assert_close("nll long vs short", nll_long[fin], nll_short[fin], atol=0, rtol=1e-6)
    assert_close("loss long vs short", l_long, l_short, atol=0, rtol=1e-6)
    # gradients: the 64-state kernel's unscaled fp32 log alpha (~ -300 at T = 63, ulp 3e-5) puts its own gradient ~1e-4 (relative)
    # from float64, so the two kernels are compared through torch: the long kernel is at least as close, and within the
    # 64-state kernel's own error of it
    _, gref = torch_ctc(logits, tg, tl)
    e_short = float((g_short.double() - gref).abs().max())
    e_long = float((g_long.double() - gref).abs().max())
    assert e_long <= e_short + 1e-7, (e_long, e_short)
    assert_close("grad long vs torch", g_long, gref, atol=2e-6, rtol=1e-4)
    assert float((g_long - g_short).abs().max()) <= 2 * e_short + 2e-6


# ---- 3. the short path is unchanged --------------------------------------------------------------------------------------------
def test_short_path_bit_identical_to_direct_call():
    from mrn_amd import ops
    B, T, C, W = 16, 63, 97, 25
    logits = rnd(B, T, C, seed=5, scale=3.0)
    tg, tl = ctc_targets([(5 * b) % 26 for b in range(B)], W, C, seed=9)
    d = ops.padded_rows(B, T, C, "cuda")
    d.copy_(logits)
    loss, ctx = ops.ctc_loss_fwd(d, tg.cuda(), tl.cuda())
    assert ctx[5].numel() == B * T * 64                                    # the 64-state layout
    l_direct, nll_direct, _ = direct_ctc(logits, tg, tl, long_kernel=False)
    assert torch.equal(loss.cpu(), l_direct)
    assert torch.equal(ctx[4].cpu(), nll_direct)


# ---- 4. model level against the oracle -----------------------------------------------------------------------------------------
def make_opt(kind, bml):
    o = types.SimpleNamespace(num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=bml)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = CFG[kind]
    return o


def build_mrn(kind, bml, classes, seed):
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as W
    opt = make_opt(kind, bml)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed=seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return opt, net.cuda(), sd


def long_inputs(kind, bml, B, classes, seed, frames=63):
    """images and CTC targets padded to bml, lengths up to min(bml, frames // 2) so that most rows are feasible, plus one at bml"""
    from mrn_amd.tools import weights as W
    image = torch.from_numpy(W.smooth_image(f"long_{kind}_{bml}", (B, 4, 32, 256), seed))
    if kind == "trba":
        text = torch.from_numpy(W.randint(f"long_text_{bml}", (B, bml + 2), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None
    hi = min(bml, frames // 2)
    lens = torch.from_numpy(W.randint(f"long_len_{bml}", (B,), 1, hi + 1, seed)).int()
    lens[0] = bml
    lens[-1] = max(1, min(bml, 40))
    labels = torch.from_numpy(W.randint(f"long_ctc_{bml}", (B, bml), 4, classes[-1], seed))
    labels[torch.arange(bml)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


@pytest.mark.parametrize("bml", [48, 63])
def test_loop_a_crnn_gradients_vs_oracle(bml):
    from mrn_amd import functional as Fn
    from oracle import mrn_oracle as O
    opt, net, sd = build_mrn("crnn", bml, (40,), 11)
    image, labels, lens = long_inputs("crnn", bml, 4, (40,), 11)
    names = [n for n, p in net.named_parameters() if n.startswith("model.0.")]
    params = [sd[n].requires_grad_(True) for n in names]
    cfg = O.Cfg(*CFG["crnn"])
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


def _loop_b_steps(kind, bml, steps, B=8, rel_l2=2e-3, rel_max=1e-2):
    from mrn_amd import functional as Fn
    from mrn_amd.optim import FlatAdam
    from oracle import mrn_oracle as O
    classes = CLASSES[kind]
    I = len(classes)
    opt, net, sd = build_mrn(kind, bml, classes, 13)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.")
    tr_names = [n for n, p in net.named_parameters() if p.requires_grad]
    adam = FlatAdam([p for n, p in net.named_parameters() if p.requires_grad], lr=5e-4)
    cfg = O.Cfg(*CFG[kind])
    sd_ref = {k: v.clone() for k, v in sd.items()}
    state = [{"m": torch.zeros_like(sd_ref[n]), "v": torch.zeros_like(sd_ref[n])} for n in tr_names]
    for step in range(1, steps + 1):
        image, tgt, lens = long_inputs(kind, bml, B, classes, 100 + step)
        domain = torch.from_numpy(np.arange(B) % I)
        params = [sd_ref[n].requires_grad_(True) for n in tr_names]
        masks = drop_masks(B, 13, f"long{bml}:{step}", I) if kind == "svtr" else None
        o = O.mrn_forward(sd_ref, cfg, I, image, True, None, True, training=True,
                          masks=[[m.clone() for m in ms] for ms in masks] if masks else None)
        ref_loss = 15 * O.ctc_loss(o["logits"], tgt, lens) + F.cross_entropy(o["index"], domain)
        ref_grads = torch.autograd.grad(ref_loss, params)
        for p in params:
            p.requires_grad_(False)
        before = {n: sd_ref[n].clone() for n in tr_names}
        with torch.no_grad():
            O.clip_and_adam(params, ref_grads, state, 5e-4, step)
        adam.zero_grad()
        set_drop_masks_from(net, masks)
        out = net(image.cuda(), True, None, True)
        loss = 15 * Fn.ctc_loss(out["logits"], tgt.cuda(), lens.cuda()) + Fn.cross_entropy(out["index"], domain.cuda(), -100)
        assert abs(loss.item() - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item())), (loss.item(), ref_loss.item())
        loss.backward()
        mine = dict(net.named_parameters())
        for n, gr in zip(tr_names, ref_grads):
            if n == "route.bias":
                continue
            _grad_check(f"step {step} {n}", mine[n].grad, gr, rel_l2=rel_l2, rel_max=rel_max)
        mine_before = {n: mine[n].detach().cpu().clone() for n in tr_names}
        adam.step(lr=5e-4, max_norm=5.0)
        for n, gr in zip(tr_names, ref_grads):
            if n == "route.bias":
                continue
            d_ref = sd_ref[n] - before[n]
            d_mine = mine[n].detach().cpu() - mine_before[n]
            rel = float((d_mine - d_ref).norm() / d_ref.norm().clamp_min(1e-30))
            assert rel <= 5e-2, (step, n, rel)


def test_loop_b_crnn3_two_steps_vs_oracle_40():
    _loop_b_steps("crnn", 40, 2)


def test_loop_b_svtr3_vs_oracle_48():
    _loop_b_steps("svtr", 48, 1)


# ---- 5. the attention backward beyond the deferred sums' old LDS staging ------------------------------------------------------
@pytest.mark.parametrize("B,D,S", [(5, 256, 126), (3, 1536, 128), (4, 256, 200)])
def test_attention_decoder_backward_long(B, D, S, T=65):
    """as test_kernels_gpu.py::test_attention_decoder_backward at T = 65: S * (T + 256) floats exceed 160 KB from S = 128 on,
    so dHb / dHproj are summed over chunks of the steps (S = 126: one launch, as before)"""
    from oracle import mrn_oracle as O
    from mrn_amd.modules.prediction import Attention
    import torch.nn as nn
    Hd, C = 256, 97
    att = Attention(D, Hd, C, nn.Linear(Hd, C))
    sd = {k: rnd(*v.shape, seed=140 + i, scale=0.08) for i, (k, v) in enumerate(att.state_dict().items())}
    sd["char_embeddings.weight"] = rnd(C, 256, seed=177)
    att.load_state_dict(sd)
    Hb = rnd(B, T, D, seed=141)
    text = torch.randint(0, C + 3, (B, S), generator=torch.Generator().manual_seed(6))
    text[:, 0] = 2
    up = rnd(B, S, C, seed=142)
    osd = {"P." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    Hr = Hb.clone().requires_grad_(True)
    ref = O.attention_forward(osd, "P.", Hr, text, True, S - 1, osd["P.generator.weight"], osd["P.generator.bias"])
    (ref * up).sum().backward()
    att = att.cuda()
    Hc = Hb.cuda().requires_grad_(True)
    out = att(Hc, text.cuda(), True, S - 1)
    (out * up.cuda()).sum().backward()
    assert_close("decoder logits", out, ref, atol=1e-4)
    scale = Hr.grad.abs().max().item()
    assert_close("decoder dH", Hc.grad, Hr.grad, atol=2e-4 * max(scale, 1.0))
    for k, prm in att.named_parameters():
        g_ref = osd["P." + k].grad
        if g_ref is None:
            continue
        tol = 2e-4 * max(g_ref.abs().max().item(), 1.0)
        assert_close("decoder d" + k, prm.grad, g_ref, atol=tol)


def _oracle_trba_grads(sd0, image, labels_index, dtype):
    """test_geometry_gpu.py's TRBA loop-A oracle at imgH = 32: autograd through the reference's arithmetic in `dtype`"""
    from oracle import mrn_oracle as O
    sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    names = [k for k in sd if k.startswith("model.0.") and sd[k].is_floating_point() and "running" not in k
             and "generator" not in k]
    params = [sd[n].requires_grad_(True) for n in names]
    for k in list(sd):               # Prediction.generator.* aliases fc.*
        if k.startswith("model.0.Prediction.generator."):
            sd[k] = sd[k.replace("Prediction.generator.", "fc.")]
    cfg = O.Cfg(*CFG["trba"], batch_max_length=labels_index.shape[1] - 2)
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


def test_loop_a_trba_gradients_vs_oracle_150():
    """TRBA at batch_max_length 150 (151 decoder steps): judged against the float64 oracle as test_geometry_gpu.py's TRBA loop A"""
    from mrn_amd import functional as Fn
    bml = 150
    opt, net, sd = build_mrn("trba", bml, (41,), 12)
    image, text, _ = long_inputs("trba", bml, 2, (41,), 12)
    names, g32, out32, loss32 = _oracle_trba_grads(sd, image, text, torch.float32)
    _, g64, _, _ = _oracle_trba_grads(sd, image, text, torch.float64)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = n.startswith("model.0.")
    preds = net.model[0](image.cuda(), text[:, :-1].cuda(), True)["predict"]
    assert preds.shape[1] == bml + 1
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


# ---- 6. evaluation and the driver ----------------------------------------------------------------------------------------------
def test_validation_ctc_at_48():
    from mrn_amd import functional as Fn
    from mrn_amd.il_modules.base import Criterion
    from mrn_amd.modules.model import Model
    from mrn_amd.test import validation
    from mrn_amd.tools import weights as W
    from mrn_amd.tools.utils import CTCLabelConverter
    from tests.helpers import DetLoader
    opt = make_opt("crnn", 48)
    opt.NED = True
    chars = "".join(chr(0x4E00 + i) for i in range(36))
    with contextlib.redirect_stdout(io.StringIO()):
        net = Model(opt)
        net.update_fc(opt.hidden_size, 40)
        net.build_prediction(opt, 40)
        conv = CTCLabelConverter(chars)
    W.fill_state_dict(net.state_dict(), 51)
    net = net.cuda().eval()
    loader = DetLoader(3, "long_validation", 51, oov=True, n_valid=2)
    loader.set_characters(chars)
    batches = list(loader.create_dataset())
    with torch.no_grad():
        res = validation(net, Criterion("CTC", None), batches, conv, opt)
        ref = []
        for image, labels in batches:
            li, ll = conv.encode(labels, batch_max_length=48)
            assert li.shape[1] == 48
            preds = net(image.cuda(), is_train=False)["predict"]
            ref.append(float(Fn.ctc_loss(preds.contiguous(), li, ll)))
    assert abs(res[0] - sum(ref) / len(ref)) <= 1e-6 * max(1.0, abs(res[0]))
    assert np.isfinite(res[0]) and 0.0 <= res[1] <= 100.0


def test_tiny_train_one_crnn_task_at_48(tmp_path):
    from torch.utils.data import ConcatDataset
    from mrn_amd import tiny_train
    from mrn_amd.data.data_manage import Dataset_Manager, Val_Dataset
    from mrn_amd.data.dataset import ArrayDataset
    from tests.helpers import fake_text_samples
    os.chdir(tmp_path)
    opt = types.SimpleNamespace(
        exp_name="t", il="mrn", memory="random", memory_num=20, batch_max_length=48, imgH=32, imgW=256, manual_seed=111,
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


# ---- 7. refusal ---------------------------------------------------------------------------------------------------------------
def test_ctc_loss_refused_at_256_launches_nothing(monkeypatch):
    from mrn_amd import functional as Fn
    from mrn_amd import ops
    B, T, C = 2, 63, 40
    logits = torch.randn(B, T, C, device="cuda", requires_grad=True)
    targets = torch.ones(B, 256, dtype=torch.long, device="cuda")
    lens = torch.tensor([3, 256], dtype=torch.int32, device="cuda")
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda *a: calls.append(a[0]) or real(*a))
    with pytest.raises(NotImplementedError, match=r"in 0\.\.255; got 256"):
        Fn.ctc_loss(logits, targets, lens)
    assert calls == []
    # greedy CTC evaluation without a loss still runs at any batch_max_length
    opt, net, _ = build_mrn("crnn", 256, (40,), 3)
    net.eval()
    with torch.no_grad():
        out = net(torch.zeros(2, 4, 32, 256, device="cuda"), True, None, False)
    assert torch.isfinite(out["logits"]).all()
