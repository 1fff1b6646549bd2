"""Hidden sizes 128 and 512 on the GPU: the LSTM layer kernels' new instantiations (8 waves at 128; 16 waves of two unit tiles each at
512) against torch and float64 on the host, the grouped forms against single launches, the order of the two unit passes at 512, the
CRNN / SVTR MRN stacks and a CRNN DERNet against the reference fixture (tests/golden/hidden.npz) and the CPU oracle, one LwF run and
one training-driver task at 128, reduced mode at 512, the refusals (attention head, sizes outside the set), and the dispatch at 256.
Bands are those of tests/test_width_gpu.py / tests/test_kernels_gpu.py for the same quantities."""
import contextlib
import io
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import assert_close, load_golden, sub
from tests.test_geometry_gpu import _grad_check
from tests.test_hidden_cpu import CLASSES, HIDDEN_CASES, STAGES, hidden_masks, hidden_state_dict, hidden_targets
from tests.test_kernels_gpu import cu, ops, rnd  # noqa: F401  (ops: the module-scoped fixture that loads the library)
from tests.test_width_gpu import recorded_calls

pytestmark = pytest.mark.gpu

HIDDEN_SET = r"\[128, 256, 512\]"


def make_opt(kind, hidden, imgW, bml=25):
    o = types.SimpleNamespace(num_fiducial=20, imgH=32, imgW=imgW, input_channel=4, output_channel=512, hidden_size=hidden,
                              batch_max_length=bml)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = (
        STAGES[kind] if kind in STAGES else ("TPS", "ResNet", "BiLSTM", "Attn"))
    return o


def build_mrn(kind, hidden, imgW, classes):
    from mrn_amd.modules.model import MRNNet
    opt = make_opt(kind, hidden, imgW)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
    return opt, net


# ---- float64 on the host: one LSTM layer, both directions, with the saves and the gate gradients ---------------------------------
def lstm_ref64(xproj, ws, b_hh, dout=None):
    """xproj [B,T,ndir*4H], ws: ndir x [4H,H], b_hh [ndir*4H] -> out [B,T,ndir*H], gates [B,T,ndir,4H] (post-activation i,f,g,o),
    cseq [B,T,ndir,H] and, with dout, dgates [B,T,ndir,4H] (gradient of the pre-activations), all float64"""
    B, T, _ = xproj.shape
    ndir, H = len(ws), ws[0].shape[1]
    x = xproj.detach().cpu().double().view(B, T, ndir, 4 * H)
    b = b_hh.detach().cpu().double().view(ndir, 4 * H)
    out = [[None] * T for _ in range(ndir)]
    gates = [[None] * T for _ in range(ndir)]
    cs = [[None] * T for _ in range(ndir)]
    zs = [[None] * T for _ in range(ndir)]
    for d in range(ndir):
        w = ws[d].detach().cpu().double()
        h, c = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        for step in range(T):
            t = step if d == 0 else T - 1 - step
            z = (x[:, t, d] + h @ w.t() + b[d]).requires_grad_(dout is not None)
            if dout is not None:
                z.retain_grad()
            i, f, g, o = z.chunk(4, 1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c = f * c + i * g
            h = o * torch.tanh(c)
            out[d][t], gates[d][t], cs[d][t], zs[d][t] = h, torch.cat([i, f, g, o], 1), c, z
    o = torch.stack([torch.stack(out[d], 1) for d in range(ndir)], 2).reshape(B, T, ndir * H)
    gt = torch.stack([torch.stack(gates[d], 1) for d in range(ndir)], 2)
    cq = torch.stack([torch.stack(cs[d], 1) for d in range(ndir)], 2)
    dg = None
    if dout is not None:
        o.backward(dout.detach().cpu().double())
        dg = torch.stack([torch.stack([z.grad for z in zs[d]], 1) for d in range(ndir)], 2)
    return o.detach(), gt.detach(), cq.detach(), dg


def packs_of(ops, ws, Hd):
    """(fp32 forward stack, fp32 transposed stack, x3 forward (streams, inv), x3 transposed (streams, inv)) of one layer's W_hh pair"""
    w_f32 = torch.stack([ops.pack_fragment_major(w, Hd) for w in ws]).contiguous()
    wT_f32 = torch.stack([ops.pack_fragment_major(w.t().contiguous(), Hd) for w in ws]).contiguous()
    p = [ops.pack_fragment_major_h(w, Hd) for w in ws]
    pT = [ops.pack_fragment_major_h(w.t().contiguous(), Hd) for w in ws]
    return (w_f32, wT_f32, (torch.stack([q[0] for q in p]).contiguous(), torch.cat([q[1] for q in p]).contiguous()),
            (torch.stack([q[0] for q in pT]).contiguous(), torch.cat([q[1] for q in pT]).contiguous()))


# ---- 1. BidirectionalLSTM against torch.nn.LSTM + Linear on the host -------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 31])
@pytest.mark.parametrize("Hd", [128, 512])
def test_bilstm_forward_backward_vs_torch(ops, Hd, T):
    """tests/test_width_gpu.py::test_bilstm_forward_backward_vs_torch with the hidden size as a parameter: inference (the x3 recurrence),
    training forward, dx and every parameter gradient; B = 19 is one full and one partial 16-row tile.  Band: that test's (atol 2e-5,
    _grad_check's 2e-3)."""
    from mrn_amd.modules.sequence_modeling import BidirectionalLSTM
    B, IN = 19, 64
    torch.manual_seed(Hd + T)
    mod = BidirectionalLSTM(IN, Hd, Hd)
    x = rnd(B, T, IN, seed=800 + T)
    xr = x.clone().requires_grad_(True)
    ref = mod.linear(mod.rnn(xr)[0])
    dy = rnd(B, T, Hd, seed=801 + T)
    ref.backward(dy)
    g_ref = {k: p.grad.clone() for k, p in mod.named_parameters()}
    mod.zero_grad()
    dev = BidirectionalLSTM(IN, Hd, Hd)
    dev.load_state_dict(mod.state_dict())
    dev = dev.cuda()
    with torch.no_grad(), recorded_calls() as log:
        y = dev(cu(x))
    assert "mrn_lstm_layer_fwd_x3_grouped" in [n for n, _ in log]
    print(f"[hidden {Hd} T {T}] inference err {float((y.cpu() - ref.detach()).abs().max()):.3e}")
    assert_close("bilstm inference", y, ref.detach(), atol=2e-5)
    xc = cu(x).requires_grad_(True)
    with recorded_calls() as log:
        out = dev(xc)
        assert_close("bilstm training forward", out, ref.detach(), atol=2e-5)
        out.backward(cu(dy))
        torch.cuda.synchronize()
    names = [n for n, _ in log]
    assert "mrn_lstm_layer_fwd_x3_save" in names and "mrn_lstm_layer_bwd_x3" in names
    _grad_check("bilstm dx", xc.grad, xr.grad)
    for k, p in dev.named_parameters():
        _grad_check("bilstm d" + k, p.grad, g_ref[k])


# ---- 2. grouped equals single -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 5])      # (5: ten sets -- a second round of eight pinned sets whose tail returns, in the fp32 kernel too)
@pytest.mark.parametrize("Hd", [128, 512])
def test_grouped_lstm_matches_single_launches(ops, Hd, G):
    B, T = 9, 7
    xproj = cu(rnd(G, B, T, 8 * Hd, seed=810 + Hd, scale=0.5))
    ws = [[cu(rnd(4 * Hd, Hd, seed=811 + 2 * g + d, scale=1 / 16.0)) for d in range(2)] for g in range(G)]
    b_hh = cu(rnd(G, 8 * Hd, seed=820, scale=1 / 16.0))
    pk = [packs_of(ops, w, Hd) for w in ws]
    w_hh = torch.stack([p[0] for p in pk]).contiguous()
    out = ops.lstm_layer_grouped(xproj, w_hh, b_hh, Hd, 2)
    w_h = torch.stack([p[2][0] for p in pk]).contiguous()
    w_inv = torch.stack([p[2][1] for p in pk]).contiguous()
    out3 = ops.lstm_layer_x3_grouped(xproj, w_h, w_inv, b_hh, Hd, 2)
    for g in range(G):
        assert torch.equal(out[g], ops.lstm_layer(xproj[g], w_hh[g], b_hh[g], Hd, 2))
        one = ops.lstm_layer_x3_grouped(xproj[g:g + 1].contiguous(), w_h[g:g + 1].contiguous(), w_inv[g:g + 1].contiguous(),
                                        b_hh[g:g + 1].contiguous(), Hd, 2)
        assert torch.equal(out3[g], one[0])
    assert_close("x3 vs exact fp32", out3, out, atol=2e-6, rtol=1e-5)


# ---- 3. the training kernels on the f16 MFMA, range safety ----------------------------------------------------------------------
@pytest.mark.parametrize("B,T,mag", [(19, 7, 1.0), (37, 31, 1e-5), (33, 31, 300.0)])
@pytest.mark.parametrize("Hd", [128, 512])
def test_lstm_training_kernels_on_f16_mfma(ops, Hd, B, T, mag):
    """tests/test_kernels_gpu.py::test_lstm_training_kernels_on_f16_mfma at the new sizes, at its bands against the exact-fp32 kernels
    (out / gates 2e-6 + 1e-5 rel, cell state 4e-6 + 1e-5 rel, gate gradients 2e-6 of their maximum).  Against float64 on the host the
    yardstick is the exact-fp32 kernel's own distance from float64: the x3 kernels may be that far plus the same band (the triangle
    inequality on the two comparisons; nothing measured on the kernels under test enters)."""
    ndir = 2
    xproj = cu(rnd(B, T, ndir * 4 * Hd, seed=840, scale=0.7))
    ws = [cu(rnd(4 * Hd, Hd, seed=841 + d, scale=1 / 16.0)) for d in range(ndir)]
    b_hh = cu(rnd(ndir * 4 * Hd, seed=850, scale=1 / 16.0))
    dout = cu(rnd(B, T, ndir * Hd, seed=860)) * mag
    w_f32, wT_f32, (w_h, w_inv), (wT_h, wT_inv) = packs_of(ops, ws, Hd)
    ref_out, ref_gates, ref_c = ops.lstm_layer(xproj, w_f32, b_hh, Hd, ndir, save=True)
    out, gates, cseq = ops.lstm_layer_x3_save(xproj, w_h, w_inv, b_hh, Hd, ndir)
    ref_dg = ops.lstm_layer_bwd(dout, ref_gates, ref_c, wT_f32, Hd, ndir)
    dg = ops.lstm_layer_bwd_x3(dout, ref_gates, ref_c, wT_h, wT_inv, Hd, ndir)
    o64, g64, c64, dg64 = lstm_ref64(xproj, ws, b_hh, dout)
    scale = float(ref_dg.abs().max())
    d = lambda a, b: float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())      # noqa: E731
    f32 = dict(out=d(ref_out, o64), gates=d(ref_gates, g64), c=d(ref_c, c64), dg=d(ref_dg, dg64))
    x3 = dict(out=d(out, o64), gates=d(gates, g64), c=d(cseq, c64), dg=d(dg, dg64))
    print(f"[hidden {Hd} B {B} T {T} mag {mag}] vs float64: exact fp32 {f32}, x3 {x3}, |dg|max {scale:.3e}, x3 vs fp32 dg {d(dg, ref_dg):.3e}")
    assert_close("x3 training forward: out", out, ref_out, atol=2e-6, rtol=1e-5)
    assert_close("x3 training forward: gates", gates, ref_gates, atol=2e-6, rtol=1e-5)
    assert_close("x3 training forward: cell state", cseq, ref_c, atol=4e-6, rtol=1e-5)
    assert d(dg, ref_dg) <= 2e-6 * scale, (d(dg, ref_dg), scale)
    assert abs(scale - float(dg64.abs().max())) <= 1e-3 * scale
    assert x3["out"] <= f32["out"] + 2e-6 + 1e-5 * float(o64.abs().max())
    assert x3["gates"] <= f32["gates"] + 2e-6 + 1e-5 * float(g64.abs().max())
    assert x3["c"] <= f32["c"] + 4e-6 + 1e-5 * float(c64.abs().max())
    assert x3["dg"] <= f32["dg"] + 2e-6 * scale
    # and the exact-fp32 kernels themselves are fp32 round-off away from float64 (2e-5: the band of the layer against torch, case 1)
    assert f32["out"] <= 2e-5 and f32["gates"] <= 2e-5 and f32["dg"] <= 2e-3 * scale


# ---- 4. / 9. every entry point against float64: the unit-pass order at 512, the dispatch at 256 --------------------------------------
def _all_entry_points_vs_float64(ops, Hd, ws, B=9, T=7, G=2):
    """the four forward entry points (single / grouped exact fp32, grouped x3, x3 with saves) and the two backward ones on one layer pair
    `ws` against float64: outputs to 2e-5 (the band of the layer against torch), gate gradients to _grad_check's 2e-3"""
    ndir = 2
    xproj = cu(rnd(B, T, ndir * 4 * Hd, seed=870 + Hd, scale=0.7))
    b_hh = cu(rnd(ndir * 4 * Hd, seed=871, scale=1 / 16.0))
    dout = cu(rnd(B, T, ndir * Hd, seed=872))
    w_f32, wT_f32, (w_h, w_inv), (wT_h, wT_inv) = packs_of(ops, ws, Hd)
    o64, g64, c64, dg64 = lstm_ref64(xproj, ws, b_hh, dout)
    out, gates, cseq = ops.lstm_layer(xproj, w_f32, b_hh, Hd, ndir, save=True)
    assert_close("lstm_layer out", out, o64, atol=2e-5, rtol=0)
    assert_close("lstm_layer gates", gates, g64, atol=2e-5, rtol=0)
    assert_close("lstm_layer cell state", cseq, c64, atol=2e-5, rtol=1e-5)
    xg = torch.stack([xproj] * G).contiguous()
    bg = torch.stack([b_hh] * G).contiguous()
    og = ops.lstm_layer_grouped(xg, torch.stack([w_f32] * G).contiguous(), bg, Hd, ndir)
    o3 = ops.lstm_layer_x3_grouped(xg, torch.stack([w_h] * G).contiguous(), torch.stack([w_inv] * G).contiguous(), bg, Hd, ndir)
    for g in range(G):
        assert_close("lstm_layer_grouped out", og[g], o64, atol=2e-5, rtol=0)
        assert_close("lstm_layer_x3_grouped out", o3[g], o64, atol=2e-5, rtol=0)
    out3, gates3, cseq3 = ops.lstm_layer_x3_save(xproj, w_h, w_inv, b_hh, Hd, ndir)
    assert_close("lstm_layer_x3_save out", out3, o64, atol=2e-5, rtol=0)
    assert_close("lstm_layer_x3_save gates", gates3, g64, atol=2e-5, rtol=0)
    assert_close("lstm_layer_x3_save cell state", cseq3, c64, atol=2e-5, rtol=1e-5)
    _grad_check("lstm_layer_bwd", ops.lstm_layer_bwd(dout, gates, cseq, wT_f32, Hd, ndir), dg64)
    _grad_check("lstm_layer_bwd_x3", ops.lstm_layer_bwd_x3(dout, gates3, cseq3, wT_h, wT_inv, Hd, ndir), dg64)
    return o64


@pytest.mark.parametrize("mask", ["rows", "rows_and_columns"])
def test_unit_pass_order_at_512(ops, mask):
    """W_hh non-zero only in the rows of the units >= 256 (the second pass's), and then only in the columns >= 256 (so that the second
    pass's units depend on nothing but the second pass's h of the previous step): a pass that read the half-updated h of its own step
    would show here and nowhere else"""
    Hd = 512
    ws = []
    for d in range(2):
        w = rnd(4 * Hd, Hd, seed=880 + d, scale=1 / 8.0).view(4, Hd, Hd)
        w[:, :256, :] = 0.0
        if mask == "rows_and_columns":
            w[:, :, :256] = 0.0
        ws.append(cu(w.view(4 * Hd, Hd).contiguous()))
    o64 = _all_entry_points_vs_float64(ops, Hd, ws)
    assert float(o64.abs().max()) > 0.1


def test_entry_points_at_256_are_unchanged(ops):
    """guards the dispatch on `hidden` (not bit-equality): each of the six entry points at 256 against float64"""
    Hd = 256
    _all_entry_points_vs_float64(ops, Hd, [cu(rnd(4 * Hd, Hd, seed=890 + d, scale=1 / 16.0)) for d in range(2)])


# ---- 5. whole nets against the fixture and the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hidden,imgW,B,seed", HIDDEN_CASES)
def test_mrn2_vs_reference_fixture(kind, hidden, imgW, B, seed):
    """the reference's own outputs (tests/golden/hidden.npz, two experts): loop A, loop B and eval with the assertions and bands of
    tests/test_width_gpu.py::test_mrn2_vs_reference_fixture (1e-4 absolute + 1e-4 of the maximum; indices exact)"""
    from mrn_amd import functional as Fn
    from tests.test_model_gpu import set_drop_masks_from
    g = load_golden("hidden")
    p = f"{kind}{hidden}/"
    opt, net = build_mrn(kind, hidden, imgW, CLASSES)
    image, tgt, lens = hidden_targets(kind, hidden, imgW, B, seed)

    def check(name, t, full=False):
        mine = (t.detach().cpu().double().numpy() if full else sub(t)[0].astype(np.float64))
        ref = g[p + name] if full else g[p + name + "/sub"].astype(np.float64)
        tol = 1e-4 + 1e-4 * np.abs(ref).max()
        err = np.abs(mine - ref).max()
        print(f"[hidden fixture {kind} {hidden}] {name}: max abs err {err:.3e}, tol {tol:.3e}")
        assert err <= tol, f"{name}: max abs err {err:.3e} > tol {tol:.3e}"

    def reload():
        net.load_state_dict(hidden_state_dict(g, p, seed), strict=True)

    reload()
    net = net.cuda().train()
    assert net.out_dim == hidden and net.feature_dim == 2 * hidden and net.channel_route.in_features == 2 * hidden
    with torch.no_grad():
        m = hidden_masks(kind, hidden, B, seed, "e0")
        set_drop_masks_from(net, [m[0], m[0]] if m else None)
        check("e0/feature", net.model[0](image.cuda(), None, True)["feature"])
        reload()
        set_drop_masks_from(net, hidden_masks(kind, hidden, B, seed, "stepB", 2))
        out = net(image.cuda(), True, None, True)
        check("stepB/weights", out["index"], full=True)
        check("stepB/logits", out["logits"])
        assert np.array_equal(out["index"].cpu().numpy().argmax(1), g[p + "stepB/weights"].argmax(1))
    # loop A: the newest expert's logits, loss and the fixture's four parameter gradients
    reload()
    for n, q in net.named_parameters():
        q.requires_grad = n.startswith("model.1.")
    m = hidden_masks(kind, hidden, B, seed, "stepA")
    set_drop_masks_from(net, [m[0], m[0]] if m else None)
    preds = net(image.cuda(), False)["logits"]
    check("stepA/logits", preds)
    loss = Fn.ctc_loss(preds, tgt.cuda(), lens.cuda())
    ref_loss = float(g[p + "stepA/loss"])
    assert abs(loss.item() - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss)), (loss.item(), ref_loss)
    loss.backward()
    mine = dict(net.named_parameters())
    names = [str(k)[len(p + "stepA/grad/"):-len("/sub")] for k in g.files if k.startswith(p + "stepA/grad/") and k.endswith("/sub")]
    assert len(names) == 4
    for n in names:
        a, b = sub(mine[n].grad)[0].astype(np.float64), g[p + "stepA/grad/" + n + "/sub"].astype(np.float64)
        l2, mx = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12), np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)
        print(f"[hidden fixture {kind} {hidden}] grad {n}: rel L2 {l2:.2e}, rel max {mx:.2e}")
        assert l2 <= 2e-3 and mx <= 2e-3, (n, l2, mx)                      # (_grad_check's band on the stored subsample)
    # eval: hard routing and argmax
    reload()
    net.eval()
    with torch.no_grad():
        oe = net(image.cuda(), True, None, False)
    assert np.array_equal(oe["index"].cpu().numpy(), g[p + "eval/index"])
    check("eval/logits", oe["logits"])
    assert float((oe["logits"].max(2)[1].cpu().numpy() == g[p + "eval/argmax"]).mean()) >= 0.99


def test_dernet_crnn3_ctc_at_128_vs_oracle():
    """three CRNN extractors, CTC head over feature_dim = 128 * 3, auxiliary head over the newest 128, B = 4, against the oracle's DER
    forward (band of tests/test_width_gpu.py::test_dernet_step_vs_oracle_32x384: 1e-4)"""
    from mrn_amd.modules.model import DERNet
    from mrn_amd.tools import weights as W
    from oracle import mrn_oracle as O
    hidden, imgW, B, classes = 128, 128, 4, (40, 70, 97)
    opt = make_opt("crnn", hidden, imgW)
    with contextlib.redirect_stdout(io.StringIO()):
        net = DERNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
            net.build_aux_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed=37)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert net.out_dim == hidden and net.feature_dim == 3 * hidden
    assert net.fc.in_features == 3 * hidden and net.aux_fc.in_features == hidden
    net = net.cuda().train()
    for ext in list(net.model)[:-1]:
        ext.eval()
    image = torch.from_numpy(W.smooth_image("hidden_der", (B, 4, 32, imgW), 37))
    cfg = O.Cfg(*STAGES["crnn"], imgH=32, imgW=imgW, hidden_size=hidden)
    with torch.no_grad():
        ref = O.dernet_forward(sd, cfg, 3, image, None, True, training=True)
        out = net(image.cuda())
    assert out["features"].shape == (B, 31, 3 * hidden)
    assert_close("DER features", out["features"], ref["features"], atol=1e-4)
    assert_close("DER logits", out["logits"], ref["logits"], atol=1e-4)
    assert_close("DER aux logits", out["aux_logits"], ref["aux_logits"], atol=1e-4)


# ---- 6. one LwF run and one training-driver task at 128 ------------------------------------------------------------------------------
def test_lwf_learner_two_tasks_at_128(tmp_path):
    from mrn_amd.data.synthetic import SyntheticTextLines, SyntheticValidation, synthetic_characters
    from mrn_amd.il_modules.lwf import LwF
    from tests.test_learner_gpu import make_opt as learner_opt
    os.chdir(tmp_path)
    opt = learner_opt(tmp_path, "crnn")
    opt.il, opt.memory, opt.hidden_size, opt.num_iter, opt.val_interval = "lwf", None, 128, 2, 2
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = LwF(opt)
        train, valid = SyntheticTextLines(opt), SyntheticValidation(opt)
        chars = ""
        for taski, n_new in enumerate((30, 20)):             # (the second task takes the distillation step against the first's model)
            chars = synthetic_characters(len(chars) + n_new)
            train.set_characters(chars)
            valid.set_characters(chars)
            learner.incremental_train(taski, chars, train, valid)
            learner.after_task()
    net = learner.model
    assert net.fc.in_features == 128 and net.fc.out_features == 54
    assert all(torch.isfinite(p).all() for p in net.parameters())


def test_tiny_train_one_task_at_hidden_128(tmp_path):
    """tests/test_width_gpu.py::test_tiny_train_one_task_at_32x128's options with hidden_size = 128"""
    from torch.utils.data import ConcatDataset
    from mrn_amd import tiny_train
    from mrn_amd.data.data_manage import Dataset_Manager, Val_Dataset
    from mrn_amd.data.dataset import ArrayDataset
    from tests.helpers import fake_text_samples
    os.chdir(tmp_path)
    opt = types.SimpleNamespace(
        exp_name="t", il="mrn", memory="random", memory_num=20, batch_max_length=25, imgH=32, imgW=128, manual_seed=111,
        start_task=0, num_fiducial=20, input_channel=4, output_channel=512, hidden_size=128, schedule="super",
        optimizer="adam", lr=0.0005, batch_size=6, num_iter=4, val_interval=2, grad_clip=5, lan_list=["A"], NED=True,
        workers=0, select_data=["rootA"], valid_datas=["valA"], Aug="None")
    opt.Transformation, opt.FeatureExtraction, opt.SequenceModeling, opt.Prediction = STAGES["crnn"]

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
    assert learner.model.patch == 31 and learner.model.out_dim == 128
    assert all(torch.isfinite(p).all() for p in learner.model.parameters())


# ---- 7. reduced mode --------------------------------------------------------------------------------------------------------------------
def test_reduced_mode_loop_b_at_512():
    """loop B of CRNN x 2 at hidden 512 with the plain-fp16 products against parity mode: the band of
    tests/test_width_gpu.py::test_reduced_mode_loop_b (routing weights 2e-2, logits 5e-2 of their maximum)"""
    from mrn_amd import ops
    from mrn_amd.tools import weights as W
    hidden, imgW, B, seed = 512, 128, 8, 41
    opt, net = build_mrn("crnn", hidden, imgW, CLASSES)
    W.fill_state_dict(net.state_dict(), seed=seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().train()
    image = torch.from_numpy(W.smooth_image("hidden_reduced", (B, 4, 32, imgW), seed)).cuda()
    with torch.no_grad():
        ref = net(image, True, None, True)
    saved = ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS
    try:
        ops.X3_PRODUCTS = ops.TRAIN_PRODUCTS = 1            # bench.py --precision fp16
        net.load_state_dict(sd, strict=True)                # (the same running statistics before the step)
        with torch.no_grad(), recorded_calls() as log:
            out = net(image, True, None, True)
        torch.cuda.synchronize()
    finally:
        ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS = saved
    assert any(n == "mrn_lstm_layer_fwd_x3_grouped" for n, _ in log)
    w, w0 = out["index"].cpu(), ref["index"].cpu()
    lg, lg0 = out["logits"].cpu(), ref["logits"].cpu()
    err_w = float((w - w0).abs().max())
    err_l = float((lg - lg0).abs().max()) / max(float(lg0.abs().max()), 1e-6)
    print(f"[hidden 512 reduced] routing weights err {err_w:.3e}, logits err {err_l:.3e} of the maximum")
    assert torch.isfinite(lg).all()
    assert err_w <= 2e-2 and err_l <= 5e-2, (err_w, err_l)
    assert err_w > 1e-7 or err_l > 1e-7                     # the reduced arithmetic really ran


# ---- 8. refusals, before any launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hidden", [("trba", 128), ("crnn", 192)])
def test_unsupported_hidden_is_refused_before_any_launch(kind, hidden):
    from mrn_amd.modules.model import DERNet, Model
    from mrn_amd.modules.prediction import Attention
    from mrn_amd.modules.sequence_modeling import BidirectionalLSTM
    torch.cuda.synchronize()
    with recorded_calls() as log:
        with pytest.raises(NotImplementedError, match=HIDDEN_SET + ".*attention head runs 256 only"):
            build_mrn(kind, hidden, 256, (41,))
        with contextlib.redirect_stdout(io.StringIO()), pytest.raises(NotImplementedError, match=HIDDEN_SET):
            Model(make_opt(kind, hidden, 256))
        with contextlib.redirect_stdout(io.StringIO()), pytest.raises(NotImplementedError, match=HIDDEN_SET):
            DERNet(make_opt(kind, hidden, 256))
        if kind == "trba":
            att = Attention(256, hidden, 41, torch.nn.Linear(hidden, 41)).cuda().eval()
            with torch.no_grad(), pytest.raises(NotImplementedError, match="attention head runs 256 only"):
                att(torch.zeros(2, 33, 256, device="cuda"), torch.full((2, 26), 2, dtype=torch.int64, device="cuda"), True)
        else:
            seq = BidirectionalLSTM(64, hidden, hidden).cuda().eval()
            with torch.no_grad(), pytest.raises(NotImplementedError, match=HIDDEN_SET):
                seq(torch.zeros(2, 7, 64, device="cuda"))
            x = torch.zeros(2, 7, 64, device="cuda", requires_grad=True)
            with pytest.raises(NotImplementedError, match=HIDDEN_SET):
                seq.train()(x)
    assert log == []
