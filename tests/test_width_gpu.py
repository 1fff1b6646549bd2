"""Input widths 128 ... 512 on the GPU: every kernel family at the map widths those inputs produce (the odd tails 33 / 129 of the
ResNet stack, 31 / 127 of the VGG stack, the short sequence lengths of the recurrences and losses) against torch on the host, the
CRNN / TRBA MRN stacks against the CPU oracle and the reference fixture (tests/golden/width.npz) at 32 x 128, 32 x 512, 48 x 320
and 64 x 192 (forward, loop A, loop B, DER, reduced mode), the per-call pixel budget, the refusals, and the training driver end to
end.  Bands are those of tests/test_geometry_gpu.py / tests/test_kernels_gpu.py (whose parametrised bodies the kernel cases call
with the new shapes)."""
import contextlib
import io
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import assert_close, oracle_dtype
from tests.test_geometry_gpu import _grad_check
from tests.test_kernels_gpu import cu, ops, rnd  # noqa: F401  (ops: the module-scoped fixture that loads the library)

pytestmark = pytest.mark.gpu

CLASSES = {"crnn": (40, 70, 97), "trba": (41, 71, 98)}
CFG = {"crnn": ("None", "VGG", "BiLSTM", "CTC"), "trba": ("TPS", "ResNet", "BiLSTM", "Attn")}
GEOMETRIES = ((32, 128), (32, 512), (48, 320), (64, 192))
WIDTH_SET = r"\{128, 192, 256, 320, 384, 448, 512\}"


def make_opt(kind, imgH, imgW, bml=25):
    o = types.SimpleNamespace(num_fiducial=20, imgH=imgH, imgW=imgW, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=bml)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = CFG[kind]
    return o


def build_mrn(kind, imgH, imgW, classes, seed, bml=25):
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as W
    opt = make_opt(kind, imgH, imgW, bml)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed=seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return opt, net.cuda(), sd


def inputs(kind, imgH, imgW, B, classes, seed, bml=25):
    from mrn_amd.tools import weights as W
    image = torch.from_numpy(W.smooth_image(f"width_{kind}_{imgH}x{imgW}", (B, 4, imgH, imgW), seed))
    if kind == "trba":
        text = torch.from_numpy(W.randint(f"width_text_{imgH}x{imgW}", (B, bml + 2), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None
    lens = torch.from_numpy(W.randint(f"width_len_{imgH}x{imgW}", (B,), 1, bml + 1, seed)).int()
    labels = torch.from_numpy(W.randint(f"width_ctc_{imgH}x{imgW}", (B, bml), 4, classes[-1], seed))
    labels[torch.arange(bml)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


@contextlib.contextmanager
def recorded_calls():
    """names (and results) of every C-ABI call made inside the block"""
    from mrn_amd import _lib
    log, real = [], _lib.LIB.call

    def spy(name, *a):
        rc = real(name, *a)
        log.append((name, rc))
        return rc
    _lib.LIB.call = spy
    try:
        yield log
    finally:
        del _lib.LIB.call           # (the instance attribute: the class's method is back)


# ---- 1. the kernels at the map widths the new inputs produce ----------------------------------------------------------------
# ResNet: W -> W/2 -> W/4 -> W/4 + 1 (33 ... 129) -> W/4 + 2 -> W/4 + 1;  VGG: W -> W/2 -> W/4 -> W/4 - 1 (31 ... 127)
@pytest.mark.parametrize("G,B,H,W,Cout,shared,act", [(2, 2, 32, 128, 32, False, 0), (2, 2, 32, 512, 64, True, 1), (1, 2, 48, 320, 64, True, 0),
                                                     (2, 1, 64, 192, 32, False, 1)])
def test_first_conv_at_width(ops, G, B, H, W, Cout, shared, act):
    from tests.test_kernels_gpu import test_first_conv_c4_grouped
    test_first_conv_c4_grouped(ops, G, B, H, W, Cout, shared, act)


@pytest.mark.parametrize("G,B,H,W,Cin,Cout,shared", [(2, 2, 16, 192, 32, 64, False), (2, 2, 8, 96, 64, 128, False), (2, 1, 32, 512, 32, 64, False),
                                                     (1, 2, 24, 160, 32, 64, True), (2, 2, 16, 64, 32, 64, False)])
def test_patch_resident_conv_at_width(ops, G, B, H, W, Cin, Cout, shared):
    from tests.test_kernels_gpu import test_patch_resident_conv
    test_patch_resident_conv(ops, G, B, H, W, Cin, Cout, shared)


X3_AT_WIDTH = [
    # G, B, H, W, Cin, Cout, k, s, p, shared input
    (3, 3, 4, 33, 64, 128, (3, 3), (1, 1), (1, 1), False),      # ResNet stage 4 at 32 x 128
    (2, 2, 4, 129, 64, 128, (3, 3), (1, 1), (1, 1), False),     #   ... at 32 x 512
    (2, 2, 6, 81, 64, 96, (3, 3), (1, 1), (1, 1), False),       #   ... at 48 x 320
    (2, 2, 4, 33, 64, 256, (2, 2), (2, 1), (0, 1), False),      # ResNet conv4_1 at 32 x 128: 4 x 33 -> 2 x 34
    (2, 2, 2, 130, 64, 256, (2, 2), (1, 1), (0, 0), False),     # ResNet conv4_2 at 32 x 512: 2 x 130 -> 1 x 129
    (2, 3, 3, 32, 64, 256, (2, 2), (1, 1), (0, 0), False),      # VGG's last conv at 48 x 128: 3 x 32 -> 2 x 31
    (2, 2, 2, 128, 64, 256, (2, 2), (1, 1), (0, 0), False),     # VGG's last conv at 32 x 512: 2 x 128 -> 1 x 127
    (2, 2, 8, 96, 32, 64, (3, 3), (1, 1), (1, 1), True),        # a pooled early map, one input for all groups
    (2, 62, 1, 1, 64, 96, (1, 1), (1, 1), (0, 0), False),       # a grouped Linear over B * T = 2 * 31 rows
]


@pytest.mark.parametrize("cfg", X3_AT_WIDTH)
def test_grouped_x3_conv_at_width(ops, cfg):
    from tests.test_kernels_gpu import test_grouped_x3_conv_bn_pool
    test_grouped_x3_conv_bn_pool(ops, cfg)


@pytest.mark.parametrize("cfg", [(2, 4, 33, 128, 128, (3, 3), (1, 1), (1, 1)), (2, 4, 129, 4, 32, (3, 3), (1, 1), (1, 1)),
                                 (2, 3, 32, 128, 512, (2, 2), (1, 1), (0, 0)), (2, 16, 192, 32, 64, (3, 3), (1, 1), (1, 1))])
def test_single_conv_and_batch_stats_at_width(ops, cfg):
    from tests.test_kernels_gpu import test_conv2d_and_batch_stats
    test_conv2d_and_batch_stats(ops, cfg)


WINO_AT_WIDTH = [
    # G, B, H, W, Cin, Cout, shortcut, relu
    (2, 3, 4, 33, 64, 128, "hl32", True),        # ResNet stage 4 at 32 x 128 (one column of the last group inside the row)
    (2, 2, 4, 129, 128, 256, "none", True),      #   ... at 32 x 512
    (2, 2, 6, 81, 64, 96, "f32", True),          #   ... at 48 x 320: a 6-row map
    (1, 2, 12, 49, 64, 64, "hl32", True),        #   ... at 64 x 192 (stage 3 of a taller input)
    (3, 2, 8, 96, 128, 128, "none", True),       # a pooled map of whole column groups
    (2, 2, 16, 192, 32, 64, "none", True),       # an early map of a 512-pixel line
    (2, 3, 2, 32, 128, 128, "none", True),       # VGG's 512-channel layers at 32 x 128
    (2, 2, 2, 128, 128, 128, "none", False),     #   ... at 32 x 512
]


@pytest.mark.parametrize("R", [4, 2])
@pytest.mark.parametrize("cfg", WINO_AT_WIDTH)
def test_winograd_conv_at_width(ops, cfg, R):
    from mrn_amd._lib import call
    from tests.test_kernels_gpu import test_winograd_conv_matches_direct
    G, B, H, W, Cin, Cout, _, _ = cfg
    # the form: the row-block rule depends on (H, R, Cout) only -- a 33- or 129-wide map takes the kernel a 65-wide one takes
    assert bool(call("mrn_conv2d_x3_wino_rows", H, R, Cout)) == (R == 4 and H % 4 == 0)
    test_winograd_conv_matches_direct(ops, cfg, R)


@pytest.mark.parametrize("cfg", [(2, 2, 4, 33, 128, 128, "hl32", True), (2, 2, 4, 129, 64, 160, "none", True), (2, 2, 8, 96, 128, 256, "none", True)])
def test_winograd_reduced_mode_at_width(ops, cfg):
    from tests.test_kernels_gpu import test_winograd_d16_reduced_mode
    test_winograd_d16_reduced_mode(ops, cfg)


@pytest.mark.parametrize("G,B,H,W,C,pool", [(2, 2, 8, 96, 64, ((2, 2), (2, 2), (0, 0))), (2, 2, 8, 32, 64, ((2, 2), (2, 1), (0, 1))),
                                            (2, 2, 8, 128, 32, ((2, 2), (2, 1), (0, 1))), (1, 2, 4, 32, 64, ((2, 1), (2, 1), (0, 0)))])
def test_maxpool_winograd_producer_at_width(ops, G, B, H, W, C, pool):
    from tests.test_kernels_gpu import test_maxpool_winograd_producer
    test_maxpool_winograd_producer(ops, G, B, H, W, C, pool)


@pytest.mark.parametrize("H,W,Cin,Cout", [(4, 33, 128, 128), (4, 129, 64, 128), (6, 81, 128, 64), (2, 32, 128, 256), (16, 192, 32, 64),
                                          (32, 128, 4, 32)])
def test_trained_conv_fwd_dgrad_wgrad_at_width(ops, H, W, Cin, Cout):
    """ConvBlockFn (3x3 / stride 1 / pad 1: the Winograd form from Cin = 128, the direct form below) -- forward, data, weight and bias
    gradients against torch autograd"""
    from tests.test_kernels_gpu import test_strided_conv_block_gradients
    test_strided_conv_block_gradients(ops, H, W, Cin, Cout, (1, 1))


@pytest.mark.parametrize("B,H,W,Cin,Cout,magnitude", [(3, 4, 33, 128, 128, 1.0), (2, 4, 129, 512, 512, 1e-5), (2, 6, 81, 128, 256, 300.0)])
def test_trained_conv_winograd_at_width(ops, B, H, W, Cin, Cout, magnitude):
    from tests.test_kernels_gpu import test_trained_conv_winograd_range_safe
    test_trained_conv_winograd_range_safe(ops, B, H, W, Cin, Cout, magnitude)


@pytest.mark.parametrize("cfg", [(3, 4, 33, 64, 128, (3, 3), (1, 1), (1, 1)), (2, 4, 129, 32, 64, (3, 3), (1, 1), (1, 1)),
                                 (2, 2, 130, 64, 128, (2, 2), (1, 1), (0, 0)), (3, 3, 32, 64, 96, (2, 2), (1, 1), (0, 0))])
@pytest.mark.parametrize("magnitude", [1.0, 1e-6])
def test_conv_weight_gradient_at_width(ops, cfg, magnitude):
    from tests.test_kernels_gpu import test_conv_weight_gradient_x3
    test_conv_weight_gradient_x3(ops, cfg, magnitude)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(32, 4, 33, 64, 128), (32, 4, 129, 128, 96), (4, 16, 192, 32, 64), (8, 2, 32, 64, 48)])
def test_wgrad_without_im2col_at_width(B, H, W, Cin, Cout):
    from tests.test_kernels_gpu import test_wgrad_without_im2col_matches_exact_fp32
    test_wgrad_without_im2col_matches_exact_fp32(B, H, W, Cin, Cout)


@pytest.mark.parametrize("B,H,W,Cin,Cout,magnitude", [(32, 4, 33, 128, 128, 1e-4), (32, 4, 129, 128, 256, 30.0), (8, 2, 32, 256, 128, 1e-4)])
def test_wgrad_in_the_winograd_domain_at_width(B, H, W, Cin, Cout, magnitude):
    from tests.test_kernels_gpu import test_wgrad_in_the_winograd_domain
    test_wgrad_in_the_winograd_domain(B, H, W, Cin, Cout, magnitude)


@pytest.mark.parametrize("T", [31, 129])
def test_bilstm_forward_backward_vs_torch(ops, T):
    """BidirectionalLSTM (inference: the x3 recurrence; training: BiLSTMFn with saves + backward through time) against torch.nn.LSTM +
    Linear on the host at the shortest and the longest supported sequence"""
    from mrn_amd.modules.sequence_modeling import BidirectionalLSTM
    B, IN, Hd = 11, 512, 256
    torch.manual_seed(T)
    mod = BidirectionalLSTM(IN, Hd, Hd)
    x = rnd(B, T, IN, seed=600 + T)
    xr = x.clone().requires_grad_(True)
    ref = mod.linear(mod.rnn(xr)[0])
    dy = rnd(B, T, Hd, seed=601 + T)
    ref.backward(dy)
    g_ref = {k: p.grad.clone() for k, p in mod.named_parameters()}
    mod.zero_grad()
    dev = BidirectionalLSTM(IN, Hd, Hd)
    dev.load_state_dict(mod.state_dict())
    dev = dev.cuda()
    with torch.no_grad():
        assert_close("bilstm inference", dev(cu(x)), ref.detach(), atol=2e-5)
    xc = cu(x).requires_grad_(True)
    out = dev(xc)
    assert_close("bilstm training forward", out, ref.detach(), atol=2e-5)
    out.backward(cu(dy))
    _grad_check("bilstm dx", xc.grad, xr.grad)
    for k, p in dev.named_parameters():
        _grad_check("bilstm d" + k, p.grad, g_ref[k])


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("T", [31, 129])
def test_grouped_lstm_matches_single_launches_at_T(ops, G, T):
    B, Hd = 9, 256
    xproj = cu(rnd(G, B, T, 8 * Hd, seed=610 + T, scale=0.5))
    w_hh = torch.stack([torch.stack([ops.pack_fragment_major(cu(rnd(4 * Hd, Hd, seed=611 + 2 * g + d, scale=1 / 16.0)))
                                     for d in range(2)]) for g in range(G)]).contiguous()
    b_hh = cu(rnd(G, 8 * Hd, seed=620, scale=1 / 16.0))
    out = ops.lstm_layer_grouped(xproj, w_hh, b_hh, Hd, 2)
    for g in range(G):
        assert torch.equal(out[g], ops.lstm_layer(xproj[g], w_hh[g], b_hh[g], Hd, 2))


@pytest.mark.parametrize("B,T,mag", [(19, 31, 1.0), (37, 129, 1e-5), (256, 129, 300.0)])
def test_lstm_training_kernels_at_T(ops, B, T, mag):
    from tests.test_kernels_gpu import test_lstm_training_kernels_on_f16_mfma
    test_lstm_training_kernels_on_f16_mfma(ops, B, T, mag)


@pytest.mark.parametrize("D", [256, 1536])
@pytest.mark.parametrize("T", [33, 129])
def test_attention_decoder_forward_backward_at_T(ops, D, T):
    """the teacher-forced decoder (forward with saves, BPTT) against autograd through the oracle's step loop, D = 256 (an MRN expert) and
    1536 (a six-extractor DERNet head); at both the forward keeps its single-launch form (the tile's whole context in LDS)"""
    from tests.test_kernels_gpu import test_attention_decoder_backward
    assert ops.attn_decoder_whole_context(D, T, True) and ops.attn_decoder_whole_context(D, T, False)
    assert not ops.attn_decoder_whole_context(2048, T, True)            # (eight extractors: the chunked form, as at T = 65)
    test_attention_decoder_backward(ops, 21, D, T, 26)


@pytest.mark.parametrize("D", [256, 1536])
@pytest.mark.parametrize("T", [33, 129])
def test_grouped_decoder_single_launch_form_at_T(ops, D, T, monkeypatch):
    """mrn_attn_decoder_fwd_x3_grouped at T = 33 / 129: bit-identical to one launch per expert, and -- the single-launch form being the
    one taken -- only round-off away from the chunked form when that one is forced"""
    G, B, Hd, S = 3, 19, 256, 7
    Hb, Hproj = cu(rnd(G, B, T, D, seed=641)), cu(rnd(G, B, T, Hd, seed=642))
    eproj = cu(rnd(G, B, S, 4 * Hd, seed=643, scale=0.5))
    mk = lambda shape, seed: [cu(rnd(*shape, seed=seed + g, scale=1 / 16.0)) for g in range(G)]        # noqa: E731
    packs = [ops.pack_decoder_x3(a, b, c, D) for a, b, c in zip(mk((Hd, Hd), 650), mk((4 * Hd, D + 256), 660), mk((4 * Hd, Hd), 670))]
    b_h2h, w_score, b_hh2 = mk((Hd,), 680), mk((1, Hd), 690), mk((4 * Hd,), 700)
    args = ([p[0] for p in packs], b_h2h, w_score, [p[1] for p in packs], [p[2] for p in packs], b_hh2, Hd)
    hid = ops.attn_decoder_grouped(Hb, Hproj, eproj, *args, w_inv=[p[3] for p in packs])
    for g in range(G):
        one = ops.attn_decoder(Hb[g], Hproj[g], eproj[g], packs[g][0], b_h2h[g], w_score[g], packs[g][1], packs[g][2], b_hh2[g], Hd,
                               w_inv=packs[g][3])
        assert torch.equal(hid[g], one)
    monkeypatch.setenv("MRN_ATTN_CTX_CHUNK", "1")
    chunked = ops.attn_decoder_grouped(Hb, Hproj, eproj, *args, w_inv=[p[3] for p in packs])
    monkeypatch.delenv("MRN_ATTN_CTX_CHUNK")
    assert_close("chunked vs single launch", chunked, hid, atol=1e-6, rtol=1e-6)
    assert torch.equal(ops.attn_decoder_grouped(Hb, Hproj, eproj, *args, w_inv=[p[3] for p in packs]), hid)


def _labels_with_repeats(B, T, C, seed, W=25, lengths=None):
    """[B, 25] padded labels of 16 .. 25 characters built from runs of equal characters: sample b has `rep` adjacent equal pairs, chosen so
    that L + rep sits at T - 1, T (both feasible), T + 1 or beyond (no alignment in T frames) in turn.  W / lengths: another padded width
    and the B label lengths (0 .. W) instead of 17 .. 25; a label of L characters can hold at most L - 1 pairs"""
    g = torch.Generator().manual_seed(seed)
    tg = torch.ones(B, W, dtype=torch.int64)
    tl = torch.zeros(B, dtype=torch.int32)
    need = []
    for b in range(B):
        L = 17 + (b * 3) % 9 if lengths is None else lengths[b]         # 17 .. 25
        rep = min(max(L - 1, 0), max(0, T - L + (-1, 1, 0, 3, -6, 2)[b % 6]))
        same = set(torch.randperm(max(L - 1, 0), generator=g)[:rep].add(1).tolist())
        ch = int(torch.randint(2, C, (1,), generator=g))
        for i in range(L):
            if i and i not in same:
                nxt = int(torch.randint(2, C - 1, (1,), generator=g))
                ch = nxt + (nxt >= ch)                                  # any class but the previous one
            tg[b, i] = ch
        tl[b] = L
        need.append(L + rep)
    return tg, tl, need


@pytest.mark.parametrize("B", [12, 64])
def test_ctc_kernels_with_infeasible_samples_at_T31(ops, B):
    """T = 31 (VGG at 32 x 128): a 20-character label with twelve doubled letters has no alignment.  Under zero_infinity such a sample
    contributes loss 0 and gradient 0 while the others keep their 1 / (L * B) weights: the 64-state kernel (which never met one at
    T = 63), the long kernel and the ops entry against torch.nn.CTCLoss(reduction="mean", zero_infinity=True), value and gradient"""
    from tests.test_long_labels_gpu import direct_ctc, torch_ctc
    T, C = 31, 40
    logits = rnd(B, T, C, seed=700 + B, scale=3.0)
    tg, tl, need = _labels_with_repeats(B, T, C, seed=B)
    lp = logits.log_softmax(2).permute(1, 0, 2)
    per = torch.nn.CTCLoss(reduction="none")(lp, tg, torch.full((B,), T, dtype=torch.int32), tl)
    bad = torch.isinf(per)
    assert B // 4 <= int(bad.sum()) <= 3 * B // 4, int(bad.sum())
    assert bad.tolist() == [n > T for n in need]
    ref, gref = torch_ctc(logits, tg, tl)
    assert torch.isfinite(ref) and float(ref) > 0
    for long_kernel in (False, True):
        loss, nll, dl = direct_ctc(logits, tg, tl, long_kernel)
        assert_close(f"ctc loss (long={long_kernel})", loss, ref.view(1), atol=1e-5, rtol=1e-5)
        assert_close(f"ctc grad (long={long_kernel})", dl, gref, atol=2e-6, rtol=1e-4)
        assert torch.isinf(nll[bad]).all() and torch.isfinite(nll[~bad]).all()
        assert float(dl[bad].abs().max()) == 0.0
        assert float(dl[~bad].abs().amax((1, 2)).min()) > 0
    d = ops.padded_rows(B, T, C, "cuda")
    d.copy_(logits)
    loss, ctx = ops.ctc_loss_fwd(d, tg.cuda(), tl.cuda())
    dl = ops.ctc_loss_bwd(ctx, torch.tensor([15.0], device="cuda"))
    assert_close("ctc loss (ops)", loss, ref.view(1), atol=1e-5, rtol=1e-5)
    assert_close("ctc grad (ops)", dl, gref, atol=2e-6, rtol=1e-4)


@pytest.mark.parametrize("I", [3, 16])
@pytest.mark.parametrize("P", [31, 129])
def test_gate_tail_at_P(ops, P, I):
    B, beta = 37, 1.0
    g = torch.Generator().manual_seed(7 * I + P)
    r, Wr, br = torch.randn(B, P, I, generator=g), torch.randn(P, generator=g) * 0.2, torch.randn(1, generator=g)
    r64, W64, b64 = r.double().requires_grad_(True), Wr.double().requires_grad_(True), br.double().requires_grad_(True)
    s64 = (r64 * W64[None, :, None]).sum(1) + b64
    w64 = torch.softmax(beta * s64, 1)
    s, w = ops.gate_tail_fwd(r.cuda(), Wr.cuda(), br.cuda(), beta)
    assert_close("s", s, s64, atol=1e-5, rtol=1e-5)
    assert_close("w", w, w64, atol=1e-6, rtol=1e-5)
    _, am = ops.gate_tail_fwd(r.cuda(), Wr.cuda(), br.cuda(), beta, hard=True)
    top2 = s64.detach().topk(2, 1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert torch.equal(am.cpu()[clear], s64.detach().argmax(1)[clear])
    dw = torch.randn(B, I, generator=g)
    w64.backward(dw.double())
    dr, dW, db = ops.gate_tail_bwd(w, dw.cuda(), r.cuda(), Wr.cuda(), beta)
    assert_close("dr", dr, r64.grad, atol=1e-6, rtol=1e-4)
    assert_close("dWr", dW, W64.grad, atol=1e-5, rtol=1e-4)
    assert_close("dbr", db, b64.grad, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("I", [3, 16])
@pytest.mark.parametrize("P", [31, 129])
def test_dm_router_at_P(P, I):
    """DMRouterFn (LayerNorms over channels and over the P columns, spatial gating over P * I tokens, channel gating) against the
    float64 oracle -- as tests/test_task_count_gpu.py::test_dm_router_sixteen_experts_vs_float64 at P = 65"""
    from mrn_amd.modules.dm_router import DM_Router
    from oracle import mrn_oracle as O
    C, B = 256, 3
    torch.manual_seed(29 + P + I)
    router = DM_Router(C, 2 * C, P, I)
    sd = {"r." + k: v.detach().clone() for k, v in router.state_dict().items()}
    x = torch.randn(B, I, P, C) * 0.5
    with oracle_dtype(torch.float64) as od:
        sd64 = od.cast(sd)
        for v in sd64.values():
            v.requires_grad_(True)
        x64 = x.double().requires_grad_(True)
        ref = O.dm_router_forward(sd64, "r.", x64)
        dy = torch.randn(B, I, P, C, dtype=torch.float64)
        ref.backward(dy)
    router = router.cuda()
    xd = x.cuda().requires_grad_(True)
    out = router(xd)
    scale = float(ref.detach().abs().max())
    assert_close("DM-Router fwd", out, ref.detach(), atol=1e-4 * scale, rtol=0)
    out.backward(dy.float().cuda())
    for name, a, b in [("dx", xd.grad, x64.grad)] + [(k, router.get_parameter(k[2:]).grad, sd64[k].grad) for k in
                                                      ("r.spatial_gating.proj.weight", "r.channel_gating.proj.weight", "r.proj_1.weight",
                                                       "r.channel_gating.norm.weight")]:
        a, b = a.cpu().double(), b.double()
        l2 = float((a - b).norm() / b.norm())
        assert l2 <= 2e-3, (name, l2)


@pytest.mark.parametrize("H,W", [(32, 128), (64, 512)])
def test_tps_sampler_forward_backward_at_size(ops, H, W):
    """mrn_tps_grid_sample_f32 / _bwd_f32 with inv_delta_C / P_hat built for I_r_size = (H, W): as tests/test_kernels_gpu.py's two TPS
    tests at 32 x 256"""
    from oracle.mrn_oracle import tps_constants
    from mrn_amd.tools.weights import fiducial_bias, smooth_image, uniform
    B = 3
    img = torch.from_numpy(smooth_image("tps_width", (B, 4, H, W), 3))
    cp = (torch.from_numpy(fiducial_bias(20)).view(1, 20, 2) + torch.from_numpy(uniform("cpw", (B, 20, 2), -0.15, 0.15, 1))).requires_grad_(True)
    inv, ph = tps_constants(20, (H, W))
    cz = torch.cat([cp, torch.zeros(B, 3, 2)], 1)
    grid = torch.bmm(ph.repeat(B, 1, 1), torch.bmm(inv.repeat(B, 1, 1), cz)).reshape(B, H, W, 2)
    ref = F.grid_sample(img, grid, padding_mode="border", align_corners=True)
    out, g = ops.tps_grid_sample(ops.nchw_to_nhwc(cu(img)), cu(cp.detach()), cu(inv), cu(ph), (H, W), want_grid=True)
    assert_close("tps grid", g.view(B, H, W, 2), grid.detach(), atol=2e-5)
    assert_close("tps sample", out.permute(0, 3, 1, 2), ref.detach(), atol=5e-4)
    dout = torch.from_numpy(uniform("doutw", (B, 4, H, W), -1, 1, 2))
    ref.backward(dout)
    d = ops.tps_grid_sample_bwd(ops.nchw_to_nhwc(cu(img)), cu(cp.detach()), cu(inv), cu(ph), ops.nchw_to_nhwc(cu(dout)))
    a, b = d.cpu().double().numpy(), cp.grad.double().numpy()
    rel = np.linalg.norm(a - b) / np.linalg.norm(b)
    assert rel < 3e-3, f"d C' relative L2 error {rel:.3e}"


# ---- 2. MRN forward (train + eval) against the oracle ----------------------------------------------------------------------
def oracle_forward_case(kind, imgH, imgW, sd, B=32, seed=5):
    """the fp32 and float64 oracle sides of _mrn_forward_case (host only)"""
    from oracle import mrn_oracle as O
    classes = CLASSES[kind]
    I = len(classes)
    image, tgt, lens = inputs(kind, imgH, imgW, B, classes, seed)
    domain = torch.from_numpy(np.arange(B) % 2)
    cfg = O.Cfg(*CFG[kind], imgH=imgH, imgW=imgW)
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
    sos = torch.LongTensor(B).fill_(2) if attn else None
    with torch.no_grad():
        oe32 = O.mrn_forward({k: v.detach() for k, v in sd32.items()}, cfg, I, image, True, sos, False, training=False)
    with oracle_dtype(torch.float64) as od, torch.no_grad():
        oe64 = O.mrn_forward(od.cast({k: v.detach() for k, v in sd32.items()}), cfg, I, image.double(), True, sos, False,
                             training=False)
    return dict(image=image, tgt=tgt, lens=lens, domain=domain, text_in=text_in, names=names, out32=out32, loss32=loss32, g32=g32,
                out64=out64, sos=sos, oe32=oe32, oe64=oe64)


def _mrn_forward_case(kind, imgH, imgW, B=32, seed=5):
    from mrn_amd import functional as Fn
    from mrn_amd.modules.geometry import frames
    classes = CLASSES[kind]
    opt, net, sd = build_mrn(kind, imgH, imgW, classes, seed)
    assert net.patch == frames(opt.FeatureExtraction, imgW) and net.route.in_features == net.patch
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.")
    o = oracle_forward_case(kind, imgH, imgW, sd, B, seed)
    image, tgt, lens, domain, text_in, names = o["image"], o["tgt"], o["lens"], o["domain"], o["text_in"], o["names"]
    out32, out64, loss32, g32 = o["out32"], o["out64"], o["loss32"], o["g32"]
    attn = kind == "trba"
    w32, l32 = out32["index"].detach(), out32["logits"].detach()
    band_w = float((w32.double() - out64["index"]).abs().max())
    band_l = float((l32.double() - out64["logits"]).abs().max())
    with torch.no_grad():
        handle = net.experts_prefetch(image.cuda(), None if text_in is None else text_in.cuda(), True)
    assert handle is not None
    assert handle["feats"].shape == (B, net.patch, len(classes), 256)
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
    print(f"[width {kind} {imgH}x{imgW}] weights err {ew:.3e} (f32-f64 {band_w:.3e}), logits err {el:.3e} (f32-f64 {band_l:.3e}, "
          f"scale {scale_l:.3e}), loss {float(loss.detach()):.6f} vs {float(loss32.detach()):.6f}")
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
    oe32, oe64, sos = o["oe32"], o["oe64"], o["sos"]
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
@pytest.mark.parametrize("imgH,imgW", GEOMETRIES)
def test_mrn3_batch32_vs_oracle(kind, imgH, imgW):
    _mrn_forward_case(kind, imgH, imgW)


@pytest.mark.parametrize("kind", ["crnn", "trba"])
@pytest.mark.parametrize("imgH,imgW", GEOMETRIES)
def test_mrn2_vs_reference_fixture(kind, imgH, imgW):
    """the reference's own outputs (tests/golden/width.npz, B = 4, two experts), with the band of
    tests/test_geometry_gpu.py::test_mrn2_vs_reference_fixture: 1e-4, or for TRBA 3x the distance of the reference's fp32 result from
    float64 arithmetic on the same quantity"""
    from mrn_amd.modules.model import MRNNet
    from oracle import mrn_oracle as O
    from tests.helpers import load_golden, sub
    from tests.test_width_cpu import WIDTH_CASES, _width_state_dict, _width_targets
    g = load_golden("width")
    p = f"{kind}{imgH}x{imgW}/"
    stages, classes, seed = WIDTH_CASES[kind]
    attn = kind == "trba"
    opt = make_opt(kind, imgH, imgW)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
    image, tgt, _ = _width_targets(kind, imgH, imgW, classes, seed)
    text = tgt[:, :-1] if attn else None
    ref64 = {}
    if attn:
        cfg = O.Cfg(*stages, imgH=imgH, imgW=imgW)
        with oracle_dtype(torch.float64) as od, torch.no_grad():
            sd = od.cast(_width_state_dict(g, p, seed))
            fm = O.resnet_forward(sd, "model.0.model.FeatureExtraction.",
                                  O.tps_forward(sd, "model.0.model.Transformation.", image.double(), True), True)
            ref64["visual"] = fm.permute(0, 2, 3, 1).mean(1)
            ob = O.mrn_forward(od.cast(_width_state_dict(g, p, seed)), cfg, 2, image.double(), True, text, True, training=True)
            ref64["stepB/weights"], ref64["stepB/logits"] = ob["index"], ob["logits"]
            ref64["stepA/logits"] = O.mrn_forward(od.cast(_width_state_dict(g, p, seed)), cfg, 2, image.double(), False, text, True,
                                                  training=True)["logits"]

    def check(name, t, full=False):
        mine = (t.detach().cpu().double().numpy() if full else sub(t)[0].astype(np.float64))
        ref = g[p + name] if full else g[p + name + "/sub"].astype(np.float64)
        tol = 1e-4 + 1e-4 * np.abs(ref).max()
        if name in ref64:
            r64 = ref64[name].numpy() if full else sub(ref64[name])[0].astype(np.float64)
            tol = max(tol, 3 * np.abs(ref - r64).max())
        err = np.abs(mine - ref).max()
        print(f"[width fixture {kind} {imgH}x{imgW}] {name}: max abs err {err:.3e}, tol {tol:.3e}")
        assert err <= tol, f"{name}: max abs err {err:.3e} > tol {tol:.3e}"

    net.load_state_dict(_width_state_dict(g, p, seed), strict=True)
    net = net.cuda().train()
    with torch.no_grad():
        check("visual", net.model[0].model.visual(image.cuda()))
        net.load_state_dict(_width_state_dict(g, p, seed), strict=True)
        out = net(image.cuda(), True, None if text is None else text.cuda(), True)
        check("stepB/weights", out["index"], full=True)
        check("stepB/logits", out["logits"])
        assert np.array_equal(out["index"].cpu().numpy().argmax(1), g[p + "stepB/weights"].argmax(1))
        net.load_state_dict(_width_state_dict(g, p, seed), strict=True)
        check("stepA/logits", net(image.cuda(), False, None if text is None else text.cuda())["logits"])
        net.load_state_dict(_width_state_dict(g, p, seed), strict=True)
        net.eval()
        oe = net(image.cuda(), True, torch.LongTensor(4).fill_(2).cuda() if attn else None, False)
    assert np.array_equal(oe["index"].cpu().numpy(), g[p + "eval/index"])
    if not attn:
        check("eval/logits", oe["logits"])
    assert float((oe["logits"].max(2)[1].cpu().numpy() == g[p + "eval/argmax"]).mean()) >= 0.99


def test_expert_forward_takes_the_kernel_forms_of_256():
    """the frozen experts' lock-step forward at 32 x 128 and 32 x 512 calls the entry points it calls at 32 x 256 -- no layer leaves the
    row-block Winograd kernel, the patch-resident kernel or the grouped decoder for another form -- and every row-block query
    (mrn_conv2d_x3_wino_rows) answers as at 256"""
    seen = {}
    for kind in ("trba", "crnn"):
        for imgW in (256, 128, 512):
            opt, net, sd = build_mrn(kind, 32, imgW, CLASSES[kind], 7)
            net.train()
            image, tgt, _ = inputs(kind, 32, imgW, 8, CLASSES[kind], 7)
            text_in = tgt[:, :-1].cuda() if kind == "trba" else None
            with torch.no_grad(), recorded_calls() as log:
                out = net(image.cuda(), True, text_in, True)
                torch.cuda.synchronize()
            assert torch.isfinite(out["logits"]).all()
            names = sorted({n for n, _ in log})
            rows = [rc for n, rc in log if n == "mrn_conv2d_x3_wino_rows"]
            seen[(kind, imgW)] = (names, rows)
            del net
        assert any(n.startswith("mrn_conv2d_x3_wino") for n in seen[(kind, 256)][0])
        for imgW in (128, 512):
            assert seen[(kind, imgW)][0] == seen[(kind, 256)][0], (kind, imgW, set(seen[(kind, imgW)][0]) ^ set(seen[(kind, 256)][0]))
            assert seen[(kind, imgW)][1] == seen[(kind, 256)][1], (kind, imgW)


# ---- 3. loop A: an expert's parameter gradients ----------------------------------------------------------------------------
def test_loop_a_crnn_gradients_vs_oracle_32x128():
    from mrn_amd import functional as Fn
    from oracle import mrn_oracle as O
    opt, net, sd = build_mrn("crnn", 32, 128, (40,), 11)
    image, labels, lens = inputs("crnn", 32, 128, 3, (40,), 11)
    names = [n for n, p in net.named_parameters() if n.startswith("model.0.")]
    params = [sd[n].requires_grad_(True) for n in names]
    cfg = O.Cfg(*CFG["crnn"], imgH=32, imgW=128)
    ref_out = O.model_forward(sd, "model.0.", cfg, image, None, True, training=True)["predict"]
    assert ref_out.shape[1] == 31
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


def _oracle_trba_grads(sd0, image, labels_index, dtype, imgH, imgW, bml=25):
    from oracle import mrn_oracle as O
    sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    names = [k for k in sd if k.startswith("model.0.") and sd[k].is_floating_point() and "running" not in k
             and "generator" not in k]
    params = [sd[n].requires_grad_(True) for n in names]
    for k in list(sd):               # Prediction.generator.* aliases fc.*
        if k.startswith("model.0.Prediction.generator."):
            sd[k] = sd[k.replace("Prediction.generator.", "fc.")]
    cfg = O.Cfg(*CFG["trba"], imgH=imgH, imgW=imgW, batch_max_length=bml)
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


def test_loop_a_trba_gradients_vs_oracle_32x512(bml=25, B=3):
    """as tests/test_geometry_gpu.py::test_loop_a_trba_gradients_vs_oracle_64 (B = 3): judged against the float64 oracle, at least as
    close to it as 3x the reference's own fp32 arithmetic, floor 2e-3"""
    from mrn_amd import functional as Fn
    opt, net, sd = build_mrn("trba", 32, 512, (41,), 12, bml)
    image, text, _ = inputs("trba", 32, 512, B, (41,), 12, bml)
    names, g32, out32, loss32 = _oracle_trba_grads(sd, image, text, torch.float32, 32, 512, bml)
    _, g64, _, _ = _oracle_trba_grads(sd, image, text, torch.float64, 32, 512, bml)
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


# ---- 4. loop B: two router steps at 48 x 320 -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["crnn", "trba"])
def test_loop_b_two_steps_vs_oracle_48x320(kind, imgH=48, imgW=320, classes=None, bml=25, f64_yardstick=False):
    """f64_yardstick: the float64 oracle takes the same two steps next to the fp32 one.  A gradient or an Adam step on which the fp32
    oracle is itself further from the float64 oracle than the band is judged against float64 instead, at 3x that distance (the rule of
    tests/test_model_gpu.py::test_loop_a_trba_gradients_vs_oracle).  The first Adam step is lr * g / |g|, so an element whose gradient
    is round-off sized takes a step of either sign, and the trajectories enter the second step with different weights."""
    from mrn_amd import functional as Fn
    from mrn_amd.optim import FlatAdam
    from oracle import mrn_oracle as O
    classes = classes or CLASSES[kind]
    I, B = len(classes), 8
    opt, net, sd = build_mrn(kind, imgH, imgW, classes, 13, bml)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.")
    tr_names = [n for n, p in net.named_parameters() if p.requires_grad]
    adam = FlatAdam([p for n, p in net.named_parameters() if p.requires_grad], lr=5e-4)
    cfg = O.Cfg(*CFG[kind], imgH=imgH, imgW=imgW, batch_max_length=bml)
    attn = kind == "trba"
    sd_ref = {k: v.clone() for k, v in sd.items()}
    state = [{"m": torch.zeros_like(sd_ref[n]), "v": torch.zeros_like(sd_ref[n])} for n in tr_names]
    if f64_yardstick:
        sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        state64 = [{"m": torch.zeros_like(sd64[n]), "v": torch.zeros_like(sd64[n])} for n in tr_names]

    def dist(a, b):
        a, b = a.detach().cpu().double().numpy(), b.detach().double().numpy()
        return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12), np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)

    for step in (1, 2):
        image, tgt, lens = inputs(kind, imgH, imgW, B, classes, 100 + step, bml)
        domain = torch.from_numpy(np.arange(B) % I)
        text_in = tgt[:, :-1] if attn else None
        g64, d64 = None, None
        if f64_yardstick:
            with oracle_dtype(torch.float64):
                p64 = [sd64[n].requires_grad_(True) for n in tr_names]
                o64 = O.mrn_forward(sd64, cfg, I, image.double(), True, text_in, True, training=True)
                c64 = O.attn_ce_loss(o64["logits"], tgt) if attn else O.ctc_loss(o64["logits"], tgt, lens)
                g64 = torch.autograd.grad(15 * c64 + F.cross_entropy(o64["index"], domain), p64)
                for p in p64:
                    p.requires_grad_(False)
                b64 = [p.clone() for p in p64]
                with torch.no_grad():
                    O.clip_and_adam(p64, g64, state64, 5e-4, step)
                d64 = [p - b for p, b in zip(p64, b64)]
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
        rel_l2, rel_max = (2e-3, 1e-2) if not attn else (5e-3, 2.5e-2)
        for i, (n, gr) in enumerate(zip(tr_names, ref_grads)):
            if n == "route.bias":
                continue
            if g64 is not None:
                l2_ref, mx_ref = dist(gr, g64[i])
                if l2_ref > rel_l2 or mx_ref > rel_max:
                    l2, mx = dist(mine[n].grad, g64[i])
                    assert l2 <= 3.0 * l2_ref and mx <= 3.0 * mx_ref, \
                        f"step {step} {n}: HIP vs f64 {l2:.2e} / {mx:.2e}, torch-f32 vs f64 {l2_ref:.2e} / {mx_ref:.2e}"
                    continue
            _grad_check(f"step {step} {n}", mine[n].grad, gr, rel_l2=rel_l2, rel_max=rel_max)
        mine_before = {n: mine[n].detach().cpu().clone() for n in tr_names}
        adam.step(lr=5e-4, max_norm=5.0)
        for i, (n, gr) in enumerate(zip(tr_names, ref_grads)):
            if n == "route.bias":
                continue          # (a round-off gradient's Adam step has a random sign)
            d_ref = sd_ref[n] - before[n]
            d_mine = mine[n].detach().cpu() - mine_before[n]
            if d64 is not None:
                rel_ref = float((d_ref.double() - d64[i]).norm() / d64[i].norm().clamp_min(1e-30))
                if rel_ref > 5e-2:
                    rel = float((d_mine.double() - d64[i]).norm() / d64[i].norm().clamp_min(1e-30))
                    assert rel <= 3.0 * rel_ref, (step, n, rel, rel_ref)
                    continue
            rel = float((d_mine - d_ref).norm() / d_ref.norm().clamp_min(1e-30))
            assert rel <= 5e-2, (step, n, rel)


# ---- 5. DER: one step at 32 x 384 -------------------------------------------------------------------------------------------
def test_dernet_step_vs_oracle_32x384(kind="crnn", imgW=384, classes=(40, 70), bml=25, frames=95):
    """kind="trba": a gradient on which the fp32 oracle itself is further than the band (2e-3 relative L2, 1e-2 of the maximum) from the
    float64 oracle is judged against float64 at 3x that distance instead.  Measured on the host for nine extractors at 32 x 512,
    batch_max_length 120, B = 8: the fp32 oracle is 2.9e-2 .. 4.4e-2 (L2) from float64 on the newest extractor's TPS localisation network
    and 4e-3 .. 2.7e-2 on its ResNet, while features / logits agree to 8.8e-5 / 4.7e-6"""
    from mrn_amd import functional as Fn
    from mrn_amd.modules.model import DERNet
    from mrn_amd.tools import weights as W
    from oracle import mrn_oracle as O
    opt = make_opt(kind, 32, imgW, bml)
    B, attn, last = 8, kind == "trba", f"model.{len(classes) - 1}."
    with contextlib.redirect_stdout(io.StringIO()):
        net = DERNet(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
            net.build_aux_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed=17)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().train()
    for ext in list(net.model)[:-1]:
        ext.eval()                                              # DER's model_eval_and_train: the old extractors in eval mode, frozen
    for n, p in net.named_parameters():
        p.requires_grad = n.startswith(last) or not n.startswith("model.")
    image, labels, lens = inputs(kind, 32, imgW, B, classes, 17, bml)
    text_in = labels[:, :-1] if attn else None
    cfg = O.Cfg(*CFG[kind], imgH=32, imgW=imgW, batch_max_length=bml)
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    params = [sd[n].requires_grad_(True) for n in names]
    ref = O.dernet_forward(sd, cfg, len(classes), image, text_in, True, training=True)
    assert ref["features"].shape[1] == frames
    ref_loss = O.attn_ce_loss(ref["logits"], labels) if attn else O.ctc_loss(ref["logits"], labels, lens)
    ref_grads = torch.autograd.grad(ref_loss, params, allow_unused=True)      # (the attention heads are unused by CTC)
    g64 = None
    if attn:                                                    # TPS: the conditioning yardstick, as the TRBA loop-A tests
        with oracle_dtype(torch.float64) as od:
            sd64 = od.cast({k: v.detach() for k, v in sd.items()})
            p64 = [sd64[n].requires_grad_(True) for n in names]
            r64 = O.dernet_forward(sd64, cfg, len(classes), image.double(), text_in, True, training=True)
            g64 = torch.autograd.grad(O.attn_ce_loss(r64["logits"], labels), p64, allow_unused=True)
    out = net(image.cuda(), text_in.cuda()) if attn else net(image.cuda())
    assert_close("DER features", out["features"], ref["features"], atol=1e-4)
    assert_close("DER logits", out["logits"], ref["logits"], atol=1e-4)
    assert_close("DER aux logits", out["aux_logits"], ref["aux_logits"], atol=1e-4)
    loss = Fn.cross_entropy(out["logits"], labels[:, 1:].cuda(), 1) if attn else Fn.ctc_loss(out["logits"], labels.cuda(), lens.cuda())
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * max(1.0, abs(ref_loss.item()))
    loss.backward()
    mine = dict(net.named_parameters())
    def dist(a, b):
        a, b = a.detach().cpu().double().numpy(), b.detach().double().numpy()
        return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12), np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)

    for i, (n, rg) in enumerate(zip(names, ref_grads)):
        if rg is None or rg.abs().max() < 1e-9:
            continue
        if g64 is not None:
            l2_ref, mx_ref = dist(rg, g64[i])
            if l2_ref > 2e-3 or mx_ref > 1e-2:
                # the fp32 oracle itself misses the band against float64 here (a gradient through the TPS grid): judged against float64,
                # at most 3x as far from it as the fp32 oracle (the rule of tests/test_model_gpu.py::test_loop_a_trba_gradients_vs_oracle)
                l2, mx = dist(mine[n].grad, g64[i])
                assert l2 <= 3.0 * l2_ref and mx <= 3.0 * mx_ref, f"{n}: HIP vs f64 {l2:.2e} / {mx:.2e}, torch-f32 vs f64 {l2_ref:.2e} / {mx_ref:.2e}"
                continue
        _grad_check(n, mine[n].grad, rg, rel_l2=2e-3, rel_max=1e-2)


# ---- 6. reduced mode (at 48 x 320 the 6-row maps have no plain-fp16 Winograd form and fall back, as at 48 x 256) ---------
@pytest.mark.parametrize("kind", ["crnn", "trba"])
@pytest.mark.parametrize("imgH,imgW", [(32, 128), (48, 320)])
def test_reduced_mode_loop_b(kind, imgH, imgW, classes=None):
    from mrn_amd import ops
    classes = classes or CLASSES[kind]
    B = 8
    opt, net, sd = build_mrn(kind, imgH, imgW, classes, 19)
    net.train()
    image, tgt, _ = inputs(kind, imgH, imgW, B, classes, 19)
    text_in = tgt[:, :-1].cuda() if kind == "trba" else None
    with torch.no_grad():
        ref = net(image.cuda(), True, text_in, True)
    saved = ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS
    try:
        ops.X3_PRODUCTS = ops.TRAIN_PRODUCTS = 1            # bench.py --precision fp16
        assert ops.wino_eligible((3, 3), (1, 1), (1, 1), 512, 512, H=4) and not ops.wino_eligible((3, 3), (1, 1), (1, 1), 512, 512, H=6)
        net.load_state_dict(sd, strict=True)                # (the same running statistics before the step)
        with torch.no_grad(), recorded_calls() as log:
            out = net(image.cuda(), True, text_in, True)
        torch.cuda.synchronize()
    finally:
        ops.X3_PRODUCTS, ops.TRAIN_PRODUCTS = saved
    d16 = sum(n == "mrn_conv2d_x3_wino_d16" for n, _ in log)
    assert d16 > 0                                          # the plain-fp16 row-block form ran on the 4k-row maps ...
    if imgH == 48 and kind == "trba":
        assert any(n == "mrn_conv2d_x3_hl32" for n, _ in log)
    w, w0 = out["index"].cpu(), ref["index"].cpu()
    lg, lg0 = out["logits"].cpu(), ref["logits"].cpu()
    err_w = float((w - w0).abs().max())
    err_l = float((lg - lg0).abs().max()) / max(float(lg0.abs().max()), 1e-6)
    assert torch.isfinite(lg).all()
    assert err_w <= 2e-2 and err_l <= 5e-2, (err_w, err_l)
    assert err_w > 1e-7 or err_l > 1e-7                     # the reduced arithmetic really ran


# ---- 7. the largest supported sizes and the per-call pixel budget ---------------------------------------------------------------
@pytest.mark.parametrize("imgH,B", [(32, 256), (64, 128)])
def test_full_size_trba6_loop_b_512(imgH, B):
    from mrn_amd import functional as Fn
    from mrn_amd.modules.expert_group import BackboneGroup
    from mrn_amd.tools import weights as W
    classes = (41, 51, 61, 71, 81, 98)
    opt, net, sd = build_mrn("trba", imgH, 512, classes, 23)
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad = not n.startswith("model.")
    image = torch.from_numpy(W.uniform("width_full", (B, 4, imgH, 512), -1.0, 1.0, 23)).cuda()
    text = torch.from_numpy(W.randint("width_full_text", (B, 27), 4, classes[-1], 23)).cuda()
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
        full = grp.visual_all(image)                        # [6, B, 129, 512]
        part = grp.visual_all(image[:8].contiguous())
    assert full.shape == (6, B, 129, 512)
    assert_close("first 8 rows of the full batch vs B = 8", full[:, :8], part, atol=1e-4)
    assert torch.isfinite(full).all()


def test_call_over_the_pixel_budget_is_refused_before_any_launch():
    from mrn_amd.modules.expert_group import BackboneGroup
    from mrn_amd.modules.model import DERNet
    opt, net, sd = build_mrn("trba", 64, 512, (41, 51), 3)
    image = torch.zeros(256, 4, 64, 512, device="cuda")
    text = torch.full((256, 26), 2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    match = r"4194304.*B = 256 at 64 x 512"
    with recorded_calls() as log:
        net.train()
        with torch.no_grad(), pytest.raises(NotImplementedError, match=match):
            net(image, True, text, True)
        with torch.no_grad(), pytest.raises(NotImplementedError, match=match):
            net.experts_prefetch(image, text, True)
        with torch.no_grad(), pytest.raises(NotImplementedError, match=match):
            net(image, False, text, True)                   # loop A: the newest expert alone
        net.eval()
        with torch.no_grad(), pytest.raises(NotImplementedError, match=match):
            net(image, True, text[:, 0].contiguous(), False)
        with torch.no_grad(), pytest.raises(NotImplementedError, match=match):
            BackboneGroup([m.model for m in net.model]).visual_all(image)
    assert log == []
    with contextlib.redirect_stdout(io.StringIO()):
        der = DERNet(make_opt("crnn", 64, 512))
        for c in (40, 70):
            der.update_fc(256, c)
            der.build_prediction(der.opt, c)
            der.build_aux_prediction(der.opt, c)
    der = der.cuda().eval()
    with recorded_calls() as log, torch.no_grad(), pytest.raises(NotImplementedError, match=match):
        der(image)
    assert log == []
    with torch.no_grad():                                   # B = 128 is inside the budget (test_full_size_trba6_loop_b_512 runs it in full)
        from mrn_amd.modules.geometry import check_call
        check_call("TPS", "ResNet", 128, 64, 512)


# ---- 8. widths outside the supported set -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["crnn", "trba"])
@pytest.mark.parametrize("imgW", [100, 576])
def test_unsupported_width_is_refused(kind, imgW):
    from mrn_amd.modules.model import Model
    opt = make_opt(kind, 32, imgW)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Model(opt)
        net.update_fc(opt.hidden_size, 41)
        net.build_prediction(opt, 41)
    net = net.cuda().eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=WIDTH_SET):
        net.model.visual(torch.zeros(2, 4, 32, imgW, device="cuda"))
    _, mrn, _ = build_mrn(kind, 32, imgW, (41, 51), 3)
    mrn.eval()
    sos = torch.LongTensor(2).fill_(2).cuda() if kind == "trba" else None
    with torch.no_grad(), pytest.raises(NotImplementedError, match=WIDTH_SET):
        mrn(torch.zeros(2, 4, 32, imgW, device="cuda"), True, sos, False)
    mrn.train()
    text = torch.full((2, 26), 2, dtype=torch.int64, device="cuda") if kind == "trba" else None
    with torch.no_grad(), pytest.raises(NotImplementedError, match=WIDTH_SET):
        mrn(torch.zeros(2, 4, 32, imgW, device="cuda"), True, text, True)


def test_svtr_at_another_width_is_refused():
    from mrn_amd.modules.model import Model
    o = make_opt("crnn", 32, 128)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = "None", "SVTR", "None", "CTC"
    with contextlib.redirect_stdout(io.StringIO()):
        net = Model(o)
        net.update_fc(o.hidden_size, 41)
        net.build_prediction(o, 41)
    net = net.cuda().eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=WIDTH_SET) as e:
        net.model.visual(torch.zeros(2, 4, 32, 128, device="cuda"))
    assert "32 x 256 only" in str(e.value)


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------
def test_tiny_train_one_task_at_32x128(tmp_path):
    from torch.utils.data import ConcatDataset
    from mrn_amd import tiny_train
    from mrn_amd.data.data_manage import Dataset_Manager, Val_Dataset
    from mrn_amd.data.dataset import ArrayDataset
    from tests.helpers import fake_text_samples
    os.chdir(tmp_path)
    opt = types.SimpleNamespace(
        exp_name="t", il="mrn", memory="random", memory_num=20, batch_max_length=25, imgH=32, imgW=128, manual_seed=111,
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
    assert learner.model.patch == 31
    assert all(torch.isfinite(p).all() for p in learner.model.parameters())


@pytest.mark.parametrize("imgW", [128, 384])
def test_device_stager_and_augmentation_at_width(imgW):
    """the device stager with Aug=Blur/Crop/Rot (mrn_aug_* kernels resizing to another target width) hands out the batches the host
    (PIL) path does, bit for bit -- tests/test_data_augment_gpu.py::test_dataset_manager_device_batches_equal_host at 256"""
    from tests.test_data_augment_gpu import _manager_batches
    from tests.test_data_cpu import make_opt as data_opt
    aug = "Blur5-Crop90-Rot15"
    host, dm_h = _manager_batches(data_opt(Aug=aug, imgW=imgW, device_prefetch=False), False)
    dev, dm_d = _manager_batches(data_opt(Aug=aug, imgW=imgW, device_prefetch=True), False)
    assert dm_h.stager.stream is None and dm_d.stager.stream is not None
    for h, d in zip(host, dev):
        assert h[0].shape == d[0].shape and h[0].shape[1:] == (4, 32, imgW)
        assert torch.equal(h[0].view(torch.int32), d[0].view(torch.int32))
        assert list(h[1]) == list(d[1])


def test_checkpoint_round_trip_at_32x384(tmp_path):
    opt, net, sd = build_mrn("trba", 32, 384, CLASSES["trba"], 29)
    image, _, _ = inputs("trba", 32, 384, 4, CLASSES["trba"], 29)
    sos = torch.LongTensor(4).fill_(2).cuda()
    net.eval()
    with torch.no_grad():
        a = net(image.cuda(), True, sos, False)["logits"].cpu()
    path = os.path.join(str(tmp_path), "width384.pth")
    torch.save(net.state_dict(), path)
    state = torch.load(path)
    assert state["route.weight"].shape == (1, 97) and state["dm_router.0.spatial_gating.proj.weight"].shape == (97 * 3, 97 * 3)
    _, net2, _ = build_mrn("trba", 32, 384, CLASSES["trba"], 30)
    net2.load_state_dict(state, strict=True)
    net2.eval()
    with torch.no_grad():
        b = net2(image.cuda(), True, sos, False)["logits"].cpu()
    assert torch.equal(a, b)
    _, net3, _ = build_mrn("trba", 32, 256, CLASSES["trba"], 30)       # a 256-pixel net does not take it: the token axes differ
    with pytest.raises(RuntimeError, match="size mismatch"):
        net3.load_state_dict(state, strict=True)
