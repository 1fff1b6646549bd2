"""Where input width, task count and label length meet, on the GPU.  Every launcher rule that reads two or three of these numbers
at once is run on both sides of its boundary, and each test first states -- from ops.attn_decoder_whole_context, the library's own
mrn_attn_decoder_bwd_steps_per_launch, the recorded entry-point names or the sub-group sizes -- which path it is about to take:

  1. kernels against float64 / torch on the host: the attention decoder forward + BPTT over the (D, T) plane (single-launch vs
     1024-column chunks), the forced-chunk equivalence at the tightest single-launch tile (D = 1792, T = 129), the deferred dHb /
     dHproj sums over the (T, S) plane (one, two and three launches; behind the chunked forward), the long CTC kernel at T = 31 and
     T = 127 around the feasibility edge (the grouped SVTR kernels at G = 4 / 5 are rows of tests/test_kernels_gpu.py);
  2. the HIP nets against the reference fixture of the crossings (tests/golden/cross_axes.npz);
  3. whole nets against the CPU oracle beyond B = 2: SVTR past six experts (uneven lock-step sub-groups), TRBA loop A at 32 x 512
     with 121 decoder steps, loop B over ten CRNN experts at 32 x 512 with labels up to 100 and nine TRBA experts at 64 x 128, a DER
     step over nine TRBA extractors at 32 x 512 with labels of 120, reduced mode at one crossing, and the driver over seven SVTR tasks.

Every band is the named mould's, unchanged."""
import contextlib
import io
import os
import types

import pytest
import torch

from tests.helpers import assert_close
from tests.test_cross_axes_cpu import CASES, MRN_KEYS, STAGES, cross_cfg, cross_masks, cross_targets
from tests.test_kernels_gpu import ops, rnd  # noqa: F401  (ops: the module-scoped fixture that loads the library)
from tests.test_width_gpu import recorded_calls

pytestmark = pytest.mark.gpu

CRNN10 = tuple(40 + 6 * i + (i % 3) for i in range(10))
TRBA9 = tuple(41 + 6 * i + (i % 2) for i in range(9))
SVTR_BENCH10 = (2090, 2310, 4038, 5198, 5271, 5373, 5480, 5590, 5710, 5835)


def steps_per_launch(T):
    from mrn_amd._lib import call
    return int(call("mrn_attn_decoder_bwd_steps_per_launch", T))


# ---- 1. kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("D,T,whole", [(1792, 129, True), (2048, 129, False), (4096, 129, False), (2048, 33, False), (4096, 33, False),
                                       (1792, 33, True)])
def test_decoder_fwd_bwd_over_the_d_t_plane(ops, D, T, whole, x3, monkeypatch):
    """tests/test_task_count_gpu.py::test_wide_decoder_fwd_bwd_vs_float64 (float64 oracle: forward, dH, dW_ih, dW_i2h, greedy rows;
    its bands) at the largest single-launch tile (D = 1792 at T = 129: 158 528 B of the 163 840 B budget in the x3 form) and in the
    chunked form at T = 129 and T = 33, with the recurrent products as split-fp16 x3 and in exact fp32"""
    from tests.test_task_count_gpu import test_wide_decoder_fwd_bwd_vs_float64
    for form in (True, False):
        assert ops.attn_decoder_whole_context(D, T, form) is whole
    monkeypatch.setattr(ops, "DECODER_X3", x3)
    test_wide_decoder_fwd_bwd_vs_float64(D, T)


@pytest.mark.parametrize("x3", ["1", "0"])
@pytest.mark.parametrize("D,T", [(1792, 129), (256, 33)])
def test_forced_chunk_equals_single_launch_at_the_tight_corner(ops, D, T, x3, monkeypatch):
    """tests/test_task_count_gpu.py::test_wide_decoder_equals_single_launch_where_it_fits at the tightest tile the single launch takes"""
    from tests.test_task_count_gpu import test_wide_decoder_equals_single_launch_where_it_fits
    assert ops.attn_decoder_whole_context(D, T, x3 == "1")
    test_wide_decoder_equals_single_launch_where_it_fits(D, x3, monkeypatch, T=T)


@pytest.mark.parametrize("T,S,D,B,launches", [(129, 106, 256, 5, 1), (129, 107, 256, 5, 2), (129, 230, 256, 4, 3), (65, 256, 256, 4, 3),
                                              (33, 141, 256, 5, 1), (33, 142, 256, 5, 2), (129, 107, 2304, 3, 2)])
def test_decoder_backward_step_chunks_over_the_t_s_plane(ops, T, S, D, B, launches):
    """tests/test_long_labels_gpu.py::test_attention_decoder_backward_long (its bands) on both sides of the deferred sums' launch
    boundary at T = 129 and T = 33, with three launches (the accumulating launch taken twice) at T = 129 and T = 65, and with two
    launches behind the chunked forward (D = 2304).  The number of launches is taken from the launcher's own steps-per-launch."""
    from tests.test_long_labels_gpu import test_attention_decoder_backward_long
    fit = steps_per_launch(T)
    assert fit == (160 * 1024) // (4 * (T + 256))
    assert -(-S // fit) == launches, (S, fit)
    assert ops.attn_decoder_whole_context(D, T) is (D <= 1792)
    test_attention_decoder_backward_long(B, D, S, T=T)


def _edge_lengths(T, W):
    """18 label lengths for tests/test_width_gpu.py::_labels_with_repeats, whose row b aims at L + repeats = T + (-1, 1, 0, 3, -6, 2)
    [b % 6]: twelve rows of two lengths near the edge, then L = 0, one over the edge, L = T (no repeat: feasible), the full width,
    L = 1 and the edge plus two"""
    la, lb = min(W, T - 8), min(W, (T + 12) // 2)
    return [la, lb] * 6 + [0, min(W, T + 1), min(W, T), W, 1, min(W, T)]


@pytest.mark.parametrize("W", [40, 100, 127, 255])
@pytest.mark.parametrize("T", [31, 127])
def test_long_ctc_around_the_feasibility_edge(ops, T, W):
    """the long CTC kernel at the frame counts of the 128- and 512-pixel VGG lines: L = 0, L = T, L + repeats = T - 1, T (feasible),
    T + 1 and beyond, L > T (no alignment), against torch.nn.CTCLoss(zero_infinity=True) in float64 at the bands of
    tests/test_long_labels_gpu.py::test_long_ctc_vs_torch.  Where 2 W - 1 <= T (W = 40 at T = 127) no label reaches the edge and
    every row is feasible."""
    from tests.test_long_labels_gpu import torch_ctc
    from tests.test_width_gpu import _labels_with_repeats
    C = 97
    lengths = _edge_lengths(T, W)
    B = len(lengths)
    logits = rnd(B, T, C, seed=T + W, scale=3.0)
    tg, tl, need = _labels_with_repeats(B, T, C, seed=T * W, W=W, lengths=lengths)
    assert tl.tolist() == lengths and int(tl.max()) <= W
    lp = logits.double().log_softmax(2).permute(1, 0, 2)
    per = torch.nn.CTCLoss(reduction="none")(lp, tg, torch.full((B,), T, dtype=torch.int32), tl)
    bad = torch.isinf(per)
    assert bad.tolist() == [n > T for n in need]
    if 2 * W - 1 > T:
        assert B // 4 <= int(bad.sum()) <= 3 * B // 4, int(bad.sum())
        assert T - 1 in need and T in need and T + 1 in need
    else:
        assert int(bad.sum()) == 0
    ref, gref = torch_ctc(logits, tg, tl)
    assert torch.isfinite(ref) and float(ref) > 0
    d = ops.padded_rows(B, T, C, "cuda")
    d.copy_(logits)
    with recorded_calls() as log:
        loss, ctx = ops.ctc_loss_fwd(d, tg.cuda(), tl.cuda())
        dl = ops.ctc_loss_bwd(ctx, torch.tensor([15.0], device="cuda"))
    assert [n for n, _ in log if "ctc_loss" in n] == ["mrn_ctc_loss_fwd_long_f32", "mrn_ctc_loss_bwd_long_f32"]
    assert_close("long ctc loss", loss, ref.view(1), atol=1e-5, rtol=1e-5)
    assert_close("long ctc grad", dl, gref, atol=2e-6, rtol=1e-4)
    nll, dl = ctx[4].cpu(), dl.cpu()
    assert torch.isinf(nll[bad]).all() and torch.isfinite(nll[~bad]).all()
    if bad.any():
        assert float(dl[bad].abs().max()) == 0.0
    assert float(dl[~bad].abs().amax((1, 2)).min()) > 0


def test_long_ctc_full_batch_at_T127(ops):
    """tests/test_long_labels_gpu.py::test_long_ctc_vs_torch_full_batch (B = 256, C = 4998) at T = 127 with labels up to 127"""
    from tests.test_long_labels_gpu import test_long_ctc_vs_torch_full_batch
    with recorded_calls() as log:
        test_long_ctc_vs_torch_full_batch(127, W=127)
    assert "mrn_ctc_loss_fwd_long_f32" in [n for n, _ in log]


# ---- 2. the HIP nets against the reference fixture of the crossings -----------------------------------------------------------
def _fixture_case(key):
    from tests.test_task_count_gpu import make_opt
    kind, classes, imgH, imgW, bml, seed = CASES[key]
    return {"golden": "cross_axes", "prefix": key + "/", "classes": classes, "seed": seed, "targets": cross_targets(key),
            "opt": make_opt(kind, imgH, imgW, bml, stages=STAGES[kind]), "cfg": cross_cfg(key), "masks": cross_masks(key)}


@pytest.mark.parametrize("key", MRN_KEYS)
def test_mrn10_at_the_crossings_vs_reference_fixture(key):
    """tests/test_task_count_gpu.py::test_mrn10_vs_reference_fixture (its bands) on ten SVTR experts (sub-groups 3 + 3 + 4), ten
    CRNN experts at 32 x 512 under the long CTC loss, and ten TRBA experts at 64 x 128; the 16-wide router behind each"""
    from tests.test_task_count_gpu import test_mrn10_vs_reference_fixture
    with recorded_calls() as log:
        test_mrn10_vs_reference_fixture(CASES[key][0], case=_fixture_case(key))
    names = {n for n, _ in log}
    assert {"mrn_fanin_fwd_wide_f32", "mrn_gate_tail_fwd_wide_f32", "mrn_gate_tail_bwd_wide_f32"} <= names
    assert ("mrn_ctc_loss_fwd_long_f32" in names) == (key == "mrn_crnn10_w512_l100")


def test_dernet9_w512_l120_step_vs_reference_fixture(ops):
    """tests/test_task_count_gpu.py::test_dernet9_step_vs_reference_fixture (its bands) at D = 2304, T = 129, S = 121: the chunked
    forward and two launches of each deferred sum"""
    from tests.test_task_count_gpu import test_dernet9_step_vs_reference_fixture
    assert not ops.attn_decoder_whole_context(2304, 129) and steps_per_launch(129) < 121 <= 2 * steps_per_launch(129)
    test_dernet9_step_vs_reference_fixture(case=_fixture_case("der_trba9_w512_l120"))


# ---- 3. whole nets against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,sizes", [(7, [2, 2, 3]), (10, [3, 3, 4]), (16, [5, 5, 6])])
def test_svtr_past_six_experts_batch8_vs_oracle(n, sizes):
    """tests/test_model_gpu.py::_ctc_family_b32_case (all of its assertions) at B = 8 on smooth crops over 7, 10 and 16 SVTR experts:
    uneven lock-step sub-groups, G = 4 .. 6 in the grouped SVTR kernels, the 16-wide router from 10 on"""
    from tests.test_model_gpu import _ctc_family_b32_case
    classes = tuple(40 + 23 * i + (i % 3) for i in range(n))
    with recorded_calls() as log:
        got = _ctc_family_b32_case("svtr", classes, "smooth", seed=50 + n, B=8)
    assert got == sizes
    assert any(name == "mrn_gate_tail_fwd_wide_f32" for name, _ in log) == (n > 8)


@pytest.mark.parametrize("crops", ["smooth", "noise"])
def test_svtr10_batch32_full_class_counts_vs_oracle(crops):
    """as test_model_gpu.py::test_svtr6_batch32_full_class_counts_vs_oracle over ten experts with bench-like class counts"""
    from tests.test_model_gpu import _ctc_family_b32_case
    assert _ctc_family_b32_case("svtr", SVTR_BENCH10, crops, seed=47) == [3, 3, 4]


def test_full_size_svtr10_lockstep_matches_per_expert():
    """tests/test_model_gpu.py::test_full_size_svtr_lockstep_matches_per_expert over ten experts at B = 256 (sub-groups 3 + 3 + 4)"""
    from tests.test_model_gpu import test_full_size_svtr_lockstep_matches_per_expert
    assert test_full_size_svtr_lockstep_matches_per_expert(classes=tuple(40 + 23 * i + (i % 3) for i in range(10))) == [3, 3, 4]


def test_loop_a_trba_gradients_vs_oracle_32x512_at_120(ops):
    """tests/test_width_gpu.py::test_loop_a_trba_gradients_vs_oracle_32x512 with batch_max_length 120 (the band rule of
    test_long_labels_gpu.py::test_loop_a_trba_gradients_vs_oracle_150: 3x the fp32 oracle's distance from float64, floor 2e-3):
    121 steps at T = 129 take two launches of each deferred sum, which 121 steps at T = 65 do not"""
    from tests.test_width_gpu import test_loop_a_trba_gradients_vs_oracle_32x512
    assert steps_per_launch(129) < 121 <= steps_per_launch(65)
    test_loop_a_trba_gradients_vs_oracle_32x512(bml=120)


def test_loop_b_crnn10_two_steps_vs_oracle_32x512_at_100():
    """tests/test_width_gpu.py::test_loop_b_two_steps_vs_oracle_48x320 over ten CRNN experts at 32 x 512 (T = P = 127) with labels
    up to 100: the long CTC loss on the fused logits behind the 16-wide router, two Adam steps"""
    from tests.test_width_gpu import test_loop_b_two_steps_vs_oracle_48x320
    with recorded_calls() as log:
        test_loop_b_two_steps_vs_oracle_48x320("crnn", 32, 512, CRNN10, 100)
    names = [n for n, _ in log]
    assert names.count("mrn_ctc_loss_fwd_long_f32") == 2 and "mrn_fanin_bwd_wide_f32" in names


def test_loop_b_trba9_two_steps_vs_oracle_64x128():
    """the same over nine TRBA experts at 64 x 128 (T = P = 33, the 3-row height mean), with the float64 oracle as the yardstick of
    conditioning.  Measured on the host on this input: at step 1 the fp32 oracle's router gradients are 1.0e-4 .. 1.4e-4 (relative L2)
    from the float64 oracle's, but its Adam step of dm_router.0.proj_1.bias is 8.1e-2 from float64's, beyond the 5e-2 band (lr * g / |g|
    on round-off sized elements); the two trajectories then differ, and at step 2 every router gradient of the fp32 oracle is 8e-3 ..
    2.8e-2 from float64's, beyond the 5e-3 band, and that Adam step 8.3e-2.  Those checks are held to 3x the distance measured in the
    run, against float64; every other check keeps the mould's band."""
    from tests.test_width_gpu import test_loop_b_two_steps_vs_oracle_48x320
    with recorded_calls() as log:
        test_loop_b_two_steps_vs_oracle_48x320("trba", 64, 128, TRBA9, 25, f64_yardstick=True)
    names = {n for n, _ in log}
    assert "mrn_fanin_bwd_wide_f32" in names and "mrn_height_mean_grouped_f32" in names


def test_dernet9_trba_step_vs_oracle_32x512_at_120(ops):
    """tests/test_width_gpu.py::test_dernet_step_vs_oracle_32x384 (its bands, every trainable gradient) on the configuration of the
    fixture's der_trba9_w512_l120 at B = 8: D = 2304, T = 129, 121 decoder steps"""
    from tests.test_width_gpu import test_dernet_step_vs_oracle_32x384
    assert not ops.attn_decoder_whole_context(2304, 129) and steps_per_launch(129) < 121
    test_dernet_step_vs_oracle_32x384("trba", 512, CASES["der_trba9_w512_l120"][1], 120, frames=129)


def test_reduced_mode_loop_b_crnn10_32x512():
    """tests/test_width_gpu.py::test_reduced_mode_loop_b (2e-2 / 5e-2, the reduced arithmetic really ran) over ten CRNN experts"""
    from tests.test_width_gpu import test_reduced_mode_loop_b
    test_reduced_mode_loop_b("crnn", 32, 512, classes=CRNN10)


def test_tiny_train_seven_svtr_tasks(tmp_path):
    """tests/test_task_count_gpu.py::test_tiny_train_nine_tasks with SVTR experts over seven tasks (sub-groups 2 + 2 + 3 from the
    seventh task on): finite parameters and accuracies, and a checkpoint that round-trips bit for bit"""
    from mrn_amd import tiny_train
    from mrn_amd.modules.model import MRNNet
    os.chdir(tmp_path)
    opt = types.SimpleNamespace(
        exp_name="t", il="mrn", memory=None, memory_num=20, batch_max_length=25, imgH=32, imgW=256, manual_seed=111, start_task=0,
        num_fiducial=20, input_channel=4, output_channel=512, hidden_size=256, schedule="super", optimizer="adam", lr=0.0005,
        batch_size=4, num_iter=2, val_interval=2, grad_clip=5, lan_list=[f"L{i}" for i in range(7)], NED=True, workers=0)
    opt.Transformation, opt.FeatureExtraction, opt.SequenceModeling, opt.Prediction = STAGES["svtr"]
    train, valid, characters = tiny_train.synthetic_data(opt, [20] + [5] * 6)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        learner, best, ned = tiny_train.train(opt, io.StringIO(), data=(train, valid, characters, lambda t: [valid.create_dataset()]))
    net = getattr(learner.model, "module", learner.model)
    assert len(net.model) == 7 and len(best) == 7
    assert all(0.0 <= float(b) <= 100.0 for b in best)
    assert "nan" not in sink.getvalue().lower()
    assert all(torch.isfinite(q).all() for q in net.parameters())
    assert [hi - lo for lo, hi, _, _ in net._half_groups(True)] == [2, 2, 3]
    path = os.path.join(str(tmp_path), "svtr7.pth")
    torch.save(net.state_dict(), path)
    with contextlib.redirect_stdout(io.StringIO()):
        net2 = MRNNet(opt)
        for m in net.model:
            net2.update_fc(opt.hidden_size, m.fc.out_features)
            net2.build_prediction(opt, m.fc.out_features)
    net2.load_state_dict(torch.load(path), strict=True)
    net2 = net2.cuda().eval()
    net.eval()
    image = (torch.rand(3, 4, 32, 256, generator=torch.Generator().manual_seed(7)) * 2 - 1).cuda()
    with torch.no_grad():
        a, b = net(image, True, None, False), net2(image, True, None, False)
    assert torch.equal(a["index"], b["index"]) and torch.equal(a["logits"], b["logits"])
