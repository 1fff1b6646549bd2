"""Task counts on the CPU: the pure-Python predicate behind the refusals, the refusal of a 17th task on both nets (before any
launch), the C ABI of the 16-wide router entry points, and the CPU oracle against the reference's own outputs past eight tasks
(tests/golden/many_tasks.npz, written by tests/golden/make_golden_tasks.py) -- what makes the oracle the yardstick of
tests/test_task_count_gpu.py."""
import contextlib
import io
import types

import numpy as np
import pytest
import torch

from mrn_amd.modules.task_count import MAX_TASKS, router_uses_wide_kernels, tasks_supported, unsupported_task_count_message
from tests.helpers import assert_close, assert_sub_close, load_golden

STAGES = {"trba": ("TPS", "ResNet", "BiLSTM", "Attn"), "crnn": ("None", "VGG", "BiLSTM", "CTC")}
MRN_CASES = {"trba": (tuple(41 + 3 * i + (i % 2) for i in range(10)), 61), "crnn": (tuple(40 + 3 * i + (i % 3) for i in range(10)), 62)}
DER_CASE = (tuple(41 + 3 * i for i in range(9)), 63)
B = 2


def test_limits():
    assert MAX_TASKS == 16


@pytest.mark.parametrize("n,supported,wide", [(0, False, False), (1, True, False), (6, True, False), (8, True, False),
                                              (9, True, True), (12, True, True), (16, True, True), (17, False, False),
                                              (-1, False, False)])
def test_predicate_boundaries(n, supported, wide):
    assert tasks_supported(n) is supported
    assert router_uses_wide_kernels(n) is wide


def test_refusal_message_names_the_range():
    msg = unsupported_task_count_message("MRNNet", 17)
    assert "1..16 tasks" in msg and "MRNNet would have 17" in msg


def _opt(kind):
    o = types.SimpleNamespace(num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=25)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = STAGES[kind]
    return o


@pytest.mark.parametrize("net_name", ["MRNNet", "DERNet"])
def test_update_fc_refuses_the_17th_task(net_name):
    from mrn_amd.modules import model as M
    opt = _opt("crnn")
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(M, net_name)(opt)
        for t in range(16):
            net.update_fc(opt.hidden_size, 40 + t)
        assert len(net.model) == 16
        with pytest.raises(NotImplementedError, match=r"1\.\.16 tasks .*%s would have 17" % net_name):
            net.update_fc(opt.hidden_size, 60)
    assert len(net.model) == 16                                   # nothing was appended


def test_router_refuses_17_experts_before_any_launch(monkeypatch):
    from mrn_amd import ops
    calls = []
    monkeypatch.setattr(ops, "call", lambda *a: calls.append(a))
    with pytest.raises(NotImplementedError, match=r"1\.\.16 tasks"):
        ops.gate_tail_fwd(torch.zeros(2, 65, 17), torch.zeros(65), torch.zeros(1))
    assert calls == []


def test_router_chooses_the_form_from_the_expert_count(monkeypatch):
    from mrn_amd import ops
    names = []
    monkeypatch.setattr(ops, "call", lambda name, *a: names.append(name))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    for I in (1, 8, 9, 16):
        ops.gate_tail_fwd(torch.zeros(2, 65, I), torch.zeros(65), torch.zeros(1))
    assert names == ["mrn_gate_tail_fwd_f32"] * 2 + ["mrn_gate_tail_fwd_wide_f32"] * 2


def test_wide_entry_points_in_the_header():
    from mrn_amd import _lib
    protos = _lib.parse_header()
    for base in ("mrn_fanin_fwd", "mrn_fanin_bwd", "mrn_select_expert", "mrn_gate_tail_fwd", "mrn_gate_tail_bwd"):
        assert protos[base + "_wide_f32"] == protos[base + "_f32"]      # drop-in forms of the 8-wide entry points


# ---- the CPU oracle against the reference's outputs past eight tasks (tests/golden/make_golden_tasks.py) ---------------------
def tasks_state_dict(g, p, seed):
    from mrn_amd.tools import weights as W
    sd = {}
    for k, shp in zip(g[p + "sd_keys"], g[p + "sd_shapes"]):
        k = str(k)
        shape = tuple(int(v) for v in str(shp).split(",")) if str(shp) else ()
        sd[k] = torch.from_numpy(np.array(W.det_param(W.canonical_key(k), shape, seed)))
    return sd


def tasks_targets(tag, attn, classes, seed):
    """the generator's inputs (make_golden_tasks.py: targets)"""
    from mrn_amd.tools import weights as W
    image = torch.from_numpy(W.smooth_image(f"tasks:{tag}", (B, 4, 32, 256), seed))
    domain = torch.from_numpy(W.randint(f"tasks:{tag}:domain", (B,), 0, len(classes), seed))
    if attn:
        text = torch.from_numpy(W.randint(f"tasks:{tag}:text", (B, 27), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None, domain
    lens = torch.from_numpy(W.randint(f"tasks:{tag}:len", (B,), 1, 26, seed)).int()
    labels = torch.from_numpy(W.randint(f"tasks:{tag}:ctc", (B, 25), 4, classes[-1], seed))
    labels[torch.arange(25)[None, :] >= lens[:, None]] = 1
    return image, labels, lens, domain


@pytest.mark.parametrize("kind", ["crnn", "trba"])
def test_oracle_matches_reference_mrn10(kind):
    import torch.nn.functional as F
    from oracle import mrn_oracle as O
    g = load_golden("many_tasks")
    p = f"mrn_{kind}/"
    classes, seed = MRN_CASES[kind]
    attn = kind == "trba"
    cfg = O.Cfg(*STAGES[kind])
    image, tgt, lens, domain = tasks_targets(f"mrn_{kind}", attn, classes, seed)
    text = tgt[:, :-1] if attn else None
    sd = tasks_state_dict(g, p, seed)
    names = [str(k)[len(p + "stepB/grad/"):-len("/sub")] for k in g.files if k.startswith(p + "stepB/grad/") and k.endswith("/sub")]
    params = [sd[n].requires_grad_(True) for n in names]
    out = O.mrn_forward(sd, cfg, len(classes), image, True, text, True, training=True)
    clf = O.attn_ce_loss(out["logits"], tgt) if attn else O.ctc_loss(out["logits"], tgt, lens)
    loss = 15 * clf + F.cross_entropy(out["index"], domain)
    grads = torch.autograd.grad(loss, params)
    assert_close("routing weights", out["index"], g[p + "stepB/weights"], atol=1e-5)
    assert_sub_close(g, p + "stepB/logits", out["logits"], atol=2e-5)
    assert abs(loss.item() - float(g[p + "stepB/loss"])) <= 1e-4 * max(1.0, abs(float(g[p + "stepB/loss"])))
    for n, gr in zip(names, grads):
        assert_sub_close(g, p + "stepB/grad/" + n, gr, atol=1e-6, rtol=2e-3)
    sd = tasks_state_dict(g, p, seed)
    with torch.no_grad():
        oe = O.mrn_forward(sd, cfg, len(classes), image, True, torch.LongTensor(B).fill_(2) if attn else None, False, training=False)
    assert np.array_equal(oe["index"].numpy(), g[p + "eval/index"])
    assert np.array_equal(oe["logits"].max(2)[1].numpy(), g[p + "eval/argmax"])


def test_oracle_matches_reference_der9():
    from oracle import mrn_oracle as O
    g = load_golden("many_tasks")
    p = "der_trba/"
    classes, seed = DER_CASE
    cfg = O.Cfg(*STAGES["trba"])
    image, tgt, _, _ = tasks_targets("der_trba", True, classes, seed)
    sd = tasks_state_dict(g, p, seed)
    names = [str(k)[len(p + "grad/"):-len("/sub")] for k in g.files if k.startswith(p + "grad/") and k.endswith("/sub")]
    params = [sd[n].requires_grad_(True) for n in names]
    out = O.dernet_forward(sd, cfg, len(classes), image, tgt[:, :-1], True, training=True)
    loss = O.attn_ce_loss(out["logits"], tgt)
    grads = torch.autograd.grad(loss, params)
    assert_sub_close(g, p + "logits", out["logits"], atol=2e-5)
    assert_sub_close(g, p + "aux_logits", out["aux_logits"], atol=2e-5)
    assert abs(loss.item() - float(g[p + "loss"])) <= 1e-5 * max(1.0, abs(float(g[p + "loss"])))
    for n, gr in zip(names, grads):
        assert_sub_close(g, p + "grad/" + n, gr, atol=1e-6, rtol=2e-3)
