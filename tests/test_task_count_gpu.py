"""More than eight tasks on the GPU: the 16-wide router kernels against float64 torch (ragged class counts, ones-padding), the
8-wide path unchanged at up to 8 experts, the DM-Router at 16 experts, the wide-context attention decoder against a float64
restatement and against the single-launch kernel, CRNN / TRBA MRNNets of 10 experts and a TRBA DERNet of 9 extractors against the
reference fixture (tests/golden/many_tasks.npz) and the CPU oracle, a full-size TRBA x 12 loop B, and training over 9 tasks."""
import contextlib
import io
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import assert_close, assert_sub_close, load_golden, oracle_dtype
from tests.test_task_count_cpu import DER_CASE, MRN_CASES, STAGES, tasks_state_dict, tasks_targets

pytestmark = pytest.mark.gpu


def make_opt(kind, imgH=32, imgW=256, bml=25, stages=None, **kw):
    o = types.SimpleNamespace(num_fiducial=20, imgH=imgH, imgW=imgW, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=bml, **kw)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = stages or STAGES[kind]
    return o


def ragged_logits(I, B, T, seed):
    """I experts' logits, growing ragged class counts (most not multiples of 4), in 16-byte-aligned padded rows"""
    from mrn_amd import ops
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(I):
        C = 13 + 7 * i + (i % 3)
        t = ops.padded_rows(B, T, C, "cuda")
        t.copy_(torch.randn(B, T, C, generator=g))
        out.append(t)
    return out


def pad_ones64(logits):
    C = logits[-1].shape[-1]
    return torch.stack([torch.cat([l.cpu().double(), torch.ones(*l.shape[:2], C - l.shape[-1], dtype=torch.float64)], -1)
                        for l in logits], 0)                                          # [I, B, T, C]


# ---- 1. router kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [9, 12, 16])
def test_fanin_and_select_expert_wide_vs_float64(I):
    from mrn_amd import ops
    B, T = 5, 26
    logits = ragged_logits(I, B, T, I)
    g = torch.Generator().manual_seed(100 + I)
    w = torch.softmax(torch.randn(B, I, generator=g), 1)
    L64 = pad_ones64(logits)
    out = ops.fanin_fwd(logits, w.cuda())
    assert_close("fan-in fwd", out, torch.einsum("ibtc,bi->btc", L64, w.double()), atol=1e-5, rtol=1e-5)
    C = logits[-1].shape[-1]
    dout = ops.padded_rows(B, T, C, "cuda")
    dout.copy_(torch.randn(B, T, C, generator=g))
    dw = ops.fanin_bwd(logits, dout)
    assert_close("fan-in bwd", dw, torch.einsum("ibtc,btc->bi", L64, dout.cpu().double()), atol=1e-4, rtol=1e-5)
    index = torch.tensor([0, I - 1, 3, I // 2, 1])                  # the newest expert, the oldest (most padding), the middle
    sel = ops.select_expert(logits, index.cuda())
    assert torch.equal(sel.cpu().double(), torch.stack([L64[index[b], b] for b in range(B)]))


@pytest.mark.parametrize("I", [9, 12, 16])
@pytest.mark.parametrize("beta", [1.0, 5.0])
def test_gate_tail_wide_vs_float64(I, beta):
    from mrn_amd import ops
    B, P = 37, 65
    g = torch.Generator().manual_seed(7 * I)
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


@pytest.mark.parametrize("I", [1, 3, 6, 8])
def test_narrow_path_unchanged_up_to_eight(I, monkeypatch):
    """up to 8 experts ops takes the 8-wide entry points, the launches of the parent commit; the 16-wide form agrees bit for bit"""
    from mrn_amd import ops
    names, real = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    B, T, P = 4, 26, 65
    logits = ragged_logits(I, B, T, 40 + I)
    g = torch.Generator().manual_seed(I)
    w = torch.softmax(torch.randn(B, I, generator=g), 1).cuda()
    C = logits[-1].shape[-1]
    dout = ops.padded_rows(B, T, C, "cuda")
    dout.copy_(torch.randn(B, T, C, generator=g))
    index = (torch.arange(B) % I).cuda()
    r, Wr, br = torch.randn(B, P, I, generator=g).cuda(), torch.randn(P, generator=g).cuda(), torch.randn(1, generator=g).cuda()
    dws = torch.randn(B, I, generator=g).cuda()

    def run(wide):
        s, wt = ops.gate_tail_fwd(r, Wr, br, 2.0, wide=wide)
        _, am = ops.gate_tail_fwd(r, Wr, br, 2.0, hard=True, wide=wide)
        return (ops.fanin_fwd(logits, w, wide=wide), ops.fanin_bwd(logits, dout, wide=wide), ops.select_expert(logits, index, wide=wide),
                s, wt, am) + ops.gate_tail_bwd(wt, dws, r, Wr, 2.0, wide=wide)
    default = run(None)
    assert names and not any(n.endswith("_wide_f32") for n in names)
    for a, b, c in zip(default, run(False), run(True)):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_dm_router_sixteen_experts_vs_float64():
    """DMRouterFn at I = 16 (TRBA: spatial gating over P * I = 1040 tokens, channel gating over I * 256 = 4096 features)"""
    from mrn_amd.modules.dm_router import DM_Router
    from oracle import mrn_oracle as O
    I, P, C, B = 16, 65, 256, 3
    torch.manual_seed(29)
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
                                                      ("r.spatial_gating.proj.weight", "r.channel_gating.proj.weight", "r.proj_1.weight")]:
        a, b = a.cpu().double(), b.double()
        l2 = float((a - b).norm() / b.norm())
        assert l2 <= 2e-3, (name, l2)


# ---- 2. the wide-context attention decoder ------------------------------------------------------------------------------------
def _attention(D, num_class, seed):
    from mrn_amd.modules.prediction import Attention
    torch.manual_seed(seed)
    fc = torch.nn.Linear(256, num_class)
    att = Attention(D, 256, num_class, fc)
    for k, v in att.state_dict().items():
        with torch.no_grad():
            v.mul_(0.5 if v.dim() > 1 else 1.0)
    return att


@pytest.mark.parametrize("D,T", [(2048, 65), (4096, 63), (4096, 65)])
def test_wide_decoder_fwd_bwd_vs_float64(D, T):
    from oracle import mrn_oracle as O
    B, nc = 37, 41
    att = _attention(D, nc, D + T)
    sd = {k: v.detach().clone() for k, v in att.state_dict().items()}
    g = torch.Generator().manual_seed(D * 3 + T)
    H = torch.randn(B, T, D, generator=g) * 0.5
    text = torch.randint(4, nc, (B, 27), generator=g)
    text[:, 0] = 2
    with oracle_dtype(torch.float64) as od:
        sd64 = od.cast(sd)
        for k in ("attention_cell.rnn.weight_ih", "attention_cell.i2h.weight"):
            sd64[k].requires_grad_(True)
        H64 = H.double().requires_grad_(True)
        ref = O.attention_forward(sd64, "", H64, text[:, :-1], True, 25, sd64["generator.weight"], sd64["generator.bias"])
        dy = torch.randn(ref.shape, generator=g).double()
        ref.backward(dy)
    att = att.cuda()
    Hd = H.cuda().requires_grad_(True)
    out = att(Hd, text[:, :-1].cuda(), True)
    scale = float(ref.detach().abs().max())
    assert_close("decoder fwd", out, ref.detach(), atol=1e-4 * scale, rtol=0)
    out.backward(dy.float().cuda())
    for name, a, b in (("dH", Hd.grad, H64.grad), ("dW_ih", att.attention_cell.rnn.weight_ih.grad, sd64["attention_cell.rnn.weight_ih"].grad),
                       ("dW_i2h", att.attention_cell.i2h.weight.grad, sd64["attention_cell.i2h.weight"].grad)):
        a, b = a.cpu().double(), b.double()
        l2 = float((a - b).norm() / b.norm())
        assert l2 <= 2e-3, (name, l2)
    # greedy decoding through the same wide path
    with torch.no_grad():
        gr = att(Hd.detach(), torch.LongTensor(B).fill_(2).cuda(), False)
        with oracle_dtype(torch.float64) as od:
            gr64 = O.attention_forward(od.cast(sd), "", H.double(), torch.LongTensor(B).fill_(2), False, 25, sd["generator.weight"].double(),
                                       sd["generator.bias"].double())
    agree = (gr.argmax(2).cpu() == gr64.argmax(2)).all(1)
    assert float(agree.float().mean()) >= 0.9


@pytest.mark.parametrize("D", [256, 1792])
@pytest.mark.parametrize("x3", ["1", "0"])
def test_wide_decoder_equals_single_launch_where_it_fits(D, x3, monkeypatch, T=65):
    """at a D the single-launch form takes, the chunked form (forced) computes the same thing: the MFMAs run in the same order"""
    from mrn_amd import ops
    monkeypatch.setattr(ops, "DECODER_X3", x3 == "1")
    B, nc = 37, 41
    att = _attention(D, nc, D).cuda()
    g = torch.Generator().manual_seed(D)
    H = (torch.randn(B, T, D, generator=g) * 0.5).cuda()
    text = torch.randint(4, nc, (B, 27), generator=g).cuda()
    with torch.no_grad():
        one = att(H, text[:, :-1], True)
        monkeypatch.setenv("MRN_ATTN_CTX_CHUNK", "1")
        chunked = att(H, text[:, :-1], True)
        monkeypatch.delenv("MRN_ATTN_CTX_CHUNK")
        again = att(H, text[:, :-1], True)
    assert torch.equal(one, again)
    assert_close("chunked vs single launch", chunked, one, atol=1e-6, rtol=1e-6)


# ---- 3. nets past eight tasks against the reference fixture and the oracle -----------------------------------------------------
def _build(net_cls, kind, classes, der=False, opt=None):
    from mrn_amd.modules import model as M
    opt = opt or make_opt(kind)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(M, net_cls)(opt)
        for c in classes:
            net.update_fc(opt.hidden_size, c)
            net.build_prediction(opt, c)
            if der:
                net.build_aux_prediction(opt, c)
    return net


@pytest.mark.parametrize("kind", ["crnn", "trba"])
def test_mrn10_vs_reference_fixture(kind, case=None):
    """loop B (fused logits, routing weights, router gradients), eval routing and greedy indices of a 10-expert MRNNet against the
    reference (B = 2).  Band: 1e-4, or for TRBA 3x the distance of the reference's fp32 result from float64 arithmetic on the same
    quantity (as test_geometry_gpu.py::test_mrn2_vs_reference_fixture).  case: another fixture's configuration -- golden (file),
    prefix, classes, seed, targets (image, targets, lengths, domain), opt, cfg (the oracle's), masks (SVTR DropPath draws)"""
    from mrn_amd import functional as Fn
    from oracle import mrn_oracle as O
    from tests.test_model_gpu import set_drop_masks_from
    case = case or {}
    g = load_golden(case.get("golden", "many_tasks"))
    p = case.get("prefix", f"mrn_{kind}/")
    classes, seed = (case["classes"], case["seed"]) if case else MRN_CASES[kind]
    attn = kind == "trba"
    B = 2
    image, tgt, lens, domain = case["targets"] if case else tasks_targets(f"mrn_{kind}", attn, classes, seed)
    text = tgt[:, :-1] if attn else None
    net = _build("MRNNet", kind, classes, opt=case.get("opt"))
    net.load_state_dict(tasks_state_dict(g, p, seed), strict=True)
    ref64 = {}
    if attn:
        with oracle_dtype(torch.float64) as od, torch.no_grad():
            ob = O.mrn_forward(od.cast(tasks_state_dict(g, p, seed)), case.get("cfg") or O.Cfg(*STAGES[kind]), len(classes), image.double(), True, text, True,
                               training=True)
        ref64 = {"stepB/weights": ob["index"], "stepB/logits": ob["logits"]}

    def check(name, t, full=False):
        from tests.helpers import sub
        mine = t.detach().cpu().double().numpy() if full else sub(t)[0].astype(np.float64)
        ref = g[p + name] if full else g[p + name + "/sub"].astype(np.float64)
        tol = 1e-4 + 1e-4 * np.abs(ref).max()
        if name in ref64:
            r64 = ref64[name].numpy() if full else sub(ref64[name])[0].astype(np.float64)
            tol = max(tol, 3 * np.abs(ref - r64).max())
        err = np.abs(mine - ref).max()
        assert err <= tol, f"{name}: max abs err {err:.3e} > tol {tol:.3e}"
    net = net.cuda().train()
    for n, q in net.named_parameters():
        q.requires_grad = not n.startswith("model.")
    set_drop_masks_from(net, case.get("masks"))
    out = net(image.cuda(), True, None if text is None else text.cuda(), True)
    check("stepB/weights", out["index"], full=True)
    check("stepB/logits", out["logits"])
    assert np.array_equal(out["index"].detach().cpu().numpy().argmax(1), g[p + "stepB/weights"].argmax(1))
    clf = Fn.cross_entropy(out["logits"], tgt[:, 1:].cuda(), 1) if attn else Fn.ctc_loss(out["logits"], tgt.cuda(), lens.cuda())
    loss = 15 * clf + Fn.cross_entropy(out["index"], domain.cuda(), -100)
    loss.backward()
    for k in ("route.weight", "channel_route.weight", "dm_router.0.proj_1.weight"):
        gr = net.get_parameter(k).grad
        ref = g[p + "stepB/grad/" + k + "/sub"].astype(np.float64)
        from tests.helpers import sub
        mine = sub(gr)[0].astype(np.float64)
        rel = np.linalg.norm(mine - ref) / max(np.linalg.norm(ref), 1e-12)
        assert rel <= (2e-2 if attn else 2e-3), (k, rel)
    net.load_state_dict(tasks_state_dict(g, p, seed), strict=True)
    net.eval()
    with torch.no_grad():
        oe = net(image.cuda(), True, torch.LongTensor(B).fill_(2).cuda() if attn else None, False)
    assert np.array_equal(oe["index"].cpu().numpy(), g[p + "eval/index"])
    assert float((oe["logits"].max(2)[1].cpu().numpy() == g[p + "eval/argmax"]).mean()) >= 0.99


def test_dernet9_step_vs_reference_fixture(case=None):
    """one DER training step of a TRBA DERNet over 9 extractors (main head over D = 2304: the wide-context decoder, forward and
    backward) against the reference fixture and the oracle"""
    from mrn_amd import functional as Fn
    from oracle import mrn_oracle as O
    from tests.helpers import sub
    case = case or {}
    g = load_golden(case.get("golden", "many_tasks"))
    p = case.get("prefix", "der_trba/")
    classes, seed = (case["classes"], case["seed"]) if case else DER_CASE
    image, tgt, _, _ = case["targets"] if case else tasks_targets("der_trba", True, classes, seed)
    net = _build("DERNet", "trba", classes, der=True, opt=case.get("opt"))
    net.load_state_dict(tasks_state_dict(g, p, seed), strict=True)
    net = net.cuda().train()
    for ext in list(net.model)[:-1]:
        ext.eval()
        for q in ext.parameters():
            q.requires_grad = False
    out = net(image.cuda(), tgt[:, :-1].cuda())
    with oracle_dtype(torch.float64) as od, torch.no_grad():
        o64 = O.dernet_forward(od.cast(tasks_state_dict(g, p, seed)), case.get("cfg") or O.Cfg(*STAGES["trba"]), len(classes), image.double(),
                               tgt[:, :-1], True, training=True)
    for name, t in (("logits", out["logits"]), ("aux_logits", out["aux_logits"])):
        ref, r64 = g[p + name + "/sub"].astype(np.float64), sub(o64[name])[0].astype(np.float64)
        tol = max(1e-4 + 1e-4 * np.abs(ref).max(), 3 * np.abs(ref - r64).max())
        assert np.abs(sub(t)[0] - ref).max() <= tol, name
    loss = Fn.cross_entropy(out["logits"], tgt[:, 1:].cuda(), 1)
    assert abs(loss.item() - float(g[p + "loss"])) <= 1e-3 * max(1.0, float(g[p + "loss"]))
    loss.backward()
    params = dict(net.named_parameters(remove_duplicate=False))
    for k in ("fc.weight", "Prediction.attention_cell.rnn.weight_ih", "Prediction.attention_cell.i2h.weight"):
        ref = g[p + "grad/" + k + "/sub"].astype(np.float64)
        mine = sub(params[k].grad)[0].astype(np.float64)
        rel = np.linalg.norm(mine - ref) / max(np.linalg.norm(ref), 1e-12)
        assert rel <= 2e-2, (k, rel)


# ---- 4. full size and end to end -----------------------------------------------------------------------------------------------
def test_full_size_trba12_loop_b():
    from mrn_amd import functional as Fn
    from mrn_amd.tools import weights as W
    classes = tuple(41 + 10 * i for i in range(12))
    B = 256
    net = _build("MRNNet", "trba", classes)
    W.fill_state_dict(net.state_dict(), seed=31)
    net = net.cuda().train()
    for n, q in net.named_parameters():
        q.requires_grad = not n.startswith("model.")
    image = torch.from_numpy(W.uniform("tasks_full", (B, 4, 32, 256), -1.0, 1.0, 31)).cuda()
    text = torch.from_numpy(W.randint("tasks_full_text", (B, 27), 4, classes[-1], 31)).cuda()
    text[:, 0] = 2
    domain = torch.arange(B, device="cuda") % len(classes)
    out = net(image, True, text[:, :-1], True)
    loss = 15 * Fn.cross_entropy(out["logits"], text[:, 1:], 1) + Fn.cross_entropy(out["index"], domain, -100)
    loss.backward()
    assert out["index"].shape == (B, 12)
    assert torch.isfinite(out["logits"]).all() and torch.isfinite(loss).item()
    assert_close("routing weights sum", out["index"].sum(1), torch.ones(B), atol=1e-5)
    assert all(torch.isfinite(q.grad).all() for q in net.parameters() if q.grad is not None)


@pytest.mark.parametrize("il", ["mrn", "der"])
def test_tiny_train_nine_tasks(tmp_path, il):
    from mrn_amd import tiny_train
    os.chdir(tmp_path)
    opt = types.SimpleNamespace(
        exp_name="t", il=il, memory=None, memory_num=20, batch_max_length=25, imgH=32, imgW=256, manual_seed=111, start_task=0,
        num_fiducial=20, input_channel=4, output_channel=512, hidden_size=256, schedule="super", optimizer="adam", lr=0.0005,
        batch_size=4, num_iter=2, val_interval=2, grad_clip=5, lan_list=[f"L{i}" for i in range(9)], NED=True, workers=0)
    opt.Transformation, opt.FeatureExtraction, opt.SequenceModeling, opt.Prediction = STAGES["crnn"]
    train, valid, characters = tiny_train.synthetic_data(opt, [20] + [5] * 8)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        learner, best, ned = tiny_train.train(opt, io.StringIO(), data=(train, valid, characters, lambda t: [valid.create_dataset()]))
    assert len(learner.model.model) == 9 and len(best) == 9
    assert all(torch.isfinite(q).all() for q in learner.model.parameters())
