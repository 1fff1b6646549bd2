"""Where task count, input geometry and label length meet, on the CPU: the C ABI of the deferred-sum steps query, the dispatch
rules restated in Python at the crossings, and the CPU oracle against the reference's own outputs at four crossings
(tests/golden/cross_axes.npz, written by tests/golden/make_golden_cross.py) at the bands of tests/test_task_count_cpu.py -- what
makes the oracle the yardstick of tests/test_cross_axes_gpu.py."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close, assert_sub_close, drop_masks, load_golden
from tests.test_task_count_cpu import tasks_state_dict

STAGES = {"trba": ("TPS", "ResNet", "BiLSTM", "Attn"), "crnn": ("None", "VGG", "BiLSTM", "CTC"), "svtr": ("None", "SVTR", "None", "CTC")}
# key -> (kind, class counts, imgH, imgW, batch_max_length, seed): tests/golden/make_golden_cross.py CASES
CASES = {
    "mrn_svtr10": ("svtr", tuple(40 + 3 * i + (i % 3) for i in range(10)), 32, 256, 25, 71),
    "der_trba9_w512_l120": ("trba", tuple(41 + 3 * i for i in range(9)), 32, 512, 120, 72),
    "mrn_crnn10_w512_l100": ("crnn", tuple(40 + 3 * i + (i % 3) for i in range(10)), 32, 512, 100, 73),
    "mrn_trba10_h64_w128": ("trba", tuple(41 + 3 * i + (i % 2) for i in range(10)), 64, 128, 25, 74),
}
MRN_KEYS = [k for k in CASES if k.startswith("mrn_")]
B = 2


def cross_targets(key):
    """the generator's inputs (make_golden_cross.py: targets)"""
    from mrn_amd.tools import weights as W
    kind, classes, imgH, imgW, bml, seed = CASES[key]
    image = torch.from_numpy(W.smooth_image(f"cross:{key}", (B, 4, imgH, imgW), seed))
    domain = torch.from_numpy(W.randint(f"cross:{key}:domain", (B,), 0, len(classes), seed))
    if kind == "trba":
        text = torch.from_numpy(W.randint(f"cross:{key}:text", (B, bml + 2), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None, domain
    lens = torch.from_numpy(W.randint(f"cross:{key}:len", (B,), 1, bml + 1, seed)).int()
    lens[0] = bml
    labels = torch.from_numpy(W.randint(f"cross:{key}:ctc", (B, bml), 4, classes[-1], seed))
    labels[torch.arange(bml)[None, :] >= lens[:, None]] = 1
    return image, labels, lens, domain


def cross_cfg(key):
    from oracle import mrn_oracle as O
    kind, _, imgH, imgW, bml, _ = CASES[key]
    return O.Cfg(*STAGES[kind], imgH=imgH, imgW=imgW, batch_max_length=bml)


def cross_masks(key):
    kind, classes, _, _, _, seed = CASES[key]
    return drop_masks(B, seed, key, len(classes)) if kind == "svtr" else None


def test_steps_query_in_the_header():
    from mrn_amd import _lib
    protos = _lib.parse_header()
    assert protos["mrn_attn_decoder_bwd_steps_per_launch"] == ("int64_t", ["int"], ["T"])
    assert protos["mrn_attn_decoder_bwd_parts"][0] == "int64_t"


def test_decoder_form_at_the_crossings():
    """the forward's rule (ops.attn_decoder_whole_context) over the (D, T) plane the GPU suite walks: D = 1792 is the widest
    single-launch tile at every supported T, 158 528 B of 163 840 B at T = 129 in the x3 form"""
    from mrn_amd import ops
    for T in (33, 65, 129):
        for x3 in (True, False):
            assert ops.attn_decoder_whole_context(1792, T, x3)
            assert not ops.attn_decoder_whole_context(2048, T, x3)
    assert 4 * (2 * 16 * 260 + 16 * (1792 + 4) + 16 * 129 + 256) + 1024 == 158528


def test_fixture_is_small_and_complete():
    import os
    from tests.helpers import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "cross_axes.npz")) < 1024 * 1024
    g = load_golden("cross_axes")
    for key in CASES:
        assert key + "/sd_keys" in g.files
    assert tuple(g["mrn_crnn10_w512_l100/stepB/logits/shape"])[:2] == (B, 127)
    assert tuple(g["mrn_trba10_h64_w128/stepB/logits/shape"])[:2] == (B, 26)
    assert tuple(g["der_trba9_w512_l120/logits/shape"])[:2] == (B, 121)
    assert g["mrn_svtr10/stepB/weights"].shape == (B, 10)


@pytest.mark.parametrize("key", MRN_KEYS)
def test_oracle_matches_reference_mrn10(key):
    import torch.nn.functional as F
    from oracle import mrn_oracle as O
    g = load_golden("cross_axes")
    p = key + "/"
    kind, classes, imgH, imgW, bml, seed = CASES[key]
    attn = kind == "trba"
    cfg = cross_cfg(key)
    image, tgt, lens, domain = cross_targets(key)
    text = tgt[:, :-1] if attn else None
    sd = tasks_state_dict(g, p, seed)
    names = [str(k)[len(p + "stepB/grad/"):-len("/sub")] for k in g.files if k.startswith(p + "stepB/grad/") and k.endswith("/sub")]
    assert len(names) == 3
    params = [sd[n].requires_grad_(True) for n in names]
    out = O.mrn_forward(sd, cfg, len(classes), image, True, text, True, training=True, masks=cross_masks(key))
    clf = O.attn_ce_loss(out["logits"], tgt) if attn else O.ctc_loss(out["logits"], tgt, lens)
    loss = 15 * clf + F.cross_entropy(out["index"], domain)
    grads = torch.autograd.grad(loss, params)
    assert out["index"].shape == (B, 10)
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


def test_oracle_matches_reference_der9_w512_l120():
    from oracle import mrn_oracle as O
    key = "der_trba9_w512_l120"
    g = load_golden("cross_axes")
    p = key + "/"
    kind, classes, imgH, imgW, bml, seed = CASES[key]
    image, tgt, _, _ = cross_targets(key)
    sd = tasks_state_dict(g, p, seed)
    names = [str(k)[len(p + "grad/"):-len("/sub")] for k in g.files if k.startswith(p + "grad/") and k.endswith("/sub")]
    assert len(names) == 3
    params = [sd[n].requires_grad_(True) for n in names]
    out = O.dernet_forward(sd, cross_cfg(key), len(classes), image, tgt[:, :-1], True, training=True)
    assert out["features"].shape == (B, 129, 2304) and out["logits"].shape[1] == 121
    loss = O.attn_ce_loss(out["logits"], tgt)
    grads = torch.autograd.grad(loss, params)
    assert_sub_close(g, p + "logits", out["logits"], atol=2e-5)
    assert_sub_close(g, p + "aux_logits", out["aux_logits"], atol=2e-5)
    assert abs(loss.item() - float(g[p + "loss"])) <= 1e-5 * max(1.0, abs(float(g[p + "loss"])))
    for n, gr in zip(names, grads):
        assert_sub_close(g, p + "grad/" + n, gr, atol=1e-6, rtol=2e-3)
