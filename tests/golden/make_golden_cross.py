"""Reference outputs where task count, input geometry and label length meet (CPU, the reference implementation), for
tests/test_cross_axes_cpu.py / _gpu.py.

    python tests/golden/make_golden_cross.py [OUT.npz]

Imports the reference and the weight generator exactly as make_golden.py does (it is imported from there).  B = 2, small ragged
class counts.  Per MRNNet case (10 experts: SVTR at 32 x 256 with injected DropPath draws, CRNN at 32 x 512 with labels up to 100,
TRBA at 64 x 128) it stores what make_golden_tasks.py stores: the loop-B fused logits and routing weights, the gradients of three
router tensors under loop B's loss (15 * clf + CE(weights, domain)), and the eval-mode routing indices and greedy indices.  For a
TRBA DERNet of 9 extractors at 32 x 512 and batch_max_length 120 (old extractors in eval mode, the newest in train mode) it stores
the main and auxiliary logits, the classification loss and three head gradients.  Large tensors are make_golden.put's strided
subsample plus moments.  As in make_golden_width.py, net.patch is set to the real frame count of a line that is not 256 pixels wide
before the first update_fc.  Writes tests/golden/cross_axes.npz (or OUT.npz).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (reference import shims, state_dict filler, put, DropPath injection)
from make_golden import MRNNet, W, put  # noqa: E402

STAGES = {"trba": ("TPS", "ResNet", "BiLSTM", "Attn"), "crnn": ("None", "VGG", "BiLSTM", "CTC"), "svtr": ("None", "SVTR", "None", "CTC")}
# key -> (kind, class counts, imgH, imgW, batch_max_length, seed)
CASES = {
    "mrn_svtr10": ("svtr", tuple(40 + 3 * i + (i % 3) for i in range(10)), 32, 256, 25, 71),
    "der_trba9_w512_l120": ("trba", tuple(41 + 3 * i for i in range(9)), 32, 512, 120, 72),
    "mrn_crnn10_w512_l100": ("crnn", tuple(40 + 3 * i + (i % 3) for i in range(10)), 32, 512, 100, 73),
    "mrn_trba10_h64_w128": ("trba", tuple(41 + 3 * i + (i % 2) for i in range(10)), 64, 128, 25, 74),
}
ROUTER_GRADS = ("route.weight", "channel_route.weight", "dm_router.0.proj_1.weight")
DER_GRADS = ("fc.weight", "Prediction.attention_cell.rnn.weight_ih", "Prediction.attention_cell.i2h.weight")
B = 2


def make_opt(kind, imgH, imgW, bml):
    o = types.SimpleNamespace(num_fiducial=20, imgH=imgH, imgW=imgW, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=bml)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = STAGES[kind]
    return o


def targets(key):
    """(image, attention text [B, bml + 2] or CTC labels [B, bml] + lengths, domain): the same generator calls as the tests; the
    first CTC label has the full batch_max_length"""
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


def keys(d, p, net):
    sd = net.state_dict()
    d[p + "sd_keys"] = np.array(sorted(sd.keys()))
    d[p + "sd_shapes"] = np.array([",".join(map(str, sd[k].shape)) for k in sorted(sd.keys())])


def mrn_case(d, key):
    kind, classes, imgH, imgW, bml, seed = CASES[key]
    p = key + "/"
    opt = make_opt(kind, imgH, imgW, bml)
    net = MRNNet(opt)
    if imgW != 256:                                       # the shim of make_golden_width.py: the reference hard-codes the 256-pixel patch count
        net.patch = imgW // 4 + (1 if opt.FeatureExtraction == "ResNet" else -1)
    for c in classes:
        net.update_fc(opt.hidden_size, c)
        net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed)
    keys(d, p, net)
    attn = kind == "trba"
    image, tgt, lens, domain = targets(key)
    text = tgt[:, :-1] if attn else None
    # loop B: fused logits, routing weights, router gradients (experts in train mode, il_modules/mrn.py:323-371)
    net.train()
    net.zero_grad()
    G.DROP_MASKS.clear()
    if kind == "svtr":
        for e in G.drop_masks(B, seed, key, len(classes)):
            G.DROP_MASKS.extend(e)
    out = net(image, True, text, True)
    assert not G.DROP_MASKS
    if attn:
        clf = torch.nn.CrossEntropyLoss(ignore_index=1)(out["logits"].reshape(-1, out["logits"].shape[-1]), tgt[:, 1:].reshape(-1))
    else:
        lp = out["logits"].log_softmax(2).permute(1, 0, 2)
        clf = torch.nn.CTCLoss(reduction="mean", zero_infinity=True)(lp, tgt, torch.IntTensor([lp.size(0)] * B), lens)
    loss = 15 * clf + torch.nn.CrossEntropyLoss()(out["index"], domain)
    loss.backward()
    put(d, p + "stepB/weights", out["index"], full=True)
    put(d, p + "stepB/logits", out["logits"])
    d[p + "stepB/loss"] = np.float64(loss.item())
    params = dict(net.named_parameters())
    for k in ROUTER_GRADS:
        put(d, p + "stepB/grad/" + k, params[k].grad)
    W.fill_state_dict(net.state_dict(), seed)             # (the running statistics moved)
    # eval: hard routing, greedy decoding
    net.eval()
    with torch.no_grad():
        oe = net(image, True, torch.LongTensor(B).fill_(2) if attn else None, False)
    d[p + "eval/index"] = oe["index"].numpy()
    d[p + "eval/argmax"] = oe["logits"].max(2)[1].numpy()


def der_case(d, key):
    from modules.model import DERNet
    kind, classes, imgH, imgW, bml, seed = CASES[key]
    p = key + "/"
    opt = make_opt(kind, imgH, imgW, bml)
    net = DERNet(opt)
    for c in classes:
        net.update_fc(opt.hidden_size, c)
        net.build_prediction(opt, c)
        net.build_aux_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed)
    keys(d, p, net)
    image, tgt, _, _ = targets(key)
    net.train()
    for ext in list(net.model)[:-1]:                      # DER.model_eval_and_train: older extractors eval and frozen
        ext.eval()
        for q in ext.parameters():
            q.requires_grad = False
    net.zero_grad()
    out = net(image, tgt[:, :-1])
    loss = torch.nn.CrossEntropyLoss(ignore_index=1)(out["logits"].reshape(-1, classes[-1]), tgt[:, 1:].reshape(-1))
    loss.backward()
    put(d, p + "logits", out["logits"])
    put(d, p + "aux_logits", out["aux_logits"])
    d[p + "loss"] = np.float64(loss.item())
    params = dict(net.named_parameters(remove_duplicate=False))      # (fc aliases Prediction.generator)
    for k in DER_GRADS:
        put(d, p + "grad/" + k, params[k].grad)


if __name__ == "__main__":
    torch.set_num_threads(8)
    d = {}
    for key in CASES:
        (der_case if key.startswith("der_") else mrn_case)(d, key)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(G.OUT, "cross_axes.npz")
    np.savez_compressed(path, **d)
    print("cross_axes ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
