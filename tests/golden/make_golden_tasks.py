"""Reference outputs past eight tasks (CPU, the reference implementation), for tests/test_task_count_cpu.py / _gpu.py.

    python tests/golden/make_golden_tasks.py [OUT.npz]

Imports the reference and the weight generator exactly as make_golden.py does (it is imported from there).  For a CRNN and a TRBA
MRNNet of 10 experts (B = 2, small ragged class counts) it stores the loop-B fused logits and routing weights, the gradients of
three router tensors under loop B's loss (15 * clf + CE(weights, domain)), and the eval-mode routing indices and greedy indices.
For a TRBA DERNet of 9 extractors (old extractors in eval mode, the newest in train mode, as DER trains it) it stores the main and
auxiliary logits, the classification loss and three head gradients.  Large tensors are make_golden.put's strided subsample plus
moments.  Writes tests/golden/many_tasks.npz (or OUT.npz).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (reference import shims, state_dict filler, put)
from make_golden import MRNNet, W, put  # noqa: E402

STAGES = {"trba": ("TPS", "ResNet", "BiLSTM", "Attn"), "crnn": ("None", "VGG", "BiLSTM", "CTC")}
MRN_CASES = {"trba": (tuple(41 + 3 * i + (i % 2) for i in range(10)), 61), "crnn": (tuple(40 + 3 * i + (i % 3) for i in range(10)), 62)}
DER_CASE = (tuple(41 + 3 * i for i in range(9)), 63)
ROUTER_GRADS = ("route.weight", "channel_route.weight", "dm_router.0.proj_1.weight")
DER_GRADS = ("fc.weight", "Prediction.attention_cell.rnn.weight_ih", "Prediction.attention_cell.i2h.weight")
B = 2


def make_opt(kind):
    o = types.SimpleNamespace(num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=25)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = STAGES[kind]
    return o


def targets(tag, attn, classes, seed):
    """(image, attention text [B,27] or CTC labels [B,25] + lengths, domain): the same generator calls as the tests"""
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


def keys(d, p, net):
    sd = net.state_dict()
    d[p + "sd_keys"] = np.array(sorted(sd.keys()))
    d[p + "sd_shapes"] = np.array([",".join(map(str, sd[k].shape)) for k in sorted(sd.keys())])


def mrn_case(d, kind):
    p = f"mrn_{kind}/"
    classes, seed = MRN_CASES[kind]
    opt = make_opt(kind)
    net = MRNNet(opt)
    for c in classes:
        net.update_fc(opt.hidden_size, c)
        net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed)
    keys(d, p, net)
    attn = kind == "trba"
    image, tgt, lens, domain = targets(f"mrn_{kind}", attn, classes, seed)
    text = tgt[:, :-1] if attn else None
    # loop B: fused logits, routing weights, router gradients (experts in train mode, il_modules/mrn.py:323-371)
    net.train()
    net.zero_grad()
    out = net(image, True, text, True)
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


def der_case(d):
    from modules.model import DERNet
    p = "der_trba/"
    classes, seed = DER_CASE
    opt = make_opt("trba")
    net = DERNet(opt)
    for c in classes:
        net.update_fc(opt.hidden_size, c)
        net.build_prediction(opt, c)
        net.build_aux_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed)
    keys(d, p, net)
    image, tgt, _, _ = targets("der_trba", True, classes, seed)
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
    for kind in ("crnn", "trba"):
        mrn_case(d, kind)
    der_case(d)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(G.OUT, "many_tasks.npz")
    np.savez_compressed(path, **d)
    print("many_tasks ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
