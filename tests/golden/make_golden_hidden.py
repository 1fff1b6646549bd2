"""Reference outputs at hidden sizes other than 256 (CPU, the reference implementation), for tests/test_hidden_cpu.py.

    python tests/golden/make_golden_hidden.py

Imports the reference and the weight generator exactly as make_golden.py does (it is imported from there), and follows
make_golden_width.py: CRNN MRNNets of two experts (classes 40, 70) at hidden_size 128 and 512, 32 x 128 input (T = 31), B = 4 -- with
that generator's one shim, net.patch set to the real frame count before the first update_fc -- and one SVTR MRNNet of two experts at
hidden_size 128, 32 x 256, B = 2, with the DropPath draws injected as make_golden.py injects them.  Per case it stores: the
state-dict keys and shapes, expert 0's contextual feature (train mode), the loop-A logits / loss / four parameter gradients of the
newest expert, the loop-B fused logits and routing weights, and the eval-mode routing index and argmax.  Large tensors are stored as
make_golden.put's strided subsample plus moments.  Writes tests/golden/hidden.npz.
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

STAGES = {"crnn": ("None", "VGG", "BiLSTM", "CTC"), "svtr": ("None", "SVTR", "None", "CTC")}
CLASSES = (40, 70)
# kind, hidden_size, imgW, B, seed
CASES = (("crnn", 128, 128, 4, 71), ("crnn", 512, 128, 4, 72), ("svtr", 128, 256, 2, 73))
GRAD_KEYS = {"crnn": ("model.1.model.SequenceModeling.0.rnn.weight_hh_l0", "model.1.model.SequenceModeling.1.linear.weight",
                      "model.1.model.FeatureExtraction.ConvNet.18.weight", "model.1.fc.weight"),
             "svtr": ("model.1.model.SequenceModeling.0.weight", "model.1.model.FeatureExtraction.ConvNet.patch_embed.proj.0.weight",
                      "model.1.model.FeatureExtraction.ConvNet.blocks3.0.mixer.qkv.weight", "model.1.fc.weight")}


def make_opt(kind, hidden, imgW):
    o = types.SimpleNamespace(num_fiducial=20, imgH=32, imgW=imgW, input_channel=4, output_channel=512, hidden_size=hidden,
                              batch_max_length=25)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = STAGES[kind]
    return o


def targets(kind, hidden, imgW, B, seed):
    """(image, CTC labels [B,25], lengths): the same generator calls as tests/test_hidden_cpu.py"""
    image = torch.from_numpy(W.smooth_image(f"hidden:{kind}:{hidden}", (B, 4, 32, imgW), seed))
    lens = torch.from_numpy(W.randint(f"hidden:len:{kind}:{hidden}", (B,), 1, 26, seed)).int()
    labels = torch.from_numpy(W.randint(f"hidden:ctc:{kind}:{hidden}", (B, 25), 4, CLASSES[-1], seed))
    labels[torch.arange(25)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


def case(d, kind, hidden, imgW, B, seed):
    p = f"{kind}{hidden}/"
    opt = make_opt(kind, hidden, imgW)
    net = MRNNet(opt)
    if kind == "crnn":
        net.patch = imgW // 4 - 1                                  # (the width generator's shim: the real frame count of a VGG line)
    for c in CLASSES:
        net.update_fc(opt.hidden_size, c)
        net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed)
    sd0 = net.state_dict()
    d[p + "sd_keys"] = np.array(sorted(sd0.keys()))
    d[p + "sd_shapes"] = np.array([",".join(map(str, sd0[k].shape)) for k in sorted(sd0.keys())])
    image, tgt, lens = targets(kind, hidden, imgW, B, seed)
    ctc = torch.nn.CTCLoss(reduction="mean", zero_infinity=True)

    def inject(tag, n=1):
        G.DROP_MASKS.clear()
        if kind == "svtr":
            for e in G.drop_masks(B, seed, f"hidden{hidden}:{tag}", n):
                G.DROP_MASKS.extend(e)

    # expert 0 in train mode: the contextual feature
    net.train()
    with torch.no_grad():
        inject("e0")
        put(d, p + "e0/feature", net.model[0](image, None, True)["feature"])
    W.fill_state_dict(net.state_dict(), seed)            # (the running statistics moved)

    # loop A: the newest expert alone, train mode, loss and gradients
    net.zero_grad()
    inject("stepA")
    preds = net(image, False)["logits"]
    loss = ctc(preds.log_softmax(2).permute(1, 0, 2), tgt, torch.IntTensor([preds.size(1)] * B), lens)
    loss.backward()
    put(d, p + "stepA/logits", preds)
    d[p + "stepA/loss"] = np.float64(loss.item())
    grads = dict(net.named_parameters())
    for k in GRAD_KEYS[kind]:
        put(d, p + "stepA/grad/" + k, grads[k].grad)
    W.fill_state_dict(net.state_dict(), seed)

    # loop B forward: fused logits and routing weights, experts in train mode
    with torch.no_grad():
        inject("stepB", len(CLASSES))
        out = net(image, True, None, True)
        put(d, p + "stepB/weights", out["index"], full=True)
        put(d, p + "stepB/logits", out["logits"])
    W.fill_state_dict(net.state_dict(), seed)

    # eval mode: hard routing
    net.eval()
    with torch.no_grad():
        oe = net(image, True, None, False)
        d[p + "eval/index"] = oe["index"].numpy()
        put(d, p + "eval/logits", oe["logits"])
        d[p + "eval/argmax"] = oe["logits"].max(2)[1].numpy()


if __name__ == "__main__":
    torch.set_num_threads(8)
    d = {}
    for c in CASES:
        case(d, *c)
    path = os.path.join(G.OUT, "hidden.npz")
    np.savez_compressed(path, **d)
    print("hidden ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
