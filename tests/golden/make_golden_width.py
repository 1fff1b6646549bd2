"""Reference outputs at input widths other than 256 (CPU, the reference implementation), for tests/test_width_cpu.py.

    python tests/golden/make_golden_width.py

Imports the reference and the weight generator exactly as make_golden.py does (it is imported from there).  The reference's MRNNet
hard-codes the router's patch count for 256-pixel lines (63 / 64 / 65); every other module of it takes opt.imgW as it comes.  The
only shim here: net.patch is set to the real frame count (imgW / 4 - 1 for VGG, imgW / 4 + 1 for ResNet) before the first
update_fc, so that `route` and the router's token axis have the size the feature has.  For TRBA and CRNN MRNNets of two experts at
32 x 128, 32 x 512, 48 x 320 and 64 x 192 (B = 4) it stores: the TPS constants and the rectified image, expert 0's pooled
visual feature (permute + AdaptiveAvgPool2d((None, 1)) + squeeze of reference modules/model.py:92), the loop-A logits / loss / a few
parameter gradients of the newest expert, the loop-B fused logits and routing weights, and the eval-mode routing / greedy indices.
Large tensors are stored as make_golden.put's strided subsample plus moments.  Writes tests/golden/width.npz.
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

CASES = {"trba": (("TPS", "ResNet", "BiLSTM", "Attn"), (41, 71)), "crnn": (("None", "VGG", "BiLSTM", "CTC"), (40, 70))}
GRAD_KEYS = {"trba": ("model.1.model.FeatureExtraction.ConvNet.conv4_2.weight", "model.1.model.FeatureExtraction.ConvNet.bn4_2.weight",
                      "model.1.model.Transformation.LocalizationNetwork.localization_fc2.weight", "model.1.fc.weight"),
             "crnn": ("model.1.model.FeatureExtraction.ConvNet.18.weight", "model.1.model.FeatureExtraction.ConvNet.12.weight",
                      "model.1.model.SequenceModeling.0.linear.weight", "model.1.fc.weight")}
B = 4


GEOMETRIES = ((32, 128), (32, 512), (48, 320), (64, 192))


def make_opt(kind, imgH, imgW):
    o = types.SimpleNamespace(num_fiducial=20, imgH=imgH, imgW=imgW, input_channel=4, output_channel=512, hidden_size=256,
                              batch_max_length=25)
    o.Transformation, o.FeatureExtraction, o.SequenceModeling, o.Prediction = CASES[kind][0]
    return o


def targets(kind, imgH, imgW, classes, seed):
    """(image, attention text [B,27] or CTC labels [B,25] + lengths): the same generator calls as tests/test_width_cpu.py"""
    image = torch.from_numpy(W.smooth_image(f"width:{kind}:{imgH}x{imgW}", (B, 4, imgH, imgW), seed))
    if kind == "trba":
        text = torch.from_numpy(W.randint(f"width:text:{imgH}x{imgW}", (B, 27), 4, classes[-1], seed))
        text[:, 0] = 2
        return image, text, None
    lens = torch.from_numpy(W.randint(f"width:len:{imgH}x{imgW}", (B,), 1, 26, seed)).int()
    labels = torch.from_numpy(W.randint(f"width:ctc:{imgH}x{imgW}", (B, 25), 4, classes[-1], seed))
    labels[torch.arange(25)[None, :] >= lens[:, None]] = 1
    return image, labels, lens


def case(d, kind, imgH, imgW, seed):
    p = f"{kind}{imgH}x{imgW}/"
    opt = make_opt(kind, imgH, imgW)
    classes = CASES[kind][1]
    net = MRNNet(opt)
    net.patch = imgW // 4 + (1 if opt.FeatureExtraction == "ResNet" else -1)      # (the shim: see the module docstring)
    for c in classes:
        net.update_fc(opt.hidden_size, c)
        net.build_prediction(opt, c)
    W.fill_state_dict(net.state_dict(), seed)
    sd0 = net.state_dict()
    d[p + "sd_keys"] = np.array(sorted(sd0.keys()))
    d[p + "sd_shapes"] = np.array([",".join(map(str, sd0[k].shape)) for k in sorted(sd0.keys())])
    image, tgt, lens = targets(kind, imgH, imgW, classes, seed)
    attn = kind == "trba"
    ce = torch.nn.CrossEntropyLoss(ignore_index=1)
    ctc = torch.nn.CTCLoss(reduction="mean", zero_infinity=True)

    def clf_loss(preds):
        if attn:
            return ce(preds.reshape(-1, preds.shape[-1]), tgt[:, 1:].reshape(-1))
        return ctc(preds.log_softmax(2).permute(1, 0, 2), tgt, torch.IntTensor([preds.size(1)] * B), lens)

    # expert 0 in train mode: TPS constants, rectified image, pooled visual feature
    net.train()
    m0 = net.model[0].model
    with torch.no_grad():
        x = image
        if attn:
            gg = m0.Transformation.GridGenerator
            put(d, p + "tps/inv_delta_C", gg.inv_delta_C, full=True)
            put(d, p + "tps/P_hat", gg.P_hat)
            x = m0.Transformation(image)
            put(d, p + "tps_out", x)
        fm = m0.FeatureExtraction(x)
        d[p + "featmap_shape"] = np.array(fm.shape, dtype=np.int64)
        put(d, p + "visual", m0.AdaptiveAvgPool(fm.permute(0, 3, 1, 2)).squeeze(3))
    W.fill_state_dict(net.state_dict(), seed)            # (the running statistics moved)

    # loop A: the newest expert alone, train mode, loss and gradients
    net.train()
    net.zero_grad()
    preds = net(image, False, tgt[:, :-1] if attn else None)["logits"]
    loss = clf_loss(preds)
    loss.backward()
    put(d, p + "stepA/logits", preds)
    d[p + "stepA/loss"] = np.float64(loss.item())
    grads = dict(net.named_parameters())
    for k in GRAD_KEYS[kind]:
        put(d, p + "stepA/grad/" + k, grads[k].grad)
    W.fill_state_dict(net.state_dict(), seed)

    # loop B forward: fused logits and routing weights, experts in train mode
    with torch.no_grad():
        out = net(image, True, tgt[:, :-1] if attn else None, True)
        put(d, p + "stepB/weights", out["index"], full=True)
        put(d, p + "stepB/logits", out["logits"])
    W.fill_state_dict(net.state_dict(), seed)

    # eval mode: hard routing, greedy decoding
    net.eval()
    with torch.no_grad():
        sos = torch.LongTensor(B).fill_(2) if attn else None
        oe = net(image, True, sos, False)
        d[p + "eval/index"] = oe["index"].numpy()
        put(d, p + "eval/logits", oe["logits"])
        d[p + "eval/argmax"] = oe["logits"].max(2)[1].numpy()


if __name__ == "__main__":
    torch.set_num_threads(8)
    d = {}
    for kind, seed in (("trba", 61), ("crnn", 62)):
        for imgH, imgW in GEOMETRIES:
            case(d, kind, imgH, imgW, seed)
    path = os.path.join(G.OUT, "width.npz")
    np.savez_compressed(path, **d)
    print("width ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
