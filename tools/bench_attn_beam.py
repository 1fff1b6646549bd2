"""Decoding time of one evaluation batch on the attention head: the fused greedy decoder (mrn_attn_greedy_decode*_grouped), the fused
beam decoder (mrn_attn_beam_decode_*, one launch per eight experts) and the stepwise beam decoder (Attention.beam_search under
MRN_ATTN_BEAM=stepwise: five launches per step and expert on the B * W-row batch), in one process; then a validation() batch of TRBA x 6
decoded greedily and by beam search.

    python tools/bench_attn_beam.py [--batch 256] [--rounds 3] [--reps 5] [--no-validation]

B = 256, T = 65, D = 256, S = 26; one expert (2091 classes) and six (97, 203, 331, 1045, 2091, 5374); beam widths 1, 4 and 8.  The
heads are randomly initialised with the generator scaled by 20 (peaked distributions, as after training); the features are random.
Per round the three paths alternate, each timed by a host clock around `reps` calls that end in a device synchronise.  Also the
number of samples whose best entry agrees between the fused and the stepwise form.  Prints one JSON line; needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import types

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrn_amd import ops  # noqa: E402
from mrn_amd.modules.prediction import Attention  # noqa: E402

HID, T, D, S, SOS, EOS = 256, 65, 256, 26, 2, 3
CLASSES = {1: (2091,), 6: (97, 203, 331, 1045, 2091, 5374)}


def device_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def heads(classes, seed):
    torch.manual_seed(seed)
    out = []
    for C in classes:
        att = Attention(D, HID, C, nn.Linear(HID, C))
        with torch.no_grad():
            att.generator.weight.mul_(20.0)
        out.append(att.cuda().eval())
    return out


def decoders(atts, Hb, W):
    """(greedy, fused beam, stepwise beam) closures on G heads and features [G,B,T,D]"""
    G, B = Hb.shape[:2]
    start = torch.tensor([SOS], dtype=torch.int64, device="cuda")
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
    w_inv = cols[9] if cols[9][0] is not None else None
    logits = [ops.padded_rows(B, S, a.num_class, Hb.device) for a in atts]

    def greedy():
        ops.attn_greedy_decode_grouped(Hb, Hproj, cols[0], start, *cols[1:9], HID, S, logits, w_inv=w_inv)

    def fused():
        return ops.attn_beam_decode_grouped(Hb, Hproj, cols[0], start, *cols[1:9], HID, S, EOS, W, w_inv=w_inv)

    def stepwise():
        os.environ["MRN_ATTN_BEAM"] = "stepwise"
        try:
            return [a.beam_search(Hb[g], start, EOS, W, S - 1) for g, a in enumerate(atts)]
        finally:
            del os.environ["MRN_ATTN_BEAM"]

    return greedy, fused, stepwise


def validation_ms(B, rounds, widths):
    """infer_time of validation() on one batch of TRBA x 6 (imgW = 256): greedy, then attn_decode="beam" at every width"""
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.test import validation
    from mrn_amd.tools import weights as Wt
    from mrn_amd.tools.utils import AttnLabelConverter
    chars = "abcdefghijklmnopqrstuvwxyz0123456789"

    def opt(**kw):
        return types.SimpleNamespace(Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM", Prediction="Attn",
                                     num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                                     batch_max_length=25, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt())
        for _ in range(6):
            net.update_fc(256, 5 + len(chars))
            net.build_prediction(net.opt, 5 + len(chars))
    Wt.fill_state_dict(net.state_dict(), seed=11)
    net = net.cuda().eval()
    image = torch.from_numpy(Wt.smooth_image("bench_attn_beam", (B, 4, 32, 256), 11))
    batch = [(image, ["label"] * B)]
    conv = AttnLabelConverter(chars)
    out = {}
    for name, kw in [("greedy", {})] + [(f"beam_W{W}", {"attn_decode": "beam", "beam_width": W}) for W in widths]:
        times = []
        with torch.no_grad():
            validation(net, None, batch, conv, opt(**kw), val_choose="TF")                  # warm-up
            for _ in range(rounds):
                times.append(1e3 * validation(net, None, batch, conv, opt(**kw), val_choose="TF")[6])
        out[name] = [round(t, 3) for t in times]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-validation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_beam needs a GPU: a decoding time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B = args.batch
    out = {"batch": B, "T": T, "D": D, "S": S, "rounds": args.rounds, "reps": args.reps, "unit": "ms per batch", "shapes": {}}
    for G, classes in CLASSES.items():
        atts = heads(classes, seed=G)
        Hb = (torch.rand(G, B, T, D, generator=torch.Generator().manual_seed(7 + G)) * 2 - 1).cuda()
        for W in (1, 4, 8):
            greedy, fused, stepwise = decoders(atts, Hb, W)
            for fn in (greedy, fused, stepwise):                     # warm-up: code objects, allocator, packed weights
                fn()
            g_ms, f_ms, s_ms = [], [], []
            for _ in range(args.rounds):
                g_ms.append(device_ms(greedy, args.reps))
                f_ms.append(device_ms(fused, args.reps))
                s_ms.append(device_ms(stepwise, max(1, args.reps // 5)))
            a, b = fused(), stepwise()
            same = sum(int(torch.equal(a[4][g], b[g][4])) for g in range(G))
            rows = sum(int((a[4][g] == b[g][4]).all(dim=1).sum()) for g in range(G))
            out["shapes"][f"G{G}_W{W}"] = {"greedy_ms": [round(v, 3) for v in g_ms], "fused_beam_ms": [round(v, 3) for v in f_ms],
                                           "stepwise_beam_ms": [round(v, 2) for v in s_ms], "experts_with_the_same_best_paths": f"{same}/{G}",
                                           "samples_with_the_same_best_path": f"{rows}/{G * B}"}
        del atts, Hb
    if not args.no_validation:
        out["validation_trba6_infer_ms"] = validation_ms(B, args.rounds, (4, 8))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
