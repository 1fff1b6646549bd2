"""Decoding time of one evaluation batch on the attention head with and without a character n-gram model in the beam search: the
plain fused beam launch (mrn_attn_beam_decode_*) and the launch fused with the model (mrn_attn_beam_lm_decode_*), alternating in one
process; then a validation() batch of TRBA x 6 decoded by beam search without and with opt.attn_lm.

    python tools/bench_attn_beam_lm.py [--batch 256] [--rounds 3] [--reps 5] [--no-validation]

The shapes of tools/bench_attn_beam.py: B = 256, T = 65, D = 256, S = 26; one expert (2091 classes) and six (97, 203, 331, 1045, 2091,
5374); beam widths 4 and 8; a bigram and a trigram model over 97 classes (lm_from_rows on 2000 seeded random rows), lm_weight 0.3,
top_n 15 (so an entry proposes 15 classes where the plain launch proposes W).  The heads are randomly initialised with the generator
scaled by 20; the features are random.  Per round the paths alternate, each timed by a host clock around `reps` calls that end in a
device synchronise.  Also whether the launch with zero weights returns the plain launch's outputs bit for bit at the timed size.
Prints one JSON line; needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrn_amd import ops  # noqa: E402
from mrn_amd.modules.char_lm import build_char_lm, lm_from_rows  # noqa: E402
from tools.bench_attn_beam import CLASSES, D, EOS, HID, S, SOS, T, device_ms, heads  # noqa: E402

LM_WEIGHT, LM_BONUS, TOP_N, C_LM = 0.3, 0.05, 15, 97


def model(order, seed=3, rows=2000):
    rng = np.random.default_rng(seed)
    return lm_from_rows([rng.integers(4, C_LM, size=int(rng.integers(1, 12))).tolist() for _ in range(rows)], C_LM, order)


def decoders(atts, Hb, W, handles):
    """(plain beam, {order: beam with the model}, beam with the model at zero weights) closures on G heads and features [G,B,T,D]"""
    start = torch.tensor([SOS], dtype=torch.int64, device="cuda")
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
    w_inv = cols[9] if cols[9][0] is not None else None
    common = (Hb, Hproj, cols[0], start, *cols[1:9], HID, S, EOS, W)

    def plain():
        return ops.attn_beam_decode_grouped(*common, w_inv=w_inv)

    def fused(handle, alpha=LM_WEIGHT, beta=LM_BONUS):
        return ops.attn_beam_lm_decode_grouped(*common, handle, alpha, beta, TOP_N, w_inv=w_inv)

    return plain, {order: (lambda h=h: fused(h)) for order, h in handles.items()}, lambda: fused(handles[3], 0.0, 0.0)


def validation_ms(B, rounds, widths):
    """infer_time of validation() on one batch of TRBA x 6 (imgW = 256): attn_decode="beam" at every width, without and with attn_lm"""
    import contextlib
    import io
    import types
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.test import validation
    from mrn_amd.tools import weights as Wt
    from mrn_amd.tools.utils import AttnLabelConverter
    chars = "abcdefghijklmnopqrstuvwxyz0123456789"

    def opt(**kw):
        return types.SimpleNamespace(Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM", Prediction="Attn",
                                     num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                                     batch_max_length=25, attn_decode="beam", **kw)
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
    rng = np.random.default_rng(5)
    lm = build_char_lm(conv, ["".join(rng.choice(list(chars), size=int(rng.integers(1, 12)))) for _ in range(2000)], order=3)
    runs = [(f"beam_W{W}", {"beam_width": W}) for W in widths] + [(f"beam_lm_W{W}", {"beam_width": W, "attn_lm": lm, "lm_weight": LM_WEIGHT})
                                                                   for W in widths]
    out = {name: [] for name, _ in runs}
    with torch.no_grad():
        for name, kw in runs:
            validation(net, None, batch, conv, opt(**kw), val_choose="TF")                      # warm-up
        for _ in range(rounds):
            for name, kw in runs:                                                               # (alternating)
                out[name].append(round(1e3 * validation(net, None, batch, conv, opt(**kw), val_choose="TF")[6], 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-validation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_beam_lm needs a GPU: a decoding time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B = args.batch
    handles = {order: ops.upload_char_lm(model(order), "cuda") for order in (2, 3)}
    out = {"batch": B, "T": T, "D": D, "S": S, "rounds": args.rounds, "reps": args.reps, "top_n": TOP_N, "lm_weight": LM_WEIGHT,
           "unit": "ms per batch", "shapes": {}}
    for G, classes in CLASSES.items():
        atts = heads(classes, seed=G)
        Hb = (torch.rand(G, B, T, D, generator=torch.Generator().manual_seed(7 + G)) * 2 - 1).cuda()
        for W in (4, 8):
            plain, fused, zero = decoders(atts, Hb, W, handles)
            for fn in (plain, fused[2], fused[3], zero):                 # warm-up: code objects, allocator, packed weights
                fn()
            ms = {"plain_beam_ms": [], "bigram_ms": [], "trigram_ms": []}
            for _ in range(args.rounds):
                ms["plain_beam_ms"].append(device_ms(plain, args.reps))
                ms["bigram_ms"].append(device_ms(fused[2], args.reps))
                ms["trigram_ms"].append(device_ms(fused[3], args.reps))
            a, z, f = plain(), zero(), fused[3]()
            row = {k: [round(v, 3) for v in vs] for k, vs in ms.items()}
            row["zero_weights_equal_the_plain_launch"] = all(torch.equal(x, y) for x, y in zip(a, z))
            row["samples_whose_best_path_the_trigram_changes"] = f"{int((a[4] != f[4]).any(dim=2).sum())}/{G * B}"
            out["shapes"][f"G{G}_W{W}"] = row
        del atts, Hb
    if not args.no_validation:
        out["validation_trba6_infer_ms"] = validation_ms(B, args.rounds, (4, 8))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
