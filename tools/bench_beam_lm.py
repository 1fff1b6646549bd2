"""Decoding time of one evaluation batch of a CTC head by the device beam decoder without a language model (mrn_ctc_beam_decode_f32,
the baseline: that entry point is unchanged by the fusion), with a bigram model and with a trigram model (mrn_ctc_beam_lm_decode_f32,
one launch per batch either way), in one process; then a validation() batch of CRNN x 3 with and without the model.

    python tools/bench_beam_lm.py [--batch 256] [--rounds 3] [--reps 10] [--top-n 15] [--no-validation]

The shapes of tools/bench_beam.py: T = 63 with C = 2091, T = 127 with C = 5374; beam widths 4, 8 and 16; the same seeded logits.  Two
model sizes, both built here from synthetic text over the head's classes (a random successor table followed with probability 0.7, so
some n-grams are frequent and most contexts of the search are unseen): 2 000 texts and 50 000 texts of up to 12 characters.  Per
round the three decoders alternate; each is timed by a host clock around `reps` calls that end in a device synchronise, the model on
the device already (validation() uploads it once per call).  The added cost is the fused decoder's time over the baseline's of the
same round.  Prints one JSON line; needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrn_amd import ops  # noqa: E402
from mrn_amd.modules import char_lm  # noqa: E402
from mrn_amd.modules import decoding as D  # noqa: E402
from tools.bench_beam import device_ms, make_logits  # noqa: E402

MODEL_TEXTS = {"small": 2_000, "large": 50_000}
ALPHA, BETA = D.DEFAULT_LM_WEIGHT, D.DEFAULT_LM_BONUS


def synthetic_rows(C, n_texts, seed, max_len=12):
    rng = np.random.default_rng(seed)
    follow = rng.integers(1, C, size=C)
    lengths = rng.integers(1, max_len + 1, size=n_texts)
    rows = []
    for n in lengths:
        jump = rng.random(int(n)) >= 0.7
        fresh = rng.integers(1, C, size=int(n))
        row = [int(fresh[0])]
        for i in range(1, int(n)):
            row.append(int(fresh[i]) if jump[i] else int(follow[row[-1]]))
        rows.append(row)
    return rows


def validation_ms(B, rounds, W, K):
    """host milliseconds of a whole validation() call on one batch of CRNN x 3 (imgW = 256), routed evaluation: best path, the beam
    decoder, the beam decoder with a trigram model"""
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.test import validation
    from mrn_amd.tools import weights as Wt
    from mrn_amd.tools.utils import CTCLabelConverter
    chars = "abcdefghijklmnopqrstuvwxyz0123456789"

    def opt(**kw):
        return types.SimpleNamespace(Transformation="None", FeatureExtraction="VGG", SequenceModeling="BiLSTM", Prediction="CTC",
                                     num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                                     batch_max_length=25, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        conv = CTCLabelConverter(chars)
        net = MRNNet(opt())
        for _ in range(3):
            net.update_fc(256, len(conv.character))
            net.build_prediction(net.opt, len(conv.character))
    Wt.fill_state_dict(net.state_dict(), seed=11)
    net = net.cuda().eval()
    image = torch.from_numpy(Wt.smooth_image("bench_beam_lm", (B, 4, 32, 256), 11))
    batch = [(image, ["label"] * B)]
    rng = np.random.default_rng(3)
    texts = ["".join(chars[i] for i in rng.integers(0, len(chars), size=int(rng.integers(1, 13)))) for _ in range(2000)]
    lm = char_lm.build_char_lm(conv, texts, order=3)
    beam = {"ctc_decode": "beam", "beam_width": W, "beam_top_n": K}
    out = {}
    for name, kw in (("greedy", {}), ("beam", beam), ("beam_trigram", {**beam, "ctc_lm": lm})):
        times = []
        with torch.no_grad():
            validation(net, None, batch, conv, opt(**kw), val_choose="TF")                  # warm-up
            for _ in range(rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                validation(net, None, batch, conv, opt(**kw), val_choose="TF")
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
        out[name] = [round(t, 3) for t in times]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--top-n", type=int, default=D.DEFAULT_BEAM_TOP_N)
    ap.add_argument("--no-validation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_lm needs a GPU: a decoding time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B, K = args.batch, args.top_n
    out = {"batch": B, "rounds": args.rounds, "reps": args.reps, "top_n": K, "lm_weight": ALPHA, "lm_bonus": BETA,
           "unit": "ms per batch", "models": {}, "shapes": {}}
    for T, C in ((63, 2091), (127, 5374)):
        x = make_logits(B, T, C, seed=T)
        handles = {}
        for size, n_texts in MODEL_TEXTS.items():
            rows = synthetic_rows(C, n_texts, seed=C + n_texts)
            for order in (2, 3):
                lm = char_lm.lm_from_rows(rows, C, order)
                handles[f"{size}_order{order}"] = ops.upload_char_lm(lm, "cuda")
                out["models"][f"C{C}_{size}_order{order}"] = {"texts": n_texts, "stored_ngrams": len(lm.bigrams) + len(lm.trigrams),
                                                              "table_slots": len(lm.keys), "max_probe": int(lm.max_probe)}
        for W in (4, 8, 16):
            assert D.beam_supported("CTC", T, C, W, K)
            decoders = {"no_lm": lambda: ops.ctc_beam_decode(x, W, K)}
            for name, h in handles.items():
                decoders[name] = lambda h=h: ops.ctc_beam_decode(x, W, K, h, ALPHA, BETA)
            for fn in decoders.values():                                  # warm-up: code objects, allocator
                fn()
                fn()
            ms = {name: [] for name in decoders}
            for _ in range(args.rounds):
                for name, fn in decoders.items():
                    ms[name].append(device_ms(fn, args.reps))
            plain = ops.ctc_beam_decode(x, W, K)
            zero = ops.ctc_beam_decode(x, W, K, handles["small_order3"], 0.0, 0.0)
            same = all(torch.equal(a, b) for a, b in zip(plain, zero))
            line = {f"{name}_ms": [round(v, 4) for v in vals] for name, vals in ms.items()}
            line["added_ms_over_no_lm"] = {name: [round(v - p, 4) for v, p in zip(vals, ms["no_lm"])] for name, vals in ms.items()
                                           if name != "no_lm"}
            line["zero_weights_equal_no_lm_bit_for_bit"] = same
            out["shapes"][f"T{T}_C{C}_W{W}"] = line
    if not args.no_validation:
        out["validation_crnn3_ms"] = validation_ms(B, args.rounds, 8, K)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
