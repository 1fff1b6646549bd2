"""Time of scoring one evaluation batch against per-image word lists on the attention head: the fused scorer
(mrn_attn_score_candidates_*, one launch per eight experts), its stepwise form (Attention.score_candidates under MRN_ATTN_BEAM=stepwise:
the teacher-forced decoder on the B * K rows), and the two ways the protocol ran before -- the lexicon-constrained beam search on the
UNION of the lists (one launch, a different experiment) and one constrained search per image (timed on a few images, reported per
image) -- in one process; then a validation() batch of TRBA x 6 with and without opt.candidates.

    python tools/bench_candidates.py [--batch 256] [--slots 50] [--rounds 3] [--reps 5] [--images 8] [--no-validation]

B = 256, T = 65, D = 256, S = 26, K = 50; one expert (2091 classes) and six (97, 203, 331, 1045, 2091, 5374), the x3 and the exact
form.  Every image draws its K words from a table of 10 000 random words of 3 ... 12 characters over the 2091-class alphabet (a
character with probability 0.5 one of the first 32 classes, so that the smallest expert can spell some of the words).  The heads are
randomly initialised with the generator scaled by 20; the features are random.  Per round the paths alternate, each timed by a host
clock around `reps` calls that end in a device synchronise.  Prints one JSON line; needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrn_amd import ops  # noqa: E402
from mrn_amd.modules import decoding  # noqa: E402
from tools.bench_attn_beam import CLASSES, D, EOS, HID, S, SOS, T, device_ms, heads  # noqa: E402

WORDS = 10000
WIDTH = 8


def random_words(words, classes, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(3, 13, words).astype(np.int32)
    near = rng.random((words, 12)) < 0.5
    tokens = np.where(near, rng.integers(4, 36, (words, 12)), rng.integers(4, classes, (words, 12))).astype(np.int32)
    return tokens, lengths


def scorers(atts, Hb, handle, tokens, lengths, images):
    """(fused, stepwise, union-list beam, per-image beam) closures on G heads and features [G,B,T,D]"""
    G, B = Hb.shape[:2]
    start = torch.tensor([SOS], dtype=torch.int64, device="cuda")
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
    w_inv = cols[9] if cols[9][0] is not None else None
    union = np.unique(handle.cand[handle.cand >= 0])
    union_trie = ops.upload_trie(decoding.build_trie(tokens[union], lengths[union]), "cuda")
    own = [ops.upload_trie(decoding.build_trie(tokens[row[row >= 0]], lengths[row[row >= 0]]), "cuda") for row in handle.cand[:images]]

    def fused():
        return ops.attn_score_candidates_grouped(Hb, Hproj, cols[0], start, *cols[1:9], HID, S, EOS, handle.tokens_dev, handle.lengths_dev,
                                                 handle.cand_dev, n=1, w_inv=w_inv, check=False)

    def stepwise():
        os.environ["MRN_ATTN_BEAM"] = "stepwise"
        try:
            return [a.score_candidates(Hb[g], start, EOS, handle, S - 1) for g, a in enumerate(atts)]
        finally:
            del os.environ["MRN_ATTN_BEAM"]

    def union_beam():
        return ops.attn_lexicon_decode_grouped(Hb, Hproj, cols[0], start, *cols[1:9], HID, S, EOS, WIDTH, union_trie, w_inv=w_inv)

    def per_image():
        for b, trie in enumerate(own):
            ops.attn_lexicon_decode_grouped(Hb[:, b:b + 1].contiguous(), Hproj[:, b:b + 1].contiguous(), cols[0], start, *cols[1:9], HID, S,
                                            EOS, WIDTH, trie, w_inv=w_inv)

    return fused, stepwise, union_beam, per_image


def validation_ms(B, K, rounds):
    """infer_time of validation() on one batch of TRBA x 6 (imgW = 256): greedy, and opt.candidates with K words per image"""
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.test import validation
    from mrn_amd.tools import weights as Wt
    from mrn_amd.tools.utils import AttnLabelConverter
    chars = "abcdefghijklmnopqrstuvwxyz0123456789"
    rng = np.random.default_rng(5)
    table = ["".join(chars[k] for k in rng.integers(0, len(chars), int(rng.integers(3, 13)))) for _ in range(WORDS)]
    labels = [f"label{b}" for b in range(B)]
    lists = {gt: [table[i] for i in rng.integers(0, WORDS, K)] for gt in labels}

    def opt(**kw):
        return types.SimpleNamespace(Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM", Prediction="Attn",
                                     num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                                     batch_max_length=25, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt())
        for _ in range(6):
            net.update_fc(256, 5 + len(chars))
            net.build_prediction(net.opt, 5 + len(chars))
        conv = AttnLabelConverter(chars)
    Wt.fill_state_dict(net.state_dict(), seed=11)
    net = net.cuda().eval()
    image = torch.from_numpy(Wt.smooth_image("bench_attn_beam", (B, 4, 32, 256), 11))
    batch = [(image, labels)]
    out = {}
    for name, kw in (("greedy", {}), (f"candidates_K{K}", {"candidates": lists})):
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
    ap.add_argument("--slots", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--no-validation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_candidates needs a GPU: a scoring time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B, K = args.batch, args.slots
    out = {"batch": B, "T": T, "D": D, "S": S, "K": K, "words": WORDS, "beam_width": WIDTH, "rounds": args.rounds, "reps": args.reps,
           "unit": "ms per batch", "shapes": {}}
    tokens, lengths = random_words(WORDS, 2091, seed=WORDS)
    cand = np.random.default_rng(3).integers(0, WORDS, (B, K)).astype(np.int32)
    handle = ops.upload_words(tokens, lengths, "cuda", 1).with_cand(cand, S)
    default_x3 = ops.DECODER_X3
    for x3 in (True, False):
        ops.DECODER_X3 = x3
        for G, classes in CLASSES.items():
            atts = heads(classes, seed=G)
            Hb = (torch.rand(G, B, T, D, generator=torch.Generator().manual_seed(7 + G)) * 2 - 1).cuda()
            fused, stepwise, union_beam, per_image = scorers(atts, Hb, handle, tokens, lengths, args.images)
            for fn in (fused, stepwise, union_beam, per_image):             # warm-up: code objects, allocator, packed weights
                fn()
            f_ms, s_ms, u_ms, i_ms = [], [], [], []
            for _ in range(args.rounds):
                f_ms.append(device_ms(fused, args.reps))
                s_ms.append(device_ms(stepwise, 1))
                u_ms.append(device_ms(union_beam, args.reps))
                i_ms.append(device_ms(per_image, 1) / args.images)
            a, b = fused(), stepwise()
            same = sum(int((a[0][g][:, 0] == b[g][0][:, 0]).sum()) for g in range(G))
            out["shapes"][f"G{G}_{'x3' if x3 else 'f32'}"] = {
                "fused_ms": [round(v, 3) for v in f_ms], "stepwise_ms": [round(v, 2) for v in s_ms],
                "union_list_beam_ms": [round(v, 3) for v in u_ms], "one_beam_call_per_image_ms_per_image": [round(v, 3) for v in i_ms],
                "samples_with_the_same_best_word": f"{same}/{G * B}", "live_slots": f"{int((a[2] > float('-inf')).sum())}/{G * B * K}"}
            del atts, Hb
    ops.DECODER_X3 = default_x3
    if not args.no_validation:
        out["validation_trba6_infer_ms"] = validation_ms(B, K, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
