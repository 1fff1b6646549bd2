"""Decoding time of one evaluation batch on the attention head with a lexicon: the fused greedy decoder, the fused (unconstrained) beam
decoder (mrn_attn_beam_decode_*), the fused lexicon-constrained decoder (mrn_attn_lexicon_decode_*, one launch per eight experts and one
trie for all of them), its stepwise form (Attention.lexicon_search under MRN_ATTN_BEAM=stepwise) and the float64 host form
(decoding.attn_lexicon_host, at a small batch), in one process; then a validation() batch of TRBA x 6 with and without opt.attn_lexicon.

    python tools/bench_attn_lexicon.py [--batch 256] [--rounds 3] [--reps 5] [--host-batch 4] [--no-validation]

B = 256, T = 65, D = 256, S = 26; one expert (2091 classes) and six (97, 203, 331, 1045, 2091, 5374); beam widths 4 and 8; lexicons of
1 000 and 50 000 random words of 3 ... 12 characters over the 2091-class alphabet (a character with probability 0.5 one of the first
32 classes, so that prefixes are shared and the smallest expert can spell some of the words).  The heads are randomly initialised with
the generator scaled by 20; the features are random.  Per round the paths alternate, each timed by a host clock around `reps` calls
that end in a device synchronise.  The comparison that matters is the constrained launch against the beam launch at the same shape.
Prints one JSON line; needs a GPU.
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
from mrn_amd.modules import decoding  # noqa: E402
from tools.bench_attn_beam import CLASSES, D, EOS, HID, S, SOS, T, device_ms, heads  # noqa: E402

LEXICONS = (1000, 50000)
WIDTHS = (4, 8)


def random_trie(words, classes, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(3, 13, words).astype(np.int32)
    near = rng.random((words, 12)) < 0.5
    tokens = np.where(near, rng.integers(4, 36, (words, 12)), rng.integers(4, classes, (words, 12))).astype(np.int32)
    return decoding.build_trie(tokens, lengths)


def decoders(atts, Hb, W, handle):
    """(greedy, fused beam, fused lexicon, stepwise lexicon) closures on G heads and features [G,B,T,D]"""
    G, B = Hb.shape[:2]
    start = torch.tensor([SOS], dtype=torch.int64, device="cuda")
    with torch.no_grad():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
    w_inv = cols[9] if cols[9][0] is not None else None
    logits = [ops.padded_rows(B, S, a.num_class, Hb.device) for a in atts]

    def greedy():
        ops.attn_greedy_decode_grouped(Hb, Hproj, cols[0], start, *cols[1:9], HID, S, logits, w_inv=w_inv)

    def beam():
        return ops.attn_beam_decode_grouped(Hb, Hproj, cols[0], start, *cols[1:9], HID, S, EOS, W, w_inv=w_inv)

    def lexicon():
        return ops.attn_lexicon_decode_grouped(Hb, Hproj, cols[0], start, *cols[1:9], HID, S, EOS, W, handle, w_inv=w_inv)

    def stepwise():
        os.environ["MRN_ATTN_BEAM"] = "stepwise"
        try:
            return [a.lexicon_search(Hb[g], start, EOS, W, handle, S - 1) for g, a in enumerate(atts)]
        finally:
            del os.environ["MRN_ATTN_BEAM"]

    return greedy, beam, lexicon, stepwise


def validation_ms(B, rounds, width, words):
    """infer_time of validation() on one batch of TRBA x 6 (imgW = 256): greedy, attn_decode="beam", and opt.attn_lexicon"""
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.test import validation
    from mrn_amd.tools import weights as Wt
    from mrn_amd.tools.utils import AttnLabelConverter
    chars = "abcdefghijklmnopqrstuvwxyz0123456789"
    rng = np.random.default_rng(5)
    lexicon = ["".join(chars[k] for k in rng.integers(0, len(chars), int(rng.integers(3, 13)))) for _ in range(words)]

    def opt(**kw):
        return types.SimpleNamespace(Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM", Prediction="Attn",
                                     num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                                     batch_max_length=25, beam_width=width, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt())
        for _ in range(6):
            net.update_fc(256, 5 + len(chars))
            net.build_prediction(net.opt, 5 + len(chars))
        conv = AttnLabelConverter(chars)
    Wt.fill_state_dict(net.state_dict(), seed=11)
    net = net.cuda().eval()
    image = torch.from_numpy(Wt.smooth_image("bench_attn_beam", (B, 4, 32, 256), 11))
    batch = [(image, ["label"] * B)]
    out = {}
    for name, kw in (("greedy", {}), (f"beam_W{width}", {"attn_decode": "beam"}), (f"lexicon_{words}_W{width}", {"attn_lexicon": lexicon})):
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
    ap.add_argument("--host-batch", type=int, default=4)
    ap.add_argument("--no-validation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_lexicon needs a GPU: a decoding time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B = args.batch
    out = {"batch": B, "T": T, "D": D, "S": S, "rounds": args.rounds, "reps": args.reps, "unit": "ms per batch", "tries": {}, "shapes": {}}
    handles = {}
    for N in LEXICONS:
        t0 = time.perf_counter()
        trie = random_trie(N, 2091, seed=N)
        built = time.perf_counter() - t0
        t0 = time.perf_counter()
        handles[N] = ops.upload_trie(trie, "cuda")
        torch.cuda.synchronize()
        out["tries"][str(N)] = {"nodes": handles[N].nodes, "root_children": int(trie.child_off[1]), "depth": trie.depth,
                                "build_ms": round(1e3 * built, 1), "check_and_upload_ms": round(1e3 * (time.perf_counter() - t0), 1)}
    for G, classes in CLASSES.items():
        atts = heads(classes, seed=G)
        Hb = (torch.rand(G, B, T, D, generator=torch.Generator().manual_seed(7 + G)) * 2 - 1).cuda()
        for W in WIDTHS:
            for N in LEXICONS:
                greedy, beam, lexicon, stepwise = decoders(atts, Hb, W, handles[N])
                for fn in (greedy, beam, lexicon, stepwise):             # warm-up: code objects, allocator, packed weights
                    fn()
                g_ms, b_ms, l_ms, s_ms = [], [], [], []
                for _ in range(args.rounds):
                    g_ms.append(device_ms(greedy, args.reps))
                    b_ms.append(device_ms(beam, args.reps))
                    l_ms.append(device_ms(lexicon, args.reps))
                    s_ms.append(device_ms(stepwise, 1))
                a, b = lexicon(), stepwise()
                rows = sum(int((a[6][g][:, 0] == b[g][6][:, 0]).sum()) for g in range(G))
                live = int((a[1][:, :, 0] >= 0).sum())
                out["shapes"][f"G{G}_W{W}_N{N}"] = {"greedy_ms": [round(v, 3) for v in g_ms], "fused_beam_ms": [round(v, 3) for v in b_ms],
                                                   "fused_lexicon_ms": [round(v, 3) for v in l_ms],
                                                   "stepwise_lexicon_ms": [round(v, 2) for v in s_ms],
                                                   "samples_with_the_same_best_word": f"{rows}/{G * B}",
                                                   "samples_with_a_live_word": f"{live}/{G * B}"}
        if G == 1:                                                       # the float64 host form, one expert, a small batch
            hb = args.host_batch
            sd = {k: v.detach().cpu() for k, v in atts[0].state_dict().items()}
            t0 = time.perf_counter()
            decoding.attn_lexicon_host(sd, Hb[0, :hb].cpu(), SOS, EOS, 8, S - 1, handles[LEXICONS[0]].trie)
            out["host_form"] = {"batch": hb, "W": 8, "words": LEXICONS[0], "ms": round(1e3 * (time.perf_counter() - t0), 1)}
        del atts, Hb
    if not args.no_validation:
        out["validation_trba6_infer_ms"] = validation_ms(B, args.rounds, 8, 1000)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
