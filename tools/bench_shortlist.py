"""Time of the lexicon shortlist (mrn_lexicon_shortlist_i32: the K words of a shared lexicon nearest to every sample's greedy
transcription) and of a validation() batch that decodes with it, in one process:

  * per lexicon size N: ops.lexicon_shortlist on the device against the numpy host form decoding.lexicon_shortlist_host (timed on
    `--host-samples` samples and scaled to the batch: it is linear in the samples);
  * per N, one validation() batch of TRBA x 6 (opt.attn_lexicon) and of CRNN x 3 (opt.lexicon) with opt.lexicon_shortlist = K: the
    forward (infer_time) and the scoring section (mrn_amd.test.SCORE_TIMER), without the per-call encoding and upload of the lexicon;
  * next to those: greedy, the trie beam at W = 8 on the attention head and the exhaustive lexicon decoder on the CTC head for the
    sizes up to `--exhaustive-max`, and opt.candidates with all N words for every image at N = 1000.

    python tools/bench_shortlist.py [--batch 256] [--slots 50] [--words 1000 50000 1048576] [--rounds 3] [--reps 5] [--host-samples 4]
                                    [--exhaustive-max 50000] [--no-validation]

The words are random strings of 3 ... 12 of 36 characters; the hypotheses of the kernel timing are words of the lexicon after up to
two random edits.  The networks are randomly initialised.  Per round the paths alternate, each timed by a host clock around calls that
end in a device synchronise.  Prints one JSON line; needs a GPU.
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
from tools.bench_attn_beam import device_ms  # noqa: E402

CHARS = "abcdefghijklmnopqrstuvwxyz0123456789"
WIDTH = 8


def random_strings(words, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(3, 13, words)
    flat = rng.integers(0, len(CHARS), int(lengths.sum()))
    text = "".join(CHARS[k] for k in flat)
    ends = np.cumsum(lengths)
    return [text[e - n:e] for e, n in zip(ends, lengths)]


def kernel_times(B, K, N, rounds, reps, host_samples):
    """ops.lexicon_shortlist against the host form on a table of N words and B hypotheses of it"""
    rng = np.random.default_rng(N)
    lengths = rng.integers(3, 13, N).astype(np.int32)
    tokens = rng.integers(4, 40, (N, 12)).astype(np.int32)
    picked = rng.integers(0, N, B)
    hyp, hyp_len = tokens[picked].copy(), lengths[picked].copy()
    for b in range(B):                                             # up to two substitutions
        for at in rng.integers(0, 12, int(rng.integers(0, 3))):
            hyp[b, at] = rng.integers(4, 40)
    handle = ops.upload_words(tokens, lengths, "cuda")
    dev = (torch.from_numpy(hyp).cuda(), torch.from_numpy(hyp_len).cuda())
    got = ops.lexicon_shortlist(*dev, handle, K)                   # warm-up
    n = min(B, host_samples)
    t0 = time.perf_counter()
    ref = decoding.lexicon_shortlist_host(hyp[:n], hyp_len[:n], tokens, lengths, K)
    host_ms = 1e3 * (time.perf_counter() - t0) * B / n
    same = bool(np.array_equal(got[0][:n].cpu().numpy(), ref[0]) and np.array_equal(got[1][:n].cpu().numpy(), ref[1]))
    times = [device_ms(lambda: ops.lexicon_shortlist(*dev, handle, K), reps) for _ in range(rounds)]
    return {"kernel_ms": [round(t, 4) for t in times], "host_form_ms_scaled_from_%d_samples" % n: round(host_ms, 1), "equal_on_those": same}


def nets(B):
    """(TRBA x 6, its converter, CRNN x 3, its converter, images): imgW = 256, random weights"""
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as Wt
    from mrn_amd.tools.utils import AttnLabelConverter, CTCLabelConverter

    def opt(seq, pred, trans, fe):
        return types.SimpleNamespace(Transformation=trans, FeatureExtraction=fe, SequenceModeling=seq, Prediction=pred, num_fiducial=20,
                                     imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256, batch_max_length=25)
    out = []
    for experts, o, conv in ((6, opt("BiLSTM", "Attn", "TPS", "ResNet"), AttnLabelConverter(CHARS)),
                             (3, opt("BiLSTM", "CTC", "None", "VGG"), CTCLabelConverter(CHARS))):
        classes = len(conv.character)
        with contextlib.redirect_stdout(io.StringIO()):
            net = MRNNet(o)
            for _ in range(experts):
                net.update_fc(256, classes)
                net.build_prediction(net.opt, classes)
        Wt.fill_state_dict(net.state_dict(), seed=11)
        out += [net.cuda().eval(), conv, o]
    image = torch.from_numpy(Wt.smooth_image("bench_shortlist", (B, 4, 32, 256), 11))
    return out, image


def validation_times(B, K, sizes, rounds, exhaustive_max):
    """per batch: infer_time + the scoring section of validation(), ms"""
    import mrn_amd.test as V
    (trba, attn_conv, attn_opt, crnn, ctc_conv, ctc_opt), image = nets(B)
    labels = [f"label{b}" for b in range(B)]
    batch = [(image, labels)]

    def run(net, conv, base, **kw):
        o = types.SimpleNamespace(**{**vars(base), **kw})
        times = []
        with torch.no_grad():
            for r in range(rounds + 1):                            # the first call warms up
                V.SCORE_TIMER = []
                res = V.validation(net, None, batch, conv, o, val_choose="TF")
                torch.cuda.synchronize()
                if r:
                    times.append(round(1e3 * (res[6] + sum(V.SCORE_TIMER)), 3))
        V.SCORE_TIMER = None
        return times

    out = {"trba6": {"greedy": run(trba, attn_conv, attn_opt)}, "crnn3": {"greedy": run(crnn, ctc_conv, ctc_opt)}}
    for N in sizes:
        words = random_strings(N, seed=N)
        out["trba6"][f"shortlist_K{K}_N{N}"] = run(trba, attn_conv, attn_opt, attn_lexicon=words, lexicon_shortlist=K)
        out["crnn3"][f"shortlist_K{K}_N{N}"] = run(crnn, ctc_conv, ctc_opt, lexicon=words, lexicon_shortlist=K)
        if N <= exhaustive_max:
            out["trba6"][f"trie_beam_W{WIDTH}_N{N}"] = run(trba, attn_conv, attn_opt, attn_lexicon=words, beam_width=WIDTH)
            out["crnn3"][f"every_word_N{N}"] = run(crnn, ctc_conv, ctc_opt, lexicon=words)
        if N <= 1000:
            every = {gt: words for gt in labels}
            out["trba6"][f"candidates_all_N{N}"] = run(trba, attn_conv, attn_opt, candidates=every)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--slots", type=int, default=50)
    ap.add_argument("--words", type=int, nargs="+", default=[1000, 50000, 1 << 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=4)
    ap.add_argument("--exhaustive-max", type=int, default=50000)
    ap.add_argument("--no-validation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shortlist needs a GPU: a time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B, K = args.batch, args.slots
    out = {"batch": B, "K": K, "rounds": args.rounds, "reps": args.reps, "unit": "ms per batch", "shortlist": {}}
    for N in args.words:
        out["shortlist"][f"N{N}"] = kernel_times(B, K, N, args.rounds, args.reps, args.host_samples)
    if not args.no_validation:
        out["validation"] = validation_times(B, K, args.words, args.rounds, args.exhaustive_max)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
