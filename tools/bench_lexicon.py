"""Decoding time of one evaluation batch of a CTC head against a lexicon: best path (mrn_argmax_prob_f32), the device lexicon decoder
(mrn_ctc_lexicon_decode_f32: the row pass, one scoring launch per batch, the selection) at N = 1000 and N = 50 000 words and with
K = 50 candidate words per sample, and the float64 host form of the same algorithm (modules/decoding.py::ctc_lexicon_host) at
N = 1000 on a small batch, in one process.

    python tools/bench_lexicon.py [--batch 256] [--frames 63] [--classes 2091] [--host-batch 8] [--rounds 3] [--reps 5]

The logits are 3 * randn with the blank raised by 2.5 sigma and a random class raised above it at 40 % of the frames, generated on the
device from a seed; the words are 1 .. 25 random classes (a class repeats its neighbour with probability 0.1); a sample's candidates
are 50 random words.  Per round the paths alternate: the device paths are timed by a host clock around `reps` calls that end in a
device synchronise (the lexicon is on the device already, as in validation(), which uploads it once per call), the host path around
one call that starts with the copy of the logits to the host.  The host path's time is scaled to the full batch by its sample count:
it is a loop over samples.  Also a check that the device and the host form name the same best word on the host batch.  There is no
speed target: the numbers are what DESIGN section 7 records.  Prints one JSON line; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrn_amd import ops  # noqa: E402
from mrn_amd.modules import decoding as D  # noqa: E402
from tools.bench_beam import device_ms, make_logits  # noqa: E402


def make_lexicon(N, C, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 26, size=N).astype(np.int32)
    tokens = rng.integers(1, C, size=(N, 25)).astype(np.int32)
    again = rng.random((N, 25)) < 0.1
    for u in range(1, 25):
        tokens[:, u] = np.where(again[:, u], tokens[:, u - 1], tokens[:, u])
    tokens[np.arange(25)[None, :] >= lens[:, None]] = 0
    return tokens, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=63)
    ap.add_argument("--classes", type=int, default=2091)
    ap.add_argument("--host-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lexicon needs a GPU: a decoding time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B, T, C, Bh = args.batch, args.frames, args.classes, min(args.host_batch, args.batch)
    x = make_logits(B, T, C, seed=T)
    lex = {}
    for N in (1000, 50000):
        tokens, lens = make_lexicon(N, C, seed=N)
        assert D.lexicon_supported("CTC", T, C, tokens.shape[1], N, 1)
        lex[N] = (tokens, lens, torch.from_numpy(tokens).cuda(), torch.from_numpy(lens).cuda())
    cand = torch.from_numpy(np.random.default_rng(50).integers(0, 50000, size=(B, 50)).astype(np.int32)).cuda()
    paths = {
        "greedy_ms": lambda: ops.argmax_prob_lastdim(x),
        "lexicon_1000_ms": lambda: ops.ctc_lexicon_decode(x, lex[1000][2], lex[1000][3], 1),
        "lexicon_50000_ms": lambda: ops.ctc_lexicon_decode(x, lex[50000][2], lex[50000][3], 1),
        "candidates_50_of_50000_ms": lambda: ops.ctc_lexicon_decode(x, lex[50000][2], lex[50000][3], 1, cand),
    }
    for fn in paths.values():                                        # warm-up: code objects, allocator
        fn()
    times = {k: [] for k in paths}
    host, same = [], None
    for _ in range(args.rounds):
        for k, fn in paths.items():
            times[k].append(device_ms(fn, args.reps))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = D.ctc_lexicon_host(x[:Bh].cpu().numpy(), lex[1000][0], lex[1000][1], 1)
        host.append(1e3 * (time.perf_counter() - t0))
        if same is None:
            index = ops.ctc_lexicon_decode(x[:Bh], lex[1000][2], lex[1000][3], 1)[0].cpu().numpy()
            same = int((index[:, 0] == ref[0][:, 0]).sum())
    out = {"batch": B, "frames": T, "classes": C, "rounds": args.rounds, "reps": args.reps, "unit": "ms per batch",
           **{k: [round(v, 4) for v in vs] for k, vs in times.items()},
           "host_1000_ms_on_host_batch": [round(v, 1) for v in host], "host_batch": Bh,
           "host_1000_ms_scaled_to_batch": [round(v * B / Bh, 1) for v in host], "same_best_word": f"{same}/{Bh}",
           "pairs_per_second_50000": round(B * 50000 / (min(times["lexicon_50000_ms"]) * 1e-3))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
