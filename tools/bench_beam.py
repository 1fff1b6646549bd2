"""Decoding time of one evaluation batch of a CTC head: best path (mrn_argmax_prob_f32), the device beam decoder
(mrn_ctc_beam_decode_f32, one launch per batch) and the float64 host form of the same algorithm (modules/decoding.py::ctc_beam_host),
in one process.

    python tools/bench_beam.py [--batch 256] [--rounds 3] [--reps 10] [--top-n 15]

Two shapes at the class counts the project reaches after several languages: T = 63 with C = 2091, T = 127 with C = 5374; beam widths
4, 8 and 16.  The logits are 3 * randn with the blank raised by 2.5 sigma and a random class raised above it at 40 % of the frames
(labels with gaps and repeats), generated on the device from a seed.  Per round the three paths alternate: the device paths are timed
by a host clock around `reps` calls that end in a device synchronise, the host path around one call that starts with the copy of the
logits to the host (what validation() pays when it takes it).  The yardstick is the host path of the same round; the device path has
to beat it by more than the spread of the rounds.  Also a check that both beam decoders return the same best labels.  Prints one JSON
line; needs a GPU.
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


def make_logits(B, T, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = 3.0 * torch.randn(B, T, C, device="cuda", generator=g)
    x[:, :, 0] += 7.5
    frames = torch.rand(B, T, device="cuda", generator=g) < 0.4
    cls = torch.randint(1, C, (B, T), device="cuda", generator=g)
    x.scatter_add_(2, cls.unsqueeze(2), 15.0 * frames.unsqueeze(2).float())
    return x


def device_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def host_ms(x, W, K):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = D.ctc_beam_host(x.cpu().numpy(), W, K)
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--top-n", type=int, default=D.DEFAULT_BEAM_TOP_N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam needs a GPU: a decoding time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    B, K = args.batch, args.top_n
    out = {"batch": B, "rounds": args.rounds, "reps": args.reps, "top_n": K, "unit": "ms per batch", "shapes": {}}
    for T, C in ((63, 2091), (127, 5374)):
        x = make_logits(B, T, C, seed=T)
        for W in (4, 8, 16):
            assert D.beam_supported("CTC", T, C, W, K)
            for _ in range(2):                                       # warm-up: code objects, allocator
                ops.argmax_prob_lastdim(x)
                ops.ctc_beam_decode(x, W, K)
            greedy, device, host, same = [], [], [], None
            for _ in range(args.rounds):
                greedy.append(device_ms(lambda: ops.argmax_prob_lastdim(x), args.reps))
                device.append(device_ms(lambda: ops.ctc_beam_decode(x, W, K), args.reps))
                ms, ref = host_ms(x, W, K)
                host.append(ms)
                if same is None:
                    tokens, length = [o.cpu().numpy() for o in ops.ctc_beam_decode(x, W, K)[:2]]
                    same = sum(int(length[b, 0] == ref[1][b, 0] and (tokens[b, 0] == ref[0][b, 0]).all()) for b in range(B))
            spread = max(max(host) - min(host), max(device) - min(device))
            out["shapes"][f"T{T}_C{C}_W{W}"] = {
                "greedy_ms": [round(v, 4) for v in greedy], "device_beam_ms": [round(v, 4) for v in device],
                "host_beam_ms": [round(v, 1) for v in host], "spread_ms": round(spread, 3), "same_best_label": f"{same}/{B}",
                "device_faster_by_more_than_the_spread": min(host) - max(device) > spread}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
