"""Time of the herding selection (mrn_herding_select_f32: m picks out of an N x D feature table that stays on the device) against the
float64 numpy host form herding.herding_host, and of the feature pass (mrn_herding_features_f32) over one batch:

    python tools/bench_herding.py [--shapes 10000,256,1000 50000,256,2000 50000,2048,2000] [--rounds 3] [--reps 2] [--host-steps 50]
                                  [--batch 256,65,256]

Per shape (N, D, m): ops.herding_select on the device, a host clock around `reps` calls that end in a device synchronise, `rounds`
times; the host form timed at 1 + host-steps and at 1 + 2 host-steps steps and scaled to m (it is linear in the steps: one N x D
matrix-vector product each); whether the device's first picks equal the host's on those steps (unit rows, so differences in the last fp32 bits can
reorder near-ties: reported, not asserted); the bytes a step reads over the time of a step.  The feature pass: a [B, T, D] batch.
Prints one JSON line; needs a GPU.
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
from mrn_amd.modules import herding  # noqa: E402


def device_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def unit_rows(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, generator=g) / D ** 0.5 + torch.randn(1, D, generator=g) / D ** 0.5
    return x / x.norm(dim=1, keepdim=True)


def select_times(N, D, m, rounds, reps, host_steps):
    F = unit_rows(N, D, N + D)
    dev = F.cuda()
    got = ops.herding_select(dev, m)[0].cpu().numpy()              # warm-up
    table = F.numpy()
    herding.herding_host(table, 1)                                 # (first touch of the float64 copy's pages)
    t0 = time.perf_counter()
    ref = herding.herding_host(table, 1 + host_steps)[0]
    t1 = time.perf_counter()
    herding.herding_host(table, 1 + 2 * host_steps)
    t2 = time.perf_counter()
    per_step = max((t2 - t1) - (t1 - t0), 0.0) / host_steps        # the two calls differ by host_steps steps
    setup = max((t1 - t0) - per_step * (1 + host_steps), 0.0)
    times = [device_ms(lambda: ops.herding_select(dev, m), reps) for _ in range(rounds)]
    best = min(times)
    return {"N": N, "D": D, "m": m, "device_ms": [round(t, 3) for t in times], "device_us_per_step": round(1e3 * best / m, 3),
            "table_GB_per_s": round(N * D * 4 / (best / m * 1e-3) / 1e9, 1), "host_form_ms_scaled_from_%d_steps" % host_steps:
            round(1e3 * (setup + per_step * m), 1), "host_ms_per_step": round(1e3 * per_step, 3),
            "first_picks_equal_the_host_form": bool(np.array_equal(got[:1 + host_steps], ref))}


def feature_times(B, T, D, rounds, reps):
    feat = torch.randn(B, T, D, generator=torch.Generator().manual_seed(1)).cuda()
    table = torch.zeros(B, D, device="cuda")
    ops.herding_features(feat, out=table)
    times = [device_ms(lambda: ops.herding_features(feat, out=table), reps) for _ in range(rounds)]
    t0 = time.perf_counter()
    herding.features_host(feat.cpu().numpy())
    return {"B": B, "T": T, "D": D, "device_ms": [round(t, 4) for t in times], "host_form_ms": round(1e3 * (time.perf_counter() - t0), 2)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["10000,256,1000", "50000,256,2000", "50000,2048,2000"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=50)
    ap.add_argument("--batch", default="256,65,256")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_herding.py needs a GPU")
    out = {"select": [select_times(*(int(v) for v in s.split(",")), args.rounds, args.reps, args.host_steps) for s in args.shapes],
           "features": feature_times(*(int(v) for v in args.batch.split(",")), args.rounds, max(args.reps, 20))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
