"""Loop B at imgW = 128 / 256 / 512 (imgH = 32): the TRBA x 6 and CRNN x 3 MRN router steps bench.py times at 32 x 256, built the same
way (bench.build_learner) with another opt.imgW -- tools/bench_geometry.py's loop along the other axis.

    python tools/bench_width.py [--steps 10] [--warmup 3] [--batch 256] [--widths 128 256 512] [--height 32]

The step loop is bench.py's (pipelined: the next batch's experts are prefetched).  Per row: images/s, ms/step, and images/s x imgW /
256 -- the rate in 256-pixel-line equivalents, so that rows of different widths can be compared per pixel.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from mrn_amd.modules.geometry import call_in_budget, frames  # noqa: E402


def loop_b(model, experts, imgH, imgW, batch, steps, warmup):
    from mrn_amd.data.synthetic import SyntheticTextLines
    from mrn_amd.tools.utils import to_device
    opt = bench.make_opt(model, batch)
    opt.imgH, opt.imgW = imgH, imgW
    learner = bench.build_learner(opt, experts)
    data = SyntheticTextLines(opt, seed=111)
    data.set_characters(learner.character)

    def fetch():
        image, labels, idx = data.get_batch2()
        indexs = to_device(torch.LongTensor(idx).squeeze())
        pre = learner.prefetch_experts(image, labels)
        return image, labels, indexs, pre if (pre is not None and pre[0] is not None) else None
    pending = [fetch()]

    def step():
        image, labels, indexs, pre = pending.pop()
        pending.append(fetch())
        return learner.routing_step(image, labels, indexs, prefetched=pre)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    pending.clear()
    del learner
    torch.cuda.empty_cache()
    return {"images_per_s": round(batch * steps / elapsed, 1), "ms_per_step": round(elapsed / steps * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=32)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 256, 512])
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"batch": args.batch, "imgH": args.height, "loop_b": {}}
    for model, experts, feat in (("trba", 6, "ResNet"), ("crnn", 3, "VGG")):
        for w in args.widths:
            if not call_in_budget(args.batch, args.height, w):
                continue
            row = loop_b(model, experts, args.height, w, args.batch, args.steps, args.warmup)
            row["frames"] = frames(feat, w)
            row["images_per_s_x_w_over_256"] = round(row["images_per_s"] * w / 256.0, 1)
            res["loop_b"][f"{model}x{experts}@{args.height}x{w}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
