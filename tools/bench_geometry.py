"""Loop B at imgH = 32 / 48 / 64 (imgW = 256): the TRBA x 6 and CRNN x 3 MRN router steps bench.py times at 32 x 256, built the same
way (bench.build_learner), plus the per-launch time of the height-mean pass next to the final convolution it follows.

    python tools/bench_geometry.py [--steps 10] [--warmup 3] [--batch 256] [--heights 32 48 64]

The step loop is bench.py's (pipelined: the next batch's experts are prefetched); the kernel section times the two launches of the
lock-step group's last layer on random operands with HIP events (G experts, the final map's shape).  Prints one JSON line.
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
from mrn_amd import ops  # noqa: E402


def loop_b(model, experts, imgH, batch, steps, warmup):
    from mrn_amd.data.synthetic import SyntheticTextLines
    from mrn_amd.tools.utils import to_device
    opt = bench.make_opt(model, batch)
    opt.imgH = imgH
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


def time_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def last_layer(G, B, Hf, Wf, C=512):
    """the group's final 2x2 convolution (ResNet conv4_2 / VGG conv 18: an (Hf + 1) x (Wf + 1) map in, Hf x Wf out) with its
    BatchNorm statistics, and the height mean with the BatchNorm-apply + ReLU that follows it"""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(G, B, Hf + 1, Wf + 1, C, device="cuda", generator=g)
    x_hl = ops.split_hl32(x)
    w_hl, w_scale = ops.pack_weights_hl32([torch.randn(C, 2, 2, C, device="cuda", generator=g) * 0.02 for _ in range(G)])
    y = torch.empty(G, B, Hf, Wf, C, device="cuda")
    sc, sh = torch.rand(G, C, device="cuda") + 0.5, torch.randn(G, C, device="cuda")

    def conv():
        ops.conv2d_x3(x_hl, G, False, B, Hf + 1, Wf + 1, C, w_hl, w_scale, C, (2, 2), (1, 1), (0, 0), want_stats=True, out=y,
                      products=ops.X3_PRODUCTS)

    def hmean():
        ops.height_mean_grouped(y, sc, sh, relu=True, want_f32=False, want_hl=True)
    conv_ms, mean_ms = time_ms(conv), time_ms(hmean)
    del x, x_hl, y
    torch.cuda.empty_cache()
    mbytes = 4.0 * G * B * Wf * C * (Hf + 1)          # read the map once, write the HL32 operand once
    return {"final_conv_ms": round(conv_ms, 4), "height_mean_ms": round(mean_ms, 4),
            "height_mean_GBps": round(mbytes / (mean_ms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--heights", type=int, nargs="+", default=[32, 48, 64])
    args = ap.parse_args()
    torch.cuda.set_device(0)
    final_rows = {32: 1, 48: 2, 64: 3}
    res = {"batch": args.batch, "imgW": 256, "loop_b": {}, "last_layer": {}}
    for model, experts, Wf in (("trba", 6, 65), ("crnn", 3, 63)):
        for h in args.heights:
            res["loop_b"][f"{model}x{experts}@{h}"] = loop_b(model, experts, h, args.batch, args.steps, args.warmup)
            if final_rows.get(h, 1) > 1:
                res["last_layer"][f"{model}x{experts}@{h}"] = last_layer(experts, args.batch, final_rows[h], Wf)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
