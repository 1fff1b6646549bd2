"""Hidden sizes: the LSTM layer per step at hidden 128 / 256 / 512 -- the frozen experts' forward (split-fp16 x3, G = 1 and 3 experts x 2
directions in one launch) and one trained layer's forward with saves and backward through time -- and loop B of CRNN x 3 and SVTR x 6
at the three sizes (built as bench.py builds them, with opt.hidden_size set).

    python tools/bench_hidden.py [--steps 10] [--warmup 3] [--batch 256] [--hidden 128 256 512] [--skip-loop-b]

The layer section times launches with HIP events at B = --batch, T = 65.  The XCD pinning rules of the layer kernels are the ones tuned
at 256 (1 MiB of W_hh per expert and direction); at 512 a set is 4 MiB -- one XCD's whole L2 -- and the rules run as they are: this
tool measures that, nothing here tunes it.  Prints one JSON line.
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

T = 65


def time_us(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def layer_case(Hd, G, B):
    """us / step of the grouped x3 forward of G experts, and (G = 1) of the training forward with saves and the backward"""
    dev = torch.device("cuda:0")
    torch.manual_seed(Hd + G)
    xproj = torch.randn(G, B, T, 8 * Hd, device=dev) * 0.7
    ws = [[torch.randn(4 * Hd, Hd, device=dev) / (Hd ** 0.5) for _ in range(2)] for _ in range(G)]
    packs = [[ops.pack_fragment_major_h(w, Hd) for w in p] for p in ws]
    w_h = torch.stack([torch.stack([d[0] for d in p]) for p in packs]).contiguous()
    w_inv = torch.stack([torch.cat([d[1] for d in p]) for p in packs]).contiguous()
    b_hh = torch.randn(G, 8 * Hd, device=dev) / 16.0
    res = {"fwd_x3_us_per_step": round(time_us(lambda: ops.lstm_layer_x3_grouped(xproj, w_h, w_inv, b_hh, Hd, 2)) / T, 2)}
    if G == 1:
        out, gates, cseq = ops.lstm_layer_x3_save(xproj[0], w_h[0], w_inv[0], b_hh[0], Hd, 2)
        packsT = [ops.pack_fragment_major_h(w.t().contiguous(), Hd) for w in ws[0]]
        wT_h, wT_inv = torch.stack([p[0] for p in packsT]).contiguous(), torch.cat([p[1] for p in packsT]).contiguous()
        dout = torch.randn(B, T, 2 * Hd, device=dev) * 1e-3
        res["train_fwd_us_per_step"] = round(time_us(lambda: ops.lstm_layer_x3_save(xproj[0], w_h[0], w_inv[0], b_hh[0], Hd, 2)) / T, 2)
        res["train_bwd_us_per_step"] = round(time_us(lambda: ops.lstm_layer_bwd_x3(dout, gates, cseq, wT_h, wT_inv, Hd, 2)) / T, 2)
    torch.cuda.empty_cache()
    return res


def loop_b(model, experts, hidden, batch, steps, warmup):
    from mrn_amd.data.synthetic import SyntheticTextLines
    from mrn_amd.tools.utils import to_device
    opt = bench.make_opt(model, batch)
    opt.hidden_size = hidden
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
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--skip-loop-b", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"batch": args.batch, "T": T, "lstm_layer": {}, "loop_b": {}}
    for Hd in args.hidden:
        for G in (1, 3):
            res["lstm_layer"][f"H{Hd}_G{G}"] = layer_case(Hd, G, args.batch)
    if not args.skip_loop_b:
        for model, experts in (("crnn", 3), ("svtr", 6)):
            for Hd in args.hidden:
                res["loop_b"][f"{model}x{experts}@H{Hd}"] = loop_b(model, experts, Hd, args.batch, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
