"""Task counts: loop B of TRBA and CRNN at I = 6 / 8 / 12 / 16 experts and the DER step of TRBA at G = 7 / 8 / 12 extractors, with the
peak device memory of each point, and the attention decoder per launch at D = 1792 (G = 7) in its single-launch form and in the
wide-context (chunked) form.

    python tools/bench_many_tasks.py [--steps 10] [--warmup 3] [--batch 256] [--skip-loop-b] [--skip-der]

Learners are built as bench.py builds them.  The per-task class counts are the MLT19 ones (bench.CLASSES_MLT19) for the first six
tasks; tasks 7 and later are SYNTHETIC, 150 classes each (no dataset splits MLT19 that far).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SYNTHETIC_CLASSES = 150       # per task beyond the sixth
MLT19 = tuple(bench.CLASSES_MLT19)


def use_tasks(n):
    """bench's per-task class table extended to n tasks (the extension is synthetic)"""
    bench.CLASSES_MLT19 = MLT19 + (SYNTHETIC_CLASSES,) * max(0, n - len(MLT19))


def loop_b(model, experts, batch, steps, warmup):
    from mrn_amd.data.synthetic import SyntheticTextLines
    from mrn_amd.tools.utils import to_device
    use_tasks(experts)
    opt = bench.make_opt(model, batch)
    opt.lan_list = [f"L{i}" for i in range(experts)]
    torch.cuda.reset_peak_memory_stats()
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
    peak = torch.cuda.max_memory_allocated()
    pending.clear()
    del learner
    torch.cuda.empty_cache()
    return {"images_per_s": round(batch * steps / elapsed, 1), "ms_per_step": round(elapsed / steps * 1e3, 3),
            "peak_mem_gib": round(peak / 2 ** 30, 2)}


def der_step(extractors, batch, steps, warmup):
    use_tasks(extractors)
    opt = bench.make_opt("trba", batch)
    opt.lan_list = [f"L{i}" for i in range(extractors)]
    args = types.SimpleNamespace(experts=extractors, batch=batch, verbose=False, serial=False, model="trba")
    torch.cuda.reset_peak_memory_stats()
    res = bench.time_der_step(args, opt, 0, 1, steps, warmup)
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    return {"images_per_s": round(res["value"], 1), "ms_per_step": round(res["ms_per_step"], 3), "peak_mem_gib": round(peak / 2 ** 30, 2),
            "decoder_form": "wide (1024-column chunks)" if extractors >= 8 else "single launch"}


def decoder_launch_ms(D, chunked, B=256, T=65, reps=10):
    """one teacher-forced decoder launch (26 steps, x3 products) at B = 256"""
    from mrn_amd import ops
    g = torch.Generator(device="cuda").manual_seed(D)
    H = torch.randn(B, T, D, device="cuda", generator=g)
    Hp = torch.randn(B, T, 256, device="cuda", generator=g)
    ep = torch.randn(B, 26, 1024, device="cuda", generator=g)
    w_h2h, w_ih, w_hh = (torch.randn(s, device="cuda", generator=g) * 0.05 for s in ((256, 256), (1024, D + 256), (1024, 256)))
    a, b, c, w_inv = ops.pack_decoder_x3(w_h2h, w_ih, w_hh, D)
    bias = torch.zeros(1024, device="cuda")

    def run():
        ops.attn_decoder(H, Hp, ep, a, bias[:256], torch.randn(1, 256, device="cuda"), b, c, bias, 256, w_inv=w_inv)
    if chunked:
        os.environ["MRN_ATTN_CTX_CHUNK"] = "1"
    try:
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("MRN_ATTN_CTX_CHUNK", None)
    return round(e0.elapsed_time(e1) / reps, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--skip-loop-b", action="store_true")
    ap.add_argument("--skip-der", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"batch": args.batch, "synthetic_classes_per_task_beyond_6": SYNTHETIC_CLASSES, "loop_b": {}, "der_step": {},
           "decoder_ms_per_launch_D1792": {"single_launch": decoder_launch_ms(1792, False), "wide": decoder_launch_ms(1792, True)}}
    if not args.skip_loop_b:
        for model in ("trba", "crnn"):
            for n in (6, 8, 12, 16):
                res["loop_b"][f"{model}x{n}"] = loop_b(model, n, args.batch, args.steps, args.warmup)
                print(json.dumps({f"{model}x{n}": res["loop_b"][f"{model}x{n}"]}), file=sys.stderr, flush=True)
    if not args.skip_der:
        for n in (7, 8, 12):
            res["der_step"][f"trba_der{n}"] = der_step(n, args.batch, args.steps, args.warmup)
            print(json.dumps({f"der{n}": res["der_step"][f"trba_der{n}"]}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
