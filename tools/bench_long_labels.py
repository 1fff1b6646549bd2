"""Long labels: the CTC loss per launch at L = 25 on the 64-state kernel, L = 25 and L = 63 on the long kernel, and loop B of
CRNN x 3, SVTR x 6 and TRBA x 6 at batch_max_length 25 and 63 (built as bench.py builds them; TRBA decodes 64 steps at 63).

    python tools/bench_long_labels.py [--steps 10] [--warmup 3] [--batch 256] [--lengths 25 63] [--skip-loop-b]

The CTC section times fwd + bwd (ops.ctc_loss_fwd / ctc_loss_bwd, or the entry points directly for the long kernel at 25) with HIP
events at B = 256 on [B, T, C] logits, T = 63 (VGG) and 64 (SVTR), C = the bench's summed class counts of CRNN x 3 and SVTR x 6;
labels are drawn at lengths 1..L.  Prints one JSON line.
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
from mrn_amd._lib import call  # noqa: E402

CTC_CLASSES = {"crnn_x3": sum(bench.CLASSES_MLT19[:3]) + 4, "svtr_x6": sum(bench.CLASSES_MLT19) + 4}


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


def ctc_case(B, T, C, L, kernel):
    """fwd + bwd ms of one CTC loss; kernel "short" / "long": the 64-state kernel or the long one (at L <= 31 called directly)"""
    g = torch.Generator(device="cuda").manual_seed(L * 7 + T)
    logits = ops.padded_rows(B, T, C, "cuda")
    logits.copy_(torch.randn(B, T, C, device="cuda", generator=g) * 3)
    targets = torch.randint(2, C, (B, L), device="cuda", generator=g)
    tl = torch.randint(1, L + 1, (B,), device="cuda", generator=g).to(torch.int32)
    up = torch.ones(1, device="cuda")
    if kernel == "short" or L > 31:
        def run():
            _, ctx = ops.ctc_loss_fwd(logits, targets, tl)
            ops.ctc_loss_bwd(ctx, up)
    else:
        lse, nll = torch.empty(B * T, device="cuda"), torch.empty(B, device="cuda")
        occ = torch.empty(call("mrn_ctc_occ_floats_long", B, T, L), device="cuda")
        loss, d = torch.empty(1, device="cuda"), torch.empty_like(logits)
        st = torch.cuda.current_stream().cuda_stream

        def run():
            call("mrn_ctc_loss_fwd_long_f32", logits.data_ptr(), logits.stride(1), targets.data_ptr(), L, tl.data_ptr(), L,
                 lse.data_ptr(), nll.data_ptr(), occ.data_ptr(), loss.data_ptr(), B, T, C, 0, st)
            call("mrn_ctc_loss_bwd_long_f32", logits.data_ptr(), logits.stride(1), lse.data_ptr(), occ.data_ptr(), targets.data_ptr(),
                 L, tl.data_ptr(), L, nll.data_ptr(), up.data_ptr(), d.data_ptr(), d.stride(1), B, T, C, 0, st)
    ms = time_ms(run)
    torch.cuda.empty_cache()
    return round(ms, 4)


def loop_b(model, experts, bml, batch, steps, warmup):
    from mrn_amd.data.synthetic import SyntheticTextLines
    from mrn_amd.tools.utils import to_device
    opt = bench.make_opt(model, batch)
    opt.batch_max_length = bml
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
    ap.add_argument("--lengths", type=int, nargs="+", default=[25, 63])
    ap.add_argument("--skip-loop-b", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"batch": args.batch, "ctc_fwd_bwd_ms": {}, "loop_b": {}}
    for name, C in CTC_CLASSES.items():
        for T in (63, 64):
            key = f"{name}_C{C}_T{T}"
            res["ctc_fwd_bwd_ms"][key] = {"L25_short": ctc_case(args.batch, T, C, 25, "short"),
                                          "L25_long": ctc_case(args.batch, T, C, 25, "long"),
                                          "L63_long": ctc_case(args.batch, T, C, 63, "long")}
    if not args.skip_loop_b:
        for model, experts in (("crnn", 3), ("svtr", 6), ("trba", 6)):
            for bml in args.lengths:
                res["loop_b"][f"{model}x{experts}@{bml}"] = loop_b(model, experts, bml, args.batch, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
