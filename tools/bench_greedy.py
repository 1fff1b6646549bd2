"""Greedy decoding on the attention head: the fused launch (mrn_attn_greedy_decode*, all steps of all experts in one launch) against the
step loop it replaces (five launches per step and expert: MRN_GREEDY_DECODE=stepwise), alternately in one process.

    python tools/bench_greedy.py [--rounds 3] [--vb-sweep] [--no-validation]

B = 256, T = 65, D = 256, S = 26, the bench's TRBA class counts (2091 ... 5374).  Cases: one expert (the smallest and the largest class
count) through Attention.forward; six experts, one grouped launch behind six i2h Linears against six per-expert step loops; and one
whole validation() batch of TRBA x 6 (cross=True, is_train=False: backbones, BiLSTMs, decoders, routing, scoring).  Every figure is the
mean of a few calls between two device events (validation(): host clock around the synchronising call); `rounds` figures per path, and
the verdict asks for the fused path to beat the step loop by more than the step loop's own spread.  --vb-sweep times the fused launch
at MRN_GREEDY_VB = 2, 4, 8, 16 samples per workgroup.  Prints one JSON line; needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import types

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrn_amd import ops  # noqa: E402

CLASSES = (2091, 2311, 4039, 5199, 5272, 5374)       # bench.py: running sums of the MLT19 task sizes + the attention head's 5 tokens
B, T, D, S, HID = 256, 65, 256, 26, 256


def event_ms(fn, reps):
    fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def set_mode(mode):
    if mode == "fused":
        os.environ.pop("MRN_GREEDY_DECODE", None)
    else:
        os.environ["MRN_GREEDY_DECODE"] = mode


def heads(classes):
    from mrn_amd.modules.prediction import Attention
    out = []
    for g, C in enumerate(classes):
        torch.manual_seed(100 + g)
        att = Attention(D, HID, C, nn.Linear(HID, C))
        with torch.no_grad():
            for p in att.parameters():
                p.uniform_(-0.08, 0.08)
            att.char_embeddings.weight.uniform_(-1, 1)
        out.append(att.cuda())
    return out


def grouped_fn(atts, Hb, sos):
    outs = [ops.padded_rows(B, S, a.num_class, Hb.device) for a in atts]

    def fn():
        Hproj = torch.stack([ops.linear(Hb[g], a.attention_cell.i2h.weight) for g, a in enumerate(atts)])
        cols = list(zip(*[a.greedy_args() for a in atts]))
        ops.attn_greedy_decode_grouped(Hb, Hproj, cols[0], sos, *cols[1:9], HID, S, outs, w_inv=cols[9] if cols[9][0] is not None else None)
        return outs
    return fn


def stepwise_fn(atts, Hb, sos):
    def fn():
        return [a(Hb[g], sos, False, S - 1) for g, a in enumerate(atts)]
    return fn


def alternate(fused, stepwise, rounds, reps_fused=5, reps_step=2):
    f_ms, s_ms = [], []
    for _ in range(rounds):
        set_mode("fused")
        f_ms.append(event_ms(fused, reps_fused))
        set_mode("stepwise")
        s_ms.append(event_ms(stepwise, reps_step))
    set_mode("fused")
    spread = max(s_ms) - min(s_ms)
    return {"fused_ms": [round(v, 3) for v in f_ms], "stepwise_ms": [round(v, 3) for v in s_ms], "stepwise_spread_ms": round(spread, 3),
            "fused_faster_by_more_than_the_spread": min(s_ms) - max(f_ms) > spread}


def same_tokens(fused, stepwise):
    set_mode("fused")
    a = [o.argmax(2) for o in fused()]
    set_mode("stepwise")
    b = [o.argmax(2) for o in stepwise()]
    set_mode("fused")
    return all(torch.equal(x, y) for x, y in zip(a, b))


def validation_case(rounds):
    from mrn_amd import test as V
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as W
    from mrn_amd.tools.utils import AttnLabelConverter
    opt = types.SimpleNamespace(Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM", Prediction="Attn",
                                num_fiducial=20, imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256,
                                batch_max_length=25, NED=True)
    with contextlib.redirect_stdout(io.StringIO()):
        extra = len(AttnLabelConverter("a").character) - 1
        chars = "".join(chr(0x4E00 + i) for i in range(CLASSES[-1] - extra))
        conv = AttnLabelConverter(chars)
        net = MRNNet(opt)
        for c in CLASSES:
            net.update_fc(256, c)
            net.build_prediction(opt, c)
    assert len(conv.character) == CLASSES[-1]
    W.fill_state_dict(net.state_dict(), seed=7)
    net = net.cuda().eval()
    image = torch.from_numpy(W.smooth_image("bench_greedy", (B, 4, 32, 256), 7))
    labels = ["".join(chars[(7 * b + i) % len(chars)] for i in range(5 + b % 20)) for b in range(B)]
    loader = [(image, labels)]

    def run():
        with torch.no_grad():
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = V.validation(net, None, loader, conv, opt, "TF")
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t), res

    set_mode("fused")
    run()
    set_mode("stepwise")
    run()
    f_ms, s_ms, same = [], [], True
    for _ in range(rounds):
        set_mode("fused")
        t, rf = run()
        f_ms.append(t)
        set_mode("stepwise")
        t, rs = run()
        s_ms.append(t)
        same = same and rf[1] == rs[1] and rf[2] == rs[2]          # accuracy and normalised edit distance of the batch
    set_mode("fused")
    spread = max(s_ms) - min(s_ms)
    return {"fused_ms": [round(v, 2) for v in f_ms], "stepwise_ms": [round(v, 2) for v in s_ms], "stepwise_spread_ms": round(spread, 2),
            "same_scores": same, "fused_faster_by_more_than_the_spread": min(s_ms) - max(f_ms) > spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vb-sweep", action="store_true")
    ap.add_argument("--no-validation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_greedy needs a GPU: a decoding time from a CPU-only run would say nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    sos = torch.full((B,), 2, dtype=torch.long, device=dev)
    Hb6 = torch.rand(6, B, T, D, device=dev) * 2 - 1
    out = {"B": B, "T": T, "D": D, "S": S, "classes": list(CLASSES), "rounds": args.rounds, "unit": "ms", "cases": {}}
    with torch.no_grad():
        atts = heads(CLASSES)
        cases = {"G1_C2091": (atts[:1], Hb6[:1]), "G1_C5374": (atts[5:], Hb6[5:]), "G6": (atts, Hb6)}
        for name, (hs, Hb) in cases.items():
            fused = stepwise_fn(hs, Hb, sos) if len(hs) == 1 else grouped_fn(hs, Hb, sos)       # one expert: Attention.forward both ways
            stepwise = stepwise_fn(hs, Hb, sos)
            r = alternate(fused, stepwise, args.rounds)
            r["same_tokens"] = same_tokens(fused, stepwise)
            out["cases"][name] = r
        if args.vb_sweep:
            sweep = {}
            for name in ("G1_C2091", "G1_C5374", "G6"):
                hs, Hb = cases[name]
                fn = grouped_fn(hs, Hb, sos) if len(hs) > 1 else stepwise_fn(hs, Hb, sos)
                row = {}
                for vb in (2, 4, 8, 16):
                    os.environ["MRN_GREEDY_VB"] = str(vb)
                    row[str(vb)] = round(min(event_ms(fn, 5) for _ in range(2)), 3)
                os.environ.pop("MRN_GREEDY_VB", None)
                row["rule"] = round(min(event_ms(fn, 5) for _ in range(2)), 3)
                sweep[name] = row
            out["vb_sweep_fused_ms"] = sweep
    if not args.no_validation:
        out["validation_batch_trba6"] = validation_case(args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
