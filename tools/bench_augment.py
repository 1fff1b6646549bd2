"""Training-time text augmentation (Aug = Blur / Crop / Rot tokens): device time of the kernel chain per 256-crop batch, host (PIL)
images/s per core, and Dataset_Manager images/s with the augmentation on the host vs on the device vs Aug="None".

    python tools/bench_augment.py [--aug Blur5-Crop90-Rot15] [--batches 20] [--workers 4 8]

Crops are realistic text-line sizes (40-200 x 24-48 RGBA).  Device time comes from HIP events around the stage chain after warm-up;
bytes moved are computed from the shapes (every stage's reads and writes of its windows, the fp32 output).  Prints one JSON line.
"""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import time
import types

import numpy as np
import PIL.Image
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrn_amd.data import augment as A  # noqa: E402


def crops(n, seed):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        w, h = int(g.integers(40, 201)), int(g.integers(24, 49))
        a = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
        a[..., 3] = 255
        out.append(PIL.Image.fromarray(a, "RGBA"))
    return out


def chain_bytes(rb):
    """bytes the chain reads and writes, from the planned windows (4 bytes per pixel, 16 per output pixel of the fp32 result)"""
    total = 0
    for si, kind in enumerate(rb.kinds):
        for d in rb.desc[si]:
            if kind == "blur" and d[5] >= 0:
                total += 4 * int(d[2]) * int(d[3]) * 4            # x pass: read + write; y pass in place: read + write
            elif kind == "rot" and d[7] != 0:
                total += 4 * (int(d[2]) * int(d[3]) + int(d[5]) * int(d[6]))
    W, H = rb.size
    for d in rb.desc[-1]:
        total += 4 * int(d[2]) * int(d[3]) + 16 * W * H
        if d[5] in (A.RS_HV, A.RS_VH):
            tmp = W * int(d[3]) if d[5] == A.RS_HV else int(d[2]) * H
            total += 8 * tmp
    return total


def device_chain(aug, batches):
    from mrn_amd import ops
    stages = A.parse_aug(aug)
    plans = []
    for i in range(batches):
        torch.manual_seed(i)
        random.seed(i)
        plans.append(A.plan_batch(crops(256, i), stages, (256, 32))[0])
    out = torch.empty((256, 4, 32, 256), device="cuda")
    dev = []
    for rb in plans:
        px = torch.zeros(rb.total * 4, dtype=torch.uint8, device="cuda")
        px[:rb.pool.size] = torch.from_numpy(rb.pool).cuda()
        dev.append((rb, px, torch.from_numpy(rb.desc).cuda(), torch.from_numpy(rb.matrix).cuda()))
    for rb, px, d, m in dev[:3]:                                    # warm-up
        ops.augment_batch(px, rb, d, m, out)
    torch.cuda.synchronize()
    times = []
    for rb, px, d, m in dev:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.augment_batch(px, rb, d, m, out)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    mb = [chain_bytes(rb) / 1e6 for rb, *_ in dev]
    return {"device_ms_per_batch_median": float(np.median(times)), "device_ms_per_batch_min": float(np.min(times)),
            "launches_per_batch": 2 * sum(1 for k in plans[0].kinds if k == "blur") + sum(1 for k in plans[0].kinds if k == "rot") + 2,
            "mb_moved_per_batch": float(np.mean(mb)),
            "pool_mb_per_batch": float(np.mean([rb.pool.nbytes / 1e6 for rb in plans]))}


def host_rate(aug, n=512):
    torch.set_num_threads(1)
    ims = crops(n, 99)
    t = A.TextAugment(types.SimpleNamespace(Aug=aug, imgW=256, imgH=32))
    t0 = time.perf_counter()
    for im in ims:
        t(im)
    return n / (time.perf_counter() - t0)


def manager_rate(aug, workers, device_aug, batches):
    """images/s of get_batch with staging to the GPU; device_aug False: the augmentation stays in the workers (host path)"""
    from mrn_amd.data.data_manage import Dataset_Manager
    from mrn_amd.data.dataset import ArrayDataset
    opt = types.SimpleNamespace(imgH=32, imgW=256, batch_max_length=25, memory_num=40, batch_size=256, workers=workers, Aug=aug,
                                il="mrn", memory=None, lan_list=["Latin"], select_data=["bench"], device_prefetch=True)
    ims = [np.asarray(im) for im in crops(2048, 7)]

    def open_ds(path, o, mode="train"):
        return ArrayDataset(ims, ["abc"] * len(ims), o, mode)

    with contextlib.redirect_stdout(io.StringIO()):
        dm = Dataset_Manager(opt, open_dataset=open_ds, device=torch.device("cuda"))
        if not device_aug:
            dm._device_augment = lambda: False
        dm.select_data = opt.select_data
        dm.get_dataset(0, memory=None)
    for _ in range(3):
        dm.get_batch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        x, _ = dm.get_batch()
        x.sum()                           # consume on the compute stream
    torch.cuda.synchronize()
    return 256 * batches / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aug", default="Blur5-Crop90-Rot15")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--workers", type=int, nargs="+", default=[4, 8])
    args = ap.parse_args()
    res = {"aug": args.aug, "batch": 256}
    res.update(device_chain(args.aug, args.batches))
    res["host_images_per_s_per_core"] = host_rate(args.aug)
    torch.set_num_threads(4)
    for w in args.workers:
        res[f"manager_w{w}_host_aug"] = manager_rate(args.aug, w, False, args.batches)
        res[f"manager_w{w}_device_aug"] = manager_rate(args.aug, w, True, args.batches)
        res[f"manager_w{w}_none"] = manager_rate("None", w, True, args.batches)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
