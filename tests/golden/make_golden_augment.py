"""Generate tests/golden/augment_pil.npz: Pillow's outputs for the augmentation kernels' cases (tests/test_data_augment_gpu.py), so
that the GPU tests pin the same target whatever Pillow the GPU machine carries.  PIL, numpy and torch only (the chains use the
host path's draws under fixed seeds).

    python tests/golden/make_golden_augment.py
"""
import os
import random
import sys
import types

import numpy as np
import PIL
import PIL.Image
import PIL.ImageFilter
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mrn_amd.data import augment as A  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment_pil.npz")


def crop(g, w, h, alpha="mixed"):
    """RGBA crop of 2x2-pixel random blocks: interpolation still lands between unrelated values everywhere, and the file stays small"""
    a = np.repeat(np.repeat(g.integers(0, 256, (h // 2 + 1, w // 2 + 1, 4), dtype=np.uint8), 2, 0), 2, 1)[:h, :w]
    a = np.ascontiguousarray(a)
    if alpha == "mixed":
        a[..., 3] = np.where(g.random((h, w)) < 0.4, 255, a[..., 3])
        a[: max(1, h // 4), :, 3] = 0
    elif alpha == "opaque":
        a[..., 3] = 255
    elif alpha == "zero":
        a[..., 3] = 0
    return a


def blur_cases(g):
    sizes = [(60, 20), (30, 30), (3, 30), (40, 2), (1, 1), (7, 5)]
    sigmas = [0.1, 0.7, 1.5, 3.0, 12.0]
    ims = [crop(g, w, h) for (w, h) in sizes]                      # one crop per size, every sigma
    return [(a, s) for a in ims for s in sigmas]


def rotate_cases(g):
    angles = [float(np.float32(a)) for a in (1e-3, -0.25, 15.0, -15.0, 45.0, 90.0, 180.0, -90.0, 7.3, -14.999)]
    ims = [crop(g, w, h) for (w, h) in [(48, 16), (37, 20), (5, 3), (1, 9)]]
    return [(im, a) for im in ims for a in angles]


def resize_cases(g):
    cases = []
    for w, h in [(100, 32), (2, 400)]:                           # the training size: up, tall (two steps)
        cases.append((crop(g, w, h), (256, 32)))
    for w, h in [(1, 16), (5, 16), (64, 16), (300, 20), (80, 16), (300, 12), (64, 10), (64, 48), (90, 40), (64, 1), (3, 350), (20, 250), (1, 150)]:
        cases.append((crop(g, w, h), (64, 16)))                   # each axis up / down / unchanged at a smaller output
    cases.append((crop(g, 64, 16, "opaque"), (64, 16)))            # the exact-size copy
    cases.append((crop(g, 120, 30, "zero"), (64, 16)))
    cases.append((crop(g, 4, 450), (4, 32)))                       # tall, vertical pass only
    return cases


# (Aug, seed, output W, H): one at the training size, the others smaller (the kernels take any output size)
CHAINS = [("Blur5-Crop90-Rot15", 0, 256, 32), ("Rot45-Blur2", 1, 96, 24), ("Crop50-Rot90-Crop80", 2, 96, 24),
          ("Blur0.1-Blur9-Rot180", 3, 96, 24)]


def chain_inputs(g):
    return [crop(g, int(g.integers(30, 120)), int(g.integers(16, 36))) for _ in range(2)]


def ragged(arrays):
    shapes = np.array([a.shape[:2] for a in arrays], np.int32)
    return np.concatenate([a.reshape(-1) for a in arrays]), shapes


def main():
    g = np.random.default_rng(2024)
    out = {"pillow_version": np.array(PIL.__version__)}
    bl = blur_cases(g)
    out["blur_in"], out["blur_in_shape"] = ragged([a for a, _ in bl])
    out["blur_sigma"] = np.array([s for _, s in bl], np.float64)
    out["blur_out"], _ = ragged([np.asarray(A.pil_blur(PIL.Image.fromarray(a, "RGBA"), s)) for a, s in bl])
    ro = rotate_cases(g)
    out["rot_in"], out["rot_in_shape"] = ragged([a for a, _ in ro])
    out["rot_angle"] = np.array([s for _, s in ro], np.float64)
    out["rot_out"], out["rot_out_shape"] = ragged([np.asarray(A.pil_rotate(PIL.Image.fromarray(a, "RGBA"), s)) for a, s in ro])
    rs = resize_cases(g)
    out["rs_in"], out["rs_in_shape"] = ragged([a for a, _ in rs])
    out["rs_size"] = np.array([s for _, s in rs], np.int32)
    out["rs_out"], out["rs_out_shape"] = ragged([np.asarray(PIL.Image.fromarray(a, "RGBA").resize(s, PIL.Image.BICUBIC)) for a, s in rs])
    for i, (aug, seed, W, H) in enumerate(CHAINS):
        ims = chain_inputs(g)
        out[f"chain{i}_in"], out[f"chain{i}_in_shape"] = ragged(ims)
        opt = types.SimpleNamespace(Aug=aug, imgW=W, imgH=H)
        torch.manual_seed(seed)
        random.seed(seed)
        t = A.TextAugment(opt)
        res = torch.stack([t(PIL.Image.fromarray(a, "RGBA")) for a in ims])
        out[f"chain{i}_out"] = res.mul(0.5).add(0.5).mul(255).round().to(torch.uint8).numpy()
    out["chains"] = np.array(["|".join(str(v) for v in c) for c in CHAINS])
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
