"""Training-time text augmentation: the reference's Text_augment (data/dataset.py:249-290) for Aug strings made of Blur / Crop /
Rot tokens, on the host (PIL, the reference's semantics) and on the device (libmrn_hip.so, the same bits).

Host path -- TextAugment(opt)(image): per token, in string order,
  BlurX : RandomApply([GaussianBlur(sigma in [0.1, X])], p=0.5)     (torchvision 0.10.1 RandomApply + data/dataset.py:199-209)
  CropN : aspect-keeping random crop, ratio in [N/100, 1]           (data/dataset.py:212-233)
  RotD  : RandomRotation(D, BICUBIC, expand=True, fill=0)            (torchvision 0.10.1)
then the BICUBIC resize to imgH x imgW, ToTensor and (x - 0.5) / 0.5.  The random draws are those of the pinned torchvision:
RandomApply draws torch.rand(1) on every call, GaussianBlur random.uniform only when applied, RandomCrop random.uniform then
random.randint for x and y, RandomRotation float(torch.empty(1).uniform_(-D, D)) (a float32 angle).

Device path -- the DataLoader workers decode, make the SAME draws in the same order (plan_batch) and pack a RaggedBatch: one
uint8 RGBA pool of the decoded crops plus, per stage and sample, a descriptor of where the stage reads and writes and with which
parameters (the geometry -- crop windows, rotate matrices and output sizes -- planned here with PIL's own Python arithmetic).  The
main process uploads it and runs the kernels (mrn_amd.ops.augment_batch): a crop is a descriptor change, blur / rotate / resize
are kernels that reproduce Pillow's integer and double arithmetic bit for bit (tests/test_data_augment_gpu.py).
"""
import math
import random

import numpy as np
import PIL.Image
import PIL.ImageFilter
import torch

MAX_SIDE = 4096          # compiled-in limit of the device kernels (include/mrn_hip.h, MRN_AUG_MAX_SIDE)
DESC_INTS = 8            # ints per sample of one stage descriptor (include/mrn_hip.h)

ROT_COPY, ROT_AFFINE, ROT_180, ROT_90, ROT_270 = 0, 1, 2, 3, 4
RS_COPY, RS_H, RS_V, RS_HV, RS_VH = 0, 1, 2, 3, 4


def parse_aug(aug):
    """the reference's token parsing (data/dataset.py:254-275): str.strip of the token name's CHARACTERS, float / float/100 / int;
    malformed numbers raise as there, tokens matching none of the three are ignored, repeated tokens each add a stage"""
    stages = []
    for tok in aug.split("-"):
        if tok.startswith("Blur"):
            stages.append(("blur", float(tok.strip("Blur"))))
        if tok.startswith("Crop"):
            stages.append(("crop", float(tok.strip("Crop")) / 100))
        if tok.startswith("Rot"):
            degree = int(tok.strip("Rot"))
            if degree < 0:      # torchvision's _setup_angle
                raise ValueError("If degrees is a single number, it must be positive.")
            stages.append(("rot", degree))
    return stages


def uses_text_augment(opt, mode="train"):
    aug = getattr(opt, "Aug", "None")
    return mode == "train" and aug not in ("None", "ABINet")


# -- the random draws (identical for both paths) -----------------------------------------------------------------------------
def draw_blur(maximum):
    """RandomApply(p=0.5): torch.rand(1) on every call, skip when p < draw; then GaussianBlur's random.uniform(0.1, X)"""
    if 0.5 < torch.rand(1):
        return None
    return random.uniform(0.1, maximum)


def draw_crop(width, height, scale):
    """RandomCrop(scale=(s, 1)): (x, y, crop_width, crop_height)"""
    crop_ratio = random.uniform(scale, 1.0)
    crop_width = int(width * crop_ratio)
    crop_height = int(height * crop_ratio)
    x_start = random.randint(0, width - crop_width)
    y_start = random.randint(0, height - crop_height)
    return x_start, y_start, crop_width, crop_height


def draw_rotation(degree):
    """RandomRotation.get_params: a float32 angle in [-D, D]"""
    return float(torch.empty(1).uniform_(float(-degree), float(degree)).item())


# -- host path: PIL ------------------------------------------------------------------------------------------------------------
def pil_blur(image, sigma):
    return image.filter(PIL.ImageFilter.GaussianBlur(radius=sigma))


def pil_crop(image, box):
    x, y, cw, ch = box
    return image.crop((x, y, x + cw, y + ch))


def pil_rotate(image, angle):
    return image.rotate(angle, PIL.Image.BICUBIC, expand=True, center=None, fillcolor=(0,) * len(image.getbands()))


def to_normalized_tensor(image):
    """ToTensor + (x - 0.5) / 0.5 of an already resized image"""
    a = np.asarray(image, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div_(255.0)
    return t.sub_(0.5).div_(0.5)


def apply_host(image, stages, draws, size):
    """the PIL chain with given draws (one per stage, None = skipped blur) + the BICUBIC resize to size = (W, H) -> [C,H,W] fp32"""
    for (kind, _), d in zip(stages, draws):
        if kind == "blur" and d is not None:
            image = pil_blur(image, d)
        elif kind == "crop":
            image = pil_crop(image, d)
        elif kind == "rot":
            image = pil_rotate(image, d)
    return to_normalized_tensor(image.resize(size, PIL.Image.BICUBIC))


class TextAugment(object):
    """the reference's Text_augment on the host: draws interleaved with the PIL stages, exactly as torchvision's Compose runs them"""

    def __init__(self, opt):
        self.opt = opt
        self.stages = parse_aug(opt.Aug)

    def __call__(self, image):
        draws = []
        for kind, arg in self.stages:
            if kind == "blur":
                d = draw_blur(arg)
                if d is not None:
                    image = pil_blur(image, d)
            elif kind == "crop":
                d = draw_crop(image.size[0], image.size[1], arg)
                image = pil_crop(image, d)
            else:
                d = draw_rotation(arg)
                image = pil_rotate(image, d)
            draws.append(d)
        return to_normalized_tensor(image.resize((self.opt.imgW, self.opt.imgH), PIL.Image.BICUBIC))

    def __repr__(self):
        return f"TextAugment({self.opt.Aug!r}: {self.stages})"


# -- geometry planning with PIL's own Python arithmetic (PIL/Image.py rotate / resize) ----------------------------------------
def plan_rotate(w, h, angle):
    """Image.rotate(angle, expand=True) -> (mode, inverse affine matrix [6] or None, out_w, out_h)"""
    angle = angle % 360.0
    if angle == 0:
        return ROT_COPY, None, w, h
    if angle == 180:
        return ROT_180, None, w, h
    if angle in (90, 270):
        return (ROT_90 if angle == 90 else ROT_270), None, h, w
    center = (w / 2, h / 2)
    angle = -math.radians(angle)
    matrix = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
              round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def transform(x, y, m):
        a, b, c, d, e, f = m
        return a * x + b * y + c, d * x + e * y + f

    matrix[2], matrix[5] = transform(-center[0] - 0, -center[1] - 0, matrix)
    matrix[2] += center[0]
    matrix[5] += center[1]
    xx, yy = [], []
    for x, y in ((0, 0), (w, 0), (w, h), (0, h)):
        x, y = transform(x, y, matrix)
        xx.append(x)
        yy.append(y)
    nw = math.ceil(max(xx)) - math.floor(min(xx))
    nh = math.ceil(max(yy)) - math.floor(min(yy))
    matrix[2], matrix[5] = transform(-(nw - w) / 2.0, -(nh - h) / 2.0, matrix)
    return ROT_AFFINE, matrix, nw, nh


def gaussian_box_params(sigma):
    """Pillow's GaussianBlur(sigma) as 3 extended box passes (BoxBlur.c): the float32 box radius of _gaussian_blur_radius, then
    ImagingHorizontalBoxBlur's integer radius and 24-bit weights (ww inner, fw the two fractional edge taps).  None: a no-op."""
    f = np.float32
    radius = f(sigma)
    sigma2 = f(radius * radius) / f(3)
    L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2)
    a = a / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    box = l + a
    if box == 0:
        return None
    r = int(box)
    ww = int(f(1 << 24) / (box * f(2) + f(1)))
    fw = ((1 << 24) - (r * 2 + 1) * ww) // 2
    return r, ww, fw


def resize_mode(w, h, W, H):
    """which separable passes Image.resize((W, H), BICUBIC) of an RGBA image runs, in which order"""
    if (w, h) == (W, H):
        return RS_COPY
    if h > w * 100 and H < h:
        return RS_VH if W != w else RS_V
    if W != w and H != h:
        return RS_HV
    return RS_H if W != w else RS_V


# -- the deferred (device) batch ------------------------------------------------------------------------------------------------
class RaggedBatch(object):
    """a batch of decoded crops and their planned stages, ready for mrn_amd.ops.augment_batch:
      pool    uint8 [pixels * 4]: the source crops (RGBA, rows packed); the stages' outputs follow them on the device only
      total   pixels of the device buffer: pool + every stage's output + the resize intermediates
      kinds   the stage kinds that launch kernels, in order ("blur" / "rot"); crops are folded into the descriptors
      desc    int32 [len(kinds) + 1, B, DESC_INTS]: per kernel stage, then the final resize
      matrix  float64 [n_rot, B, 6]: inverse affine matrices of the rotate stages
      maxima  per launch stage (max w, max h of its sources, max out w, max out h)"""

    def __init__(self, pool, total, kinds, desc, matrix, maxima, size):
        self.pool, self.total, self.kinds, self.desc, self.matrix, self.maxima, self.size = pool, total, kinds, desc, matrix, maxima, size

    def __len__(self):
        return self.desc.shape[1]


def plan_batch(images, stages, size):
    """draw every sample's parameters (same order as TextAugment) and plan the device chain.
    -> (RaggedBatch, None), or (None, draws) when a sample leaves the kernels' limits (a side of 0 or above MAX_SIDE)"""
    W, H = size
    B = len(images)
    arrays = [np.asarray(im, dtype=np.uint8) for im in images]
    offs, cur = [], 0
    for a in arrays:
        offs.append(cur)
        cur += a.shape[0] * a.shape[1]
    pool_pixels = cur
    kinds = [k for k, _ in stages if k != "crop"]
    desc = np.zeros((len(kinds) + 1, B, DESC_INTS), np.int32)
    matrix = np.zeros((kinds.count("rot"), B, 6), np.float64)
    all_draws = []
    fits = True
    maxima = [[1, 1, 1, 1] for _ in range(len(kinds) + 1)]
    for b, a in enumerate(arrays):
        h, w = a.shape[:2]
        off, stride = offs[b], w
        ok = 0 < w <= MAX_SIDE and 0 < h <= MAX_SIDE
        draws, si, ri = [], 0, 0
        for kind, arg in stages:
            if kind == "blur":
                d = draw_blur(arg)
                bp = gaussian_box_params(d) if d is not None else None
                rec = desc[si, b]
                rec[:4] = (off, stride, w, h)
                if bp is None:
                    rec[4:] = (off, -1, 0, 0)
                else:
                    rec[4:] = (cur, bp[0], bp[1], bp[2])
                    off, stride = cur, w
                    cur += w * h
                m = maxima[si]
                m[0], m[1], m[2], m[3] = max(m[0], w), max(m[1], h), max(m[2], w), max(m[3], h)
                si += 1
            elif kind == "crop":
                d = draw_crop(w, h, arg)
                x, y, w, h = d
                off += y * stride + x
            else:
                d = draw_rotation(arg)
                mode, mat, ow, oh = plan_rotate(w, h, d)
                rec = desc[si, b]
                rec[:] = (off, stride, w, h, cur if mode != ROT_COPY else off, ow, oh, mode)
                if mat is not None:
                    matrix[ri, b] = mat
                m = maxima[si]
                m[0], m[1], m[2], m[3] = max(m[0], w), max(m[1], h), max(m[2], ow), max(m[3], oh)
                if mode != ROT_COPY:
                    off, stride = cur, ow
                    cur += ow * oh
                w, h = ow, oh
                si += 1
                ri += 1
            draws.append(d)
            ok = ok and 0 < w <= MAX_SIDE and 0 < h <= MAX_SIDE
        all_draws.append(draws)
        fits = fits and ok
        mode = resize_mode(w, h, W, H)
        tmp = 0
        if mode == RS_HV:
            tmp, cur = cur, cur + W * h
        elif mode == RS_VH:
            tmp, cur = cur, cur + w * H
        desc[si, b, :6] = (off, stride, w, h, tmp, mode)
        m = maxima[si]
        m[0], m[1] = max(m[0], w), max(m[1], h)
    if not fits or cur >= 2 ** 31:
        return None, all_draws
    pool = np.empty(pool_pixels * 4, np.uint8)
    for a, o in zip(arrays, offs):
        pool[o * 4:o * 4 + a.size] = a.reshape(-1)
    return RaggedBatch(pool, cur, kinds, desc, matrix, [tuple(m) for m in maxima], size), None
