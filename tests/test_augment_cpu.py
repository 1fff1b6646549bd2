"""Training-time text augmentation on the host (mrn_amd/data/augment.py): the reference's Text_augment for Aug strings of Blur / Crop /
Rot tokens (data/dataset.py:249-290 under torchvision 0.10.1), restated through PIL, and the planner the device path relies on."""
import random
import types

import numpy as np
import PIL.Image
import PIL.ImageFilter
import pytest
import torch

from mrn_amd.data import augment as A
from mrn_amd.data.dataset import AlignCollate, AlignCollate2, ResizeNormalize


def make_opt(**kw):
    o = types.SimpleNamespace(imgH=32, imgW=256, Aug="Blur5-Crop90-Rot15")
    o.__dict__.update(kw)
    return o


def crops(n, seed, wr=(40, 200), hr=(24, 48)):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        w, h = int(g.integers(*wr)), int(g.integers(*hr))
        a = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
        a[..., 3] = np.where(g.random((h, w)) < 0.4, 255, a[..., 3])
        a[: h // 4, :, 3] = 0
        out.append(PIL.Image.fromarray(a, "RGBA"))
    return out


def test_align_collate_augments_train_batches():
    ims = crops(6, 0)
    batch = [(im, f"w{i}") for i, im in enumerate(ims)]
    images, labels = AlignCollate(make_opt(), "train")(batch)
    assert images.shape == (6, 4, 32, 256) and images.dtype == torch.float32
    assert float(images.min()) >= -1.0 and float(images.max()) <= 1.0
    assert labels == tuple(f"w{i}" for i in range(6))
    images2, labels2, index = AlignCollate2(make_opt(), "train")([(b, i % 2) for i, b in enumerate(batch)])
    assert images2.shape == (6, 4, 32, 256) and index == (0, 1, 0, 1, 0, 1)


def explicit_reference(image, aug, W=256, H=32):
    """the reference's chain spelled out: torchvision 0.10.1's draws, then the PIL calls they lead to"""
    for tok in aug.split("-"):
        if tok.startswith("Blur"):
            if not (0.5 < torch.rand(1)):
                sigma = random.uniform(0.1, float(tok.strip("Blur")))
                image = image.filter(PIL.ImageFilter.GaussianBlur(radius=sigma))
        if tok.startswith("Crop"):
            w, h = image.size
            r = random.uniform(float(tok.strip("Crop")) / 100, 1.0)
            cw, ch = int(w * r), int(h * r)
            x, y = random.randint(0, w - cw), random.randint(0, h - ch)
            image = image.crop((x, y, x + cw, y + ch))
        if tok.startswith("Rot"):
            d = int(tok.strip("Rot"))
            angle = float(torch.empty(1).uniform_(float(-d), float(d)).item())
            image = image.rotate(angle, PIL.Image.BICUBIC, expand=True, fillcolor=(0, 0, 0, 0))
    a = np.asarray(image.resize((W, H), PIL.Image.BICUBIC))
    return torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255).sub(0.5).div(0.5)


@pytest.mark.parametrize("aug", ["Blur5-Crop90-Rot15", "Rot30-Blur2-Crop80", "Crop50-Crop50", "Rot90", "Blur0.1-Blur3"])
def test_host_path_equals_the_explicit_draws(aug):
    ims = crops(8, 1)
    torch.manual_seed(3)
    random.seed(3)
    got = AlignCollate(make_opt(Aug=aug), "train")([(im, "x") for im in ims])[0]
    torch.manual_seed(3)
    random.seed(3)
    want = torch.stack([explicit_reference(im, aug) for im in ims])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_parsing_quirks():
    assert A.parse_aug("Blur5-Crop90-Rot15") == [("blur", 5.0), ("crop", 0.9), ("rot", 15)]
    assert A.parse_aug("Blur5-Blur3") == [("blur", 5.0), ("blur", 3.0)]          # repeated tokens each add a stage
    assert A.parse_aug("Foo-Rot10-bar") == [("rot", 10)]                          # unknown tokens are ignored
    assert A.parse_aug("Blurr2r") == [("blur", 2.0)]                              # strip() removes the name's characters
    assert A.parse_aug("Cropo80") == [("crop", 0.8)]
    assert A.parse_aug("RotoR7t") == [("rot", 7)]
    with pytest.raises(ValueError):
        A.parse_aug("Blur")                                                       # float('')
    with pytest.raises(ValueError):
        A.parse_aug("Rot7.5")                                                     # int('7.5')
    with pytest.raises(ValueError):
        A.parse_aug("Cropx")


def test_unchanged_modes():
    ims = crops(3, 2)
    batch = [(im, "a") for im in ims]
    want = torch.stack([ResizeNormalize((256, 32))(im) for im in ims])
    for opt, mode in [(make_opt(Aug="None"), "train"), (make_opt(), "test"), (make_opt(Aug="ABINet"), "test")]:
        got = AlignCollate(opt, mode)(batch)[0]
        assert torch.equal(got, want)
    with pytest.raises(NotImplementedError, match="cv2"):
        AlignCollate(make_opt(Aug="ABINet"), "train")


def test_crop_above_100_raises_like_the_reference():
    with pytest.raises(ValueError):
        AlignCollate(make_opt(Aug="Crop120"), "train")([(crops(1, 4)[0], "a")])


def test_rotate_planner_sizes_equal_pil():
    g = np.random.default_rng(5)
    angles = [0.0, 90.0, -90.0, 180.0, 270.0, -180.0, 1e-6, -1e-6, 15.0, -15.0, 45.0, 359.99997]
    angles += [float(np.float32(a)) for a in g.uniform(-180, 180, 60)]
    for w, h in [(1, 1), (1, 7), (9, 1), (37, 24), (200, 48), (64, 64), (3, 500), (0, 12)]:
        im = PIL.Image.new("RGBA", (w, h))
        for a in angles:
            mode, mat, ow, oh = A.plan_rotate(w, h, a)
            assert (ow, oh) == im.rotate(a, PIL.Image.BICUBIC, expand=True).size, (w, h, a)
    assert A.plan_rotate(10, 5, 90.0)[0] == A.ROT_90 and A.plan_rotate(10, 5, -90.0)[0] == A.ROT_270
    assert A.plan_rotate(10, 5, 0.0)[0] == A.ROT_COPY and A.plan_rotate(10, 5, 180.0)[0] == A.ROT_180


def test_planner_draws_match_host_path():
    """the deferred collate consumes the same RNG streams as the host path and plans the same geometry"""
    ims = crops(12, 6)
    opt = make_opt(Aug="Rot20-Crop70-Blur4-Rot5")
    torch.manual_seed(9)
    random.seed(9)
    rb, _ = A.plan_batch(ims, A.parse_aug(opt.Aug), (256, 32))
    after = (torch.rand(1).item(), random.random())
    torch.manual_seed(9)
    random.seed(9)
    sizes = []
    for im in ims:
        t = A.TextAugment(opt)
        img = im
        for kind, arg in t.stages:            # the host chain, recording the size before the final resize
            if kind == "blur":
                d = A.draw_blur(arg)
                img = img if d is None else A.pil_blur(img, d)
            elif kind == "crop":
                img = A.pil_crop(img, A.draw_crop(img.size[0], img.size[1], arg))
            else:
                img = A.pil_rotate(img, A.draw_rotation(arg))
        sizes.append(img.size)
    assert after == (torch.rand(1).item(), random.random())
    final = rb.desc[-1]
    assert [(int(d[2]), int(d[3])) for d in final] == sizes


def test_limits_fall_back_to_the_host_path():
    """zero-width crops (int(w * ratio) == 0) leave the kernels' limits: the deferred collate gives the host path's bits"""
    from mrn_amd.data.data_manage import DeferredCollate
    ims = crops(4, 7, (1, 2), (20, 30))
    opt = make_opt(Aug="Crop60-Rot10")
    torch.manual_seed(1)
    random.seed(1)
    got = DeferredCollate(opt)([(im, "a") for im in ims])[0]
    torch.manual_seed(1)
    random.seed(1)
    want = AlignCollate(opt, "train")([(im, "a") for im in ims])[0]
    assert isinstance(got, torch.Tensor) and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_gaussian_box_params():
    # Pillow's own box radius for sigma = 2: sigma^2 / 3 per pass (BoxBlur.c) -> integer part 1
    r, ww, fw = A.gaussian_box_params(2.0)
    assert r == 1 and (2 * r + 1) * ww + 2 * fw <= 1 << 24
    assert A.gaussian_box_params(0.1)[0] == 0
