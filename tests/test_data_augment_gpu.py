"""The augmentation kernels (mrn_amd/csrc/augment.hip) against Pillow, bit for bit: the committed fixture
(tests/golden/augment_pil.npz, tests/golden/make_golden_augment.py) and live PIL; Dataset_Manager's device-augmented batches
against its host path."""
import contextlib
import io
import os
import random
import types

import numpy as np
import PIL.Image
import pytest
import torch

from mrn_amd.data import augment as A

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_pil.npz")


def unpack(flat, shapes):
    out, o = [], 0
    for h, w in shapes:
        out.append(flat[o:o + h * w * 4].reshape(h, w, 4))
        o += h * w * 4
    return out


def pool_of(arrays):
    offs, cur = [], 0
    for a in arrays:
        offs.append(cur)
        cur += a.shape[0] * a.shape[1]
    return np.concatenate([a.reshape(-1) for a in arrays]), offs, cur


def device_blur(arrays, sigmas):
    from mrn_amd import ops
    pool, offs, cur = pool_of(arrays)
    desc = np.zeros((len(arrays), 8), np.int32)
    dst = []
    for b, (a, s) in enumerate(zip(arrays, sigmas)):
        h, w = a.shape[:2]
        r, ww, fw = A.gaussian_box_params(s) or (-1, 0, 0)
        desc[b] = (offs[b], w, w, h, cur, r, ww, fw)
        dst.append(cur if r >= 0 else offs[b])
        cur += w * h
    px = torch.zeros(cur * 4, dtype=torch.uint8, device="cuda")
    px[:pool.size] = torch.from_numpy(pool).cuda()
    ops.aug_gaussian_blur(px, torch.from_numpy(desc).cuda(), max(a.shape[1] for a in arrays), max(a.shape[0] for a in arrays))
    host = px.cpu().numpy()
    return [host[d * 4:(d + a.shape[0] * a.shape[1]) * 4].reshape(a.shape) for a, d in zip(arrays, dst)]


def device_rotate(arrays, angles):
    from mrn_amd import ops
    pool, offs, cur = pool_of(arrays)
    desc = np.zeros((len(arrays), 8), np.int32)
    mat = np.zeros((len(arrays), 6), np.float64)
    res = []
    for b, (a, ang) in enumerate(zip(arrays, angles)):
        h, w = a.shape[:2]
        mode, m, ow, oh = A.plan_rotate(w, h, ang)
        dst = cur if mode != A.ROT_COPY else offs[b]
        desc[b] = (offs[b], w, w, h, dst, ow, oh, mode)
        if m is not None:
            mat[b] = m
        res.append((dst, oh, ow))
        if mode != A.ROT_COPY:
            cur += ow * oh
    px = torch.zeros(cur * 4, dtype=torch.uint8, device="cuda")
    px[:pool.size] = torch.from_numpy(pool).cuda()
    ops.aug_rotate(px, torch.from_numpy(desc).cuda(), torch.from_numpy(mat).cuda(), max(r[2] for r in res), max(r[1] for r in res))
    host = px.cpu().numpy()
    return [host[d * 4:(d + oh * ow) * 4].reshape(oh, ow, 4) for d, oh, ow in res]


def device_resize(arrays, size):
    from mrn_amd import ops
    W, H = size
    pool, offs, cur = pool_of(arrays)
    desc = np.zeros((len(arrays), 8), np.int32)
    for b, a in enumerate(arrays):
        h, w = a.shape[:2]
        mode = A.resize_mode(w, h, W, H)
        tmp = 0
        if mode == A.RS_HV:
            tmp, cur = cur, cur + W * h
        elif mode == A.RS_VH:
            tmp, cur = cur, cur + w * H
        desc[b, :6] = (offs[b], w, w, h, tmp, mode)
    px = torch.zeros(cur * 4, dtype=torch.uint8, device="cuda")
    px[:pool.size] = torch.from_numpy(pool).cuda()
    out = torch.full((len(arrays) + 1, 4, H, W), 7.0, device="cuda")
    ops.aug_resize_normalize(px, torch.from_numpy(desc).cuda(), max(a.shape[1] for a in arrays), max(a.shape[0] for a in arrays),
                             out, row0=1)
    out = out.cpu()
    assert torch.all(out[0] == 7.0)                 # row offset: nothing written before row0
    return out[1:]


def norm(u8_hwc):
    return A.to_normalized_tensor(PIL.Image.fromarray(np.ascontiguousarray(u8_hwc), "RGBA"))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_blur_equals_pillow(golden):
    ins = unpack(golden["blur_in"], golden["blur_in_shape"])
    want = unpack(golden["blur_out"], golden["blur_in_shape"])
    got = device_blur(ins, golden["blur_sigma"])
    for a, s, g, w in zip(ins, golden["blur_sigma"], got, want):
        assert np.array_equal(g, w), (a.shape, s)
        live = np.asarray(A.pil_blur(PIL.Image.fromarray(a, "RGBA"), float(s)))
        assert np.array_equal(g, live), (a.shape, s)


def test_blur_radii_sweep_live():
    g = np.random.default_rng(11)
    arrays = [g.integers(0, 256, (int(g.integers(1, 50)), int(g.integers(1, 150)), 4), dtype=np.uint8) for _ in range(40)]
    sigmas = list(np.linspace(0.1, 8.0, 40))
    got = device_blur(arrays, sigmas)
    for a, s, r in zip(arrays, sigmas, got):
        assert np.array_equal(r, np.asarray(A.pil_blur(PIL.Image.fromarray(a, "RGBA"), float(s)))), (a.shape, s)


def test_rotate_equals_pillow(golden):
    ins = unpack(golden["rot_in"], golden["rot_in_shape"])
    want = unpack(golden["rot_out"], golden["rot_out_shape"])
    got = device_rotate(ins, golden["rot_angle"])
    for a, ang, g, w in zip(ins, golden["rot_angle"], got, want):
        assert np.array_equal(g, w), (a.shape, ang)
        assert np.array_equal(g, np.asarray(A.pil_rotate(PIL.Image.fromarray(a, "RGBA"), float(ang)))), (a.shape, ang)


def test_premultiply_round_trip_exhaustive():
    """every (c, a) pair: an identity affine samples pixel centres exactly (dx = dy = 0), so the kernel's output is
    un-premultiply(premultiply(p)) -- Pillow's convert('RGBa').convert('RGBA')"""
    from mrn_amd import ops
    c = np.arange(256, dtype=np.uint8)
    img = np.zeros((256, 256, 4), np.uint8)
    img[..., 0] = c[:, None]
    img[..., 1] = 255 - c[:, None]
    img[..., 2] = c[:, None] // 3
    img[..., 3] = c[None, :]
    n = 256 * 256
    px = torch.zeros(2 * n * 4, dtype=torch.uint8, device="cuda")
    px[:n * 4] = torch.from_numpy(img.reshape(-1)).cuda()
    desc = torch.tensor([[0, 256, 256, 256, n, 256, 256, A.ROT_AFFINE]], dtype=torch.int32, device="cuda")
    mat = torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], dtype=torch.float64, device="cuda")
    ops.aug_rotate(px, desc, mat, 256, 256)
    got = px[n * 4:].cpu().numpy().reshape(256, 256, 4)
    want = np.asarray(PIL.Image.fromarray(img, "RGBA").convert("RGBa").convert("RGBA"))
    assert np.array_equal(got, want)
    live = PIL.Image.fromarray(img, "RGBA").transform((256, 256), PIL.Image.AFFINE, (1, 0, 0, 0, 1, 0), PIL.Image.BICUBIC)
    assert np.array_equal(got, np.asarray(live))


def test_resize_equals_pillow(golden):
    ins = unpack(golden["rs_in"], golden["rs_in_shape"])
    want = unpack(golden["rs_out"], golden["rs_out_shape"])
    sizes = [tuple(int(v) for v in s) for s in golden["rs_size"]]
    for size in sorted(set(sizes)):
        idx = [i for i, s in enumerate(sizes) if s == size]
        got = device_resize([ins[i] for i in idx], size)
        for j, i in enumerate(idx):
            w = norm(want[i])
            assert torch.equal(got[j].view(torch.int32), w.view(torch.int32)), (ins[i].shape, size)
            live = A.to_normalized_tensor(PIL.Image.fromarray(ins[i], "RGBA").resize(size, PIL.Image.BICUBIC))
            assert torch.equal(got[j].view(torch.int32), live.view(torch.int32)), (ins[i].shape, size)


def test_resize_widths_1_to_1000_live():
    g = np.random.default_rng(12)
    widths = [1, 2, 3, 7, 31, 64, 127, 128, 129, 255, 256, 257, 333, 512, 700, 999, 1000]
    arrays = [g.integers(0, 256, (int(g.integers(8, 60)), w, 4), dtype=np.uint8) for w in widths]
    got = device_resize(arrays, (256, 32))
    for a, r in zip(arrays, got):
        live = A.to_normalized_tensor(PIL.Image.fromarray(a, "RGBA").resize((256, 32), PIL.Image.BICUBIC))
        assert torch.equal(r.view(torch.int32), live.view(torch.int32)), a.shape


@pytest.mark.parametrize("i", range(4))
def test_chains_equal_the_host_path(golden, i):
    from mrn_amd import ops
    aug, seed, W, H = str(golden["chains"][i]).split("|")
    W, H = int(W), int(H)
    ims = [PIL.Image.fromarray(a, "RGBA") for a in unpack(golden[f"chain{i}_in"], golden[f"chain{i}_in_shape"])]
    torch.manual_seed(int(seed))
    random.seed(int(seed))
    rb, _ = A.plan_batch(ims, A.parse_aug(aug), (W, H))
    px = torch.zeros(rb.total * 4, dtype=torch.uint8, device="cuda")
    px[:rb.pool.size] = torch.from_numpy(rb.pool).cuda()
    out = torch.empty((len(ims), 4, H, W), device="cuda")
    ops.augment_batch(px, rb, torch.from_numpy(rb.desc).cuda(), torch.from_numpy(rb.matrix).cuda(), out)
    want = torch.from_numpy(golden[f"chain{i}_out"]).float().div(255).sub(0.5).div(0.5)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))
    torch.manual_seed(int(seed))
    random.seed(int(seed))
    t = A.TextAugment(types.SimpleNamespace(Aug=aug, imgW=W, imgH=H))
    live = torch.stack([t(im) for im in ims])
    assert torch.equal(out.cpu().view(torch.int32), live.view(torch.int32))


def test_out_of_limit_calls_return_errors():
    from mrn_amd import ops
    px = torch.zeros(64, dtype=torch.uint8, device="cuda")
    desc = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="outside"):
        ops.aug_gaussian_blur(px, desc, 5000, 4)
    with pytest.raises(RuntimeError, match="outside"):
        ops.aug_rotate(px, desc, torch.zeros((1, 6), dtype=torch.float64, device="cuda"), 4, 0)


def _manager_batches(opt, with_index, n=3):
    from mrn_amd.data.data_manage import Dataset_Manager
    from tests.test_data_cpu import open_fake
    torch.manual_seed(5)
    random.seed(5)
    np.random.seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        dm = Dataset_Manager(opt, open_dataset=open_fake)
        dm.select_data = opt.select_data
        if with_index:
            dm.get_dataset(2, memory="random", index_list=[np.arange(10)] * 2)
        else:
            dm.get_dataset(1, memory=None)
    out = []
    for _ in range(n):
        got = dm.get_batch2() if with_index else dm.get_batch()
        out.append((got[0].cpu(),) + tuple(got[1:]))
    return out, dm


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("with_index", [False, True])
def test_dataset_manager_device_batches_equal_host(workers, with_index):
    from tests.test_data_cpu import make_opt
    aug = "Blur5-Crop90-Rot15"
    host, dm_h = _manager_batches(make_opt(Aug=aug, workers=workers, device_prefetch=False), with_index)
    dev, dm_d = _manager_batches(make_opt(Aug=aug, workers=workers, device_prefetch=True), with_index)
    assert dm_h.stager.stream is None and dm_d.stager.stream is not None
    assert type(dm_d.data_loader_list[0].collate_fn).__name__ == "DeferredCollate"
    for h, d in zip(host, dev):
        assert h[0].shape == d[0].shape and h[0].shape[1:] == (4, 32, 256)
        assert torch.equal(h[0].view(torch.int32), d[0].view(torch.int32))
        assert list(h[1]) == list(d[1])
        if with_index:
            assert [list(x) for x in h[2]] == [list(x) for x in d[2]]
