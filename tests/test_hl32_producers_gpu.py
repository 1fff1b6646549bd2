"""The pure-layout producers of HL32 operands against a torch restatement of the format, byte for byte.

HL32 is one 128-byte line [hi fp16 x 32 | lo fp16 x 32] per (row, 32 channels) with hi = fp16(x), lo = fp16(x - hi); a power-of-two
prescale is an exact fp32 multiply before the split.  Each producer only decides WHERE an element lands (and where zeros go), so the
restatement places the scaled fp32 values by the producer's documented index formula, splits them on the CPU and the bytes must agree
(every byte: the many lo halves that are fp16 subnormals at unit magnitude included -- the kernels' conversions keep them).
(The two Winograd-transforming producers do arithmetic and stay under test_wgrad_in_the_winograd_domain / test_winograd_conv_matches_direct.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def scale_pair(s):
    return None if s is None else torch.tensor([s, 1.0 / s], dtype=torch.float32, device="cuda")


def hl32_lines(v):
    """fp32 [..., 32] (already scaled and placed, zeros included) -> fp16 [..., 2, 32]: the hi half and the lo half of every line"""
    assert v.dtype == torch.float32 and v.shape[-1] == 32
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.stack((hi, lo), dim=-2)


def assert_same_bytes(name, got_u8, want):
    got = got_u8.cpu().view(torch.int16)
    want = want.contiguous().view(torch.int16).reshape(-1)
    assert got.numel() == want.numel(), (name, got.numel(), want.numel())
    bad = (got != want).nonzero().flatten()
    half = (bad // 32) % 2                                   # 0 = a hi half, 1 = a lo half
    assert bad.numel() == 0, (f"{name}: {bad.numel()} of {want.numel()} halves differ ({int((half == 0).sum())} hi, {int((half == 1).sum())} lo); "
                              f"first at {int(bad[0])}: got {int(got[bad[0]]):#x} want {int(want[bad[0]]):#x}")


@pytest.mark.parametrize("rows,C,s", [(3, 32, None), (67, 96, 0.25), (67, 96, 4.0)])
def test_split_hl32(ops, rows, C, s):
    """out[row][C/32][hi 32 | lo 32]"""
    x = rnd(rows, C, seed=1)
    got = ops.split_hl32(x.cuda(), scale_pair(s))
    assert_same_bytes("split_hl32", got, hl32_lines((x * (s or 1.0)).view(rows, C // 32, 32)))


def transposed_lines(x, padded, S, s):
    """[S][C][padded / S / 32][line]: element (c, r) of matrix k is s * x[k * padded / S + r][c], zero beyond x's rows"""
    rows, C = x.shape
    xp = torch.zeros(padded, C)
    xp[:rows] = x * (s or 1.0)
    return hl32_lines(xp.view(S, padded // S, C).permute(0, 2, 1).reshape(S, C, padded // S // 32, 32))


@pytest.mark.parametrize("rows,padded,C,S,s", [(32, 32, 4, 1, None), (70, 128, 36, 2, 8.0)])
def test_split_hl32_t(ops, rows, padded, C, S, s):
    """ragged last row block, a last channel tile of 4, zero lines beyond `rows`, two split-K matrices"""
    x = rnd(rows, C, seed=2)
    got = ops.split_hl32_t(x.cuda(), S, scale_pair(s), rows_padded=padded)
    assert_same_bytes("split_hl32_t", got, transposed_lines(x, padded, S, s))


def test_split_hl32_t_with_column_sums(ops):
    """the column-sum form writes the same operand (its sums: test_transposed_split_with_column_sums)"""
    rows, padded, C, S, s = 70, 128, 36, 2, 8.0
    x = rnd(rows, C, seed=2)
    got = ops.split_hl32_t(x.cuda(), S, scale_pair(s), rows_padded=padded, colsum_out=torch.empty(C, device="cuda"))
    assert_same_bytes("split_hl32_t colsum", got, transposed_lines(x, padded, S, s))


@pytest.mark.parametrize("B,H,W,C,k,st,pad,S,s", [(2, 3, 5, 36, (3, 3), (1, 1), (1, 1), 1, None), (2, 5, 6, 36, (2, 2), (2, 2), (0, 0), 2, 0.5)])
def test_im2col_t_hl32(ops, B, H, W, C, k, st, pad, S, s):
    """out[S][tap][ci][rps / 32][line], element (tap, ci, p) = s * x[b][oy * sh + ky - ph][ox * sw + kx - pw][ci] for the output pixel
    p = (b * Ho + oy) * Wo + ox (zero outside the image and beyond B * Ho * Wo)"""
    (kh, kw), (sh, sw), (ph, pw) = k, st, pad
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    P = B * Ho * Wo
    padded = -(-P // (32 * S)) * 32 * S
    x = rnd(B, H, W, C, seed=3)
    xd, sc, out = x.cuda(), scale_pair(s), torch.empty(kh * kw * C * padded * 4, device="cuda", dtype=torch.uint8)
    ops.call("mrn_im2col_t_hl32_f32", xd.data_ptr(), out.data_ptr(), B, H, W, C, kh, kw, sh, sw, ph, pw, padded, S, ops._p(sc), ops._stream())
    xs = torch.zeros(B, H + 2 * ph, W + 2 * pw, C)
    xs[:, ph:ph + H, pw:pw + W] = x * (s or 1.0)
    cols = torch.zeros(kh * kw, padded, C)
    for ky in range(kh):
        for kx in range(kw):
            cols[ky * kw + kx, :P] = xs[:, ky:ky + sh * (Ho - 1) + 1:sh, kx:kx + sw * (Wo - 1) + 1:sw].reshape(P, C)
    want = cols.view(kh * kw, S, padded // S, C).permute(1, 0, 3, 2).reshape(S, kh * kw, C, padded // S // 32, 32)
    assert_same_bytes("im2col_t_hl32", out, hl32_lines(want))


def transpose_oy_lines(x, shift, s):
    """[C][ceil(B*H*W / 32)][line] over k = (y * B + b) * W + xx, element (c, k) = s * x[b][y][xx + shift][c], zero outside the row"""
    B, H, W, C = x.shape
    sh = torch.zeros(B, H, W, C)
    lo, hi = max(0, -shift), W - max(0, shift)
    sh[:, :, lo:hi] = x[:, :, lo + shift:hi + shift] * s
    P = B * H * W
    lines = (P + 31) // 32
    flat = torch.zeros(lines * 32, C)
    flat[:P] = sh.permute(1, 0, 2, 3).reshape(P, C)
    return hl32_lines(flat.t().reshape(C, lines, 32))


@pytest.fixture(scope="module")
def oy_case():
    return rnd(2, 3, 16, 36, seed=4), 2.0


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_transpose_oy_hl32(ops, oy_case, shift):
    x, s = oy_case
    got = ops.transpose_oy_hl32(x.cuda(), shift, scale_pair(s))
    assert_same_bytes(f"transpose_oy_hl32 shift {shift}", got, transpose_oy_lines(x, shift, s))


def test_transpose_oy3_hl32(ops, oy_case):
    """the three shifted copies from one read equal the three single passes"""
    x, s = oy_case
    B, H, W, C = x.shape
    xd, sc = x.cuda(), scale_pair(s)
    out = torch.empty(3 * C * ((B * H * W + 31) // 32) * 128, device="cuda", dtype=torch.uint8)
    ops.call("mrn_transpose_oy3_hl32_f32", xd.data_ptr(), out.data_ptr(), B, H, W, C, sc.data_ptr(), ops._stream())
    assert torch.equal(out, torch.cat([ops.transpose_oy_hl32(xd, shift, sc) for shift in (-1, 0, 1)]))
    assert_same_bytes("transpose_oy3_hl32", out, torch.stack([transpose_oy_lines(x, shift, s) for shift in (-1, 0, 1)]))


@pytest.mark.parametrize("s", [1.0, 4.0])
def test_pack_weights_hl32(ops, s):
    """w [Cout][taps][Cin] -> [Cout][Cin / 32][taps][line] of s * w"""
    Cout, taps, Cin = 5, 9, 64
    w = rnd(Cout, 3, 3, Cin, seed=5)
    got, _ = ops.pack_weights_hl32([w.cuda()], scale=scale_pair(s).view(1, 2))
    assert_same_bytes("pack_weights_hl32", got, hl32_lines((w * s).view(Cout, taps, Cin // 32, 32).permute(0, 2, 1, 3).contiguous()))
