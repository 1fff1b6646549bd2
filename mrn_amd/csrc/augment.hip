// Training-time text augmentation of ragged RGBA uint8 batches (the reference's Text_augment, data/dataset.py:249-290: PIL
// GaussianBlur / crop / RandomRotation(BICUBIC, expand=True) and the BICUBIC resize + ToTensor + (x - 0.5) / 0.5), bit-exact
// with Pillow.  One RGBA pixel is one dword, so lanes map to pixels.  Every sample is a window (offset, stride, w, h) into one
// pixel buffer: the host packs the decoded crops at its start and plans where every stage writes (mrn_amd/data/augment.py); a
// crop is a window change and launches nothing.
//
// What "bit-exact" pins down (Pillow's C, restated from its observable behaviour and checked against it by
// tests/test_data_augment_gpu.py):
//   - GaussianBlur (BoxBlur.c): 3 extended-box passes along x, then 3 along y, each rounded to uint8; a pass is an integer window
//     sum with edge replication, acc * ww + (left + right outer taps) * fw, (+ 2^23) >> 24 -- order-independent integers.
//     The box radius / weights come from the host (float32 arithmetic of _gaussian_blur_radius).  No alpha premultiply.
//   - rotate / resize of RGBA go through premultiplied RGBa: c' = MULDIV255(c, a) there, c = min(255, 255 c' / a) back
//     (alpha 0 and 255 pass through).
//   - rotate (Geometry.c): the inverse affine at pixel centres, Geometry's double-precision cubic (a = -0.5 in Horner form) with
//     edge clamping, fill 0 outside [0, w) x [0, h), truncation to uint8.  Exact 90 / 180 / 270 degrees are transposes.
//   - resize (Resample.c, 8 bpc): bicubic a = -0.5 with support scaled on downscale, fp64 coefficients normalised per output
//     pixel and rounded to 22-bit fixed point, int32 accumulation from 2^21, horizontal pass before vertical, only the passes
//     Pillow runs (a pass along an unchanged axis is skipped; images taller than 100x their width go vertical first).
// x86 Pillow builds do not contract a*b + c into FMAs; neither does this file.
#include "common.hpp"

#pragma clang fp contract(off)

#define MRN_AUG_MAX_SIDE 4096

namespace {

constexpr int kPrec = 22;                                        // Resample.c PRECISION_BITS (32 - 8 - 2)

__device__ __forceinline__ unsigned chan(unsigned p, int c) { return (p >> (8 * c)) & 255u; }

__device__ __forceinline__ unsigned muldiv255(unsigned a, unsigned b) {
  const unsigned t = a * b + 128u;
  return ((t >> 8) + t) >> 8;
}

__device__ __forceinline__ unsigned premultiply(unsigned p) {
  const unsigned a = p >> 24;
  return muldiv255(chan(p, 0), a) | (muldiv255(chan(p, 1), a) << 8) | (muldiv255(chan(p, 2), a) << 16) | (a << 24);
}

__device__ __forceinline__ unsigned unpremultiply(unsigned p) {
  const unsigned a = p >> 24;
  if (a == 0u || a == 255u) return p;
  unsigned out = a << 24;
#pragma unroll
  for (int c = 0; c < 3; ++c) out |= min(255u, (255u * chan(p, c)) / a) << (8 * c);
  return out;
}

// a sample's window lies inside the buffer and the compiled-in limits (a window that does not is skipped: never read or written)
__device__ __forceinline__ bool window_ok(long off, long stride, int w, int h, long n) {
  return w > 0 && h > 0 && w <= MRN_AUG_MAX_SIDE && h <= MRN_AUG_MAX_SIDE && off >= 0 && stride >= w &&
         off + (long)(h - 1) * stride + w <= n;
}

// ---- GaussianBlur --------------------------------------------------------------------------------------------------------

// one extended-box pass over a line of n pixels in LDS
__device__ void box_pass(const unsigned* __restrict__ in, unsigned* __restrict__ out, int n, int r, unsigned ww, unsigned fw) {
  const int last = n - 1;
  for (int x = threadIdx.x; x < n; x += blockDim.x) {
    const int lo = x - r, hi = x + r;
    const int lo_c = max(lo, 0), hi_c = min(hi, last);
    const unsigned nl = lo < 0 ? (unsigned)(-lo) : 0u, nr = hi > last ? (unsigned)(hi - last) : 0u;
    const unsigned p0 = in[0], pl = in[last];
    unsigned acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = nl * chan(p0, c) + nr * chan(pl, c);
    for (int i = lo_c; i <= hi_c; ++i) {
      const unsigned p = in[i];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += chan(p, c);
    }
    const unsigned left = in[max(lo - 1, 0)], right = in[min(hi + 1, last)];
    unsigned v = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned bulk = acc[c] * ww + (chan(left, c) + chan(right, c)) * fw;
      v |= ((bulk + (1u << 23)) >> 24) << (8 * c);
    }
    out[x] = v;
  }
}

// desc per sample: {src_off, src_stride, w, h, dst_off, radius, ww, fw}; radius < 0: the sample is not blurred.
// vertical == 0: rows of src -> rows of dst (stride w); vertical == 1: columns of dst in place.  One wave per line.
__global__ __launch_bounds__(64) void box_blur3_kernel(unsigned* __restrict__ px, long n, const int* __restrict__ desc,
                                                       int vertical) {
  __shared__ unsigned buf[2][MRN_AUG_MAX_SIDE];
  const int* d = desc + blockIdx.y * 8;
  const int r = d[5];
  if (r < 0) return;
  const long src = d[0], sstride = d[1], dst = d[4];
  const int w = d[2], h = d[3];
  if (!window_ok(src, sstride, w, h, n) || !window_ok(dst, w, w, h, n)) return;
  const int line = blockIdx.x;
  const int len = vertical ? h : w;
  if (line >= (vertical ? w : h)) return;
  const unsigned ww = (unsigned)d[6], fw = (unsigned)d[7];
  const long base = vertical ? dst + line : src + (long)line * sstride;
  const long step = vertical ? w : 1;
  for (int i = threadIdx.x; i < len; i += blockDim.x) buf[0][i] = px[base + i * step];
  __syncthreads();
  box_pass(buf[0], buf[1], len, r, ww, fw);
  __syncthreads();
  box_pass(buf[1], buf[0], len, r, ww, fw);
  __syncthreads();
  box_pass(buf[0], buf[1], len, r, ww, fw);
  __syncthreads();
  const long obase = vertical ? base : dst + (long)line * w;
  for (int i = threadIdx.x; i < len; i += blockDim.x) px[obase + i * step] = buf[1][i];
}

// ---- rotate --------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// desc per sample: {src_off, src_stride, w, h, dst_off, out_w, out_h, mode}; mode 0 = nothing to do (0 degrees), 1 = inverse
// affine (matrix: 6 doubles per sample), 2 / 3 / 4 = Transpose.ROTATE_180 / ROTATE_90 / ROTATE_270.  dst stride = out_w.
__global__ __launch_bounds__(256) void rotate_bicubic_kernel(unsigned* __restrict__ px, long n, const int* __restrict__ desc,
                                                             const double* __restrict__ matrix) {
  const int* d = desc + blockIdx.y * 8;
  const int mode = d[7];
  if (mode == 0) return;
  const long src = d[0], sstride = d[1], dst = d[4];
  const int w = d[2], h = d[3], ow = d[5], oh = d[6];
  if (!window_ok(src, sstride, w, h, n) || !window_ok(dst, ow, ow, oh, n)) return;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)ow * oh) return;
  const int x = (int)(p % ow), y = (int)(p / ow);
  unsigned v = 0;
  if (mode == 2) {
    v = px[src + (long)(h - 1 - y) * sstride + (w - 1 - x)];
  } else if (mode == 3) {
    v = px[src + (long)x * sstride + (w - 1 - y)];
  } else if (mode == 4) {
    v = px[src + (long)(h - 1 - x) * sstride + y];
  } else {
    const double* m = matrix + blockIdx.y * 6;
    const double xo = x + 0.5, yo = y + 0.5;
    double xin = m[0] * xo + m[1] * yo + m[2];
    double yin = m[3] * xo + m[4] * yo + m[5];
    if (!(xin < 0.0 || xin >= w || yin < 0.0 || yin >= h)) {
      xin -= 0.5;
      yin -= 0.5;
      int ix = xin < 0.0 ? (int)floor(xin) : (int)xin;
      int iy = yin < 0.0 ? (int)floor(yin) : (int)yin;
      const double dx = xin - ix, dy = yin - iy;
      ix--;
      iy--;
      int xs[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) xs[k] = min(max(ix + k, 0), w - 1);
      unsigned q[4][4];                                                 // premultiplied taps (rows clamped: Geometry.c's
#pragma unroll                                                          // "v_k = v_{k-1}" outside the image is the same)
      for (int j = 0; j < 4; ++j) {
        const long row = src + (long)min(max(iy + j, 0), h - 1) * sstride;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[j][k] = premultiply(px[row + xs[k]]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double vr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          vr[j] = cubic((double)chan(q[j][0], c), (double)chan(q[j][1], c), (double)chan(q[j][2], c), (double)chan(q[j][3], c), dx);
        const double f = cubic(vr[0], vr[1], vr[2], vr[3], dy);
        const unsigned u = f <= 0.0 ? 0u : (f >= 255.0 ? 255u : (unsigned)(unsigned char)f);
        v |= u << (8 * c);
      }
      v = unpremultiply(v);
    }
  }
  px[dst + (long)y * ow + x] = v;
}

// ---- resize + normalise --------------------------------------------------------------------------------------------------

__device__ __forceinline__ double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

__device__ __forceinline__ unsigned clip8(int in) {
  if (in >= (1 << kPrec << 8)) return 255u;
  if (in <= 0) return 0u;
  return (unsigned)(in >> kPrec);
}

// output pixel xx of a resample of in_size pixels (first at `base`, `step` pixels apart) to out_size along one axis
__device__ unsigned resample_1d(const unsigned* __restrict__ px, long base, long step, int in_size, int out_size, int xx,
                                bool premul) {
  const double scale = (double)((float)in_size - 0.0f) / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const double center = 0.0 + (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += bicubic_filter((x + xmin - center + 0.5) * ss);
  int acc[4] = {1 << (kPrec - 1), 1 << (kPrec - 1), 1 << (kPrec - 1), 1 << (kPrec - 1)};
  for (int x = 0; x < xmax; ++x) {
    double k = bicubic_filter((x + xmin - center + 0.5) * ss);
    if (ww != 0.0) k /= ww;
    const int kf = k < 0 ? (int)(-0.5 + k * (1 << kPrec)) : (int)(0.5 + k * (1 << kPrec));
    unsigned p = px[base + (long)(x + xmin) * step];
    if (premul) p = premultiply(p);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += (int)chan(p, c) * kf;
  }
  return clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
}

// desc per sample: {src_off, src_stride, w, h, tmp_off, mode, -, -}; mode 0 = same size (a copy: no RGBa round trip),
// 1 = horizontal only, 2 = vertical only, 3 = horizontal then vertical, 4 = vertical then horizontal (taller than 100x wide).
// First launch (final == 0): the first pass of modes 3 / 4 into tmp (RGBa, dense: out_w x h or w x out_h).
// Second launch (final == 1): the last pass (or the copy), un-premultiply, ToTensor, (x - 0.5) / 0.5 into out[row0 + b].
__global__ __launch_bounds__(256) void resize_normalize_kernel(unsigned* __restrict__ px, long n, const int* __restrict__ desc,
                                                               float* __restrict__ out, int row0, int out_h, int out_w,
                                                               int final_pass) {
  const int b = blockIdx.y;
  const int* d = desc + b * 8;
  const long src = d[0], sstride = d[1], tmp = d[4];
  const int w = d[2], h = d[3], mode = d[5];
  if (!window_ok(src, sstride, w, h, n) || mode < 0 || mode > 4) return;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (!final_pass) {
    if (mode < 3) return;
    const int tw = mode == 3 ? out_w : w, th = mode == 3 ? h : out_h;
    if (!window_ok(tmp, tw, tw, th, n) || p >= (long)tw * th) return;
    const int x = (int)(p % tw), y = (int)(p / tw);
    px[tmp + p] = mode == 3 ? resample_1d(px, src + (long)y * sstride, 1, w, out_w, x, true)
                            : resample_1d(px, src + x, sstride, h, out_h, y, true);
    return;
  }
  if (p >= (long)out_h * out_w) return;
  const int x = (int)(p % out_w), y = (int)(p / out_w);
  unsigned v;
  if (mode == 0) {
    if (w != out_w || h != out_h) return;
    v = px[src + (long)y * sstride + x];
  } else if (mode == 1) {
    if (h != out_h) return;
    v = unpremultiply(resample_1d(px, src + (long)y * sstride, 1, w, out_w, x, true));
  } else if (mode == 2) {
    if (w != out_w) return;
    v = unpremultiply(resample_1d(px, src + x, sstride, h, out_h, y, true));
  } else if (mode == 3) {
    if (!window_ok(tmp, out_w, out_w, h, n)) return;
    v = unpremultiply(resample_1d(px, tmp + x, out_w, h, out_h, y, false));
  } else {
    if (!window_ok(tmp, w, w, out_h, n)) return;
    v = unpremultiply(resample_1d(px, tmp + (long)y * w, 1, w, out_w, x, false));
  }
  const long plane = (long)out_h * out_w;
  float* o = out + (long)(row0 + b) * 4 * plane + p;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c * plane] = __fdiv_rn(__fdiv_rn((float)chan(v, c), 255.0f) - 0.5f, 0.5f);
}

bool aug_args_ok(const void* px, int64_t n, const int* desc, int B, const char* name) {
  if (!px || !desc || B < 0 || n <= 0 || n >= (1LL << 31)) {
    mrn_set_error("%s: bad operands (pixels %p, n_pixels %lld, desc %p, B %d)", name, px, (long long)n, (const void*)desc, B);
    return false;
  }
  return true;
}

bool side_ok(int v) { return v >= 1 && v <= MRN_AUG_MAX_SIDE; }

}  // namespace

MRN_EXPORT int mrn_aug_gaussian_blur_rgba_u8(void* pixels, int64_t n_pixels, const int* desc, int B, int max_w, int max_h,
                                             void* stream) {
  if (!aug_args_ok(pixels, n_pixels, desc, B, "mrn_aug_gaussian_blur_rgba_u8")) return MRN_ERR_BAD_ARG;
  MRN_CHECK_ARG(side_ok(max_w) && side_ok(max_h), "mrn_aug_gaussian_blur_rgba_u8: sides %d x %d outside 1..%d", max_w, max_h,
                MRN_AUG_MAX_SIDE);
  if (B == 0) return MRN_OK;
  hipLaunchKernelGGL(box_blur3_kernel, dim3(max_h, B), dim3(64), 0, (hipStream_t)stream, (unsigned*)pixels, (long)n_pixels, desc, 0);
  MRN_LAUNCH_CHECK("box_blur3 (x)");
  hipLaunchKernelGGL(box_blur3_kernel, dim3(max_w, B), dim3(64), 0, (hipStream_t)stream, (unsigned*)pixels, (long)n_pixels, desc, 1);
  MRN_LAUNCH_CHECK("box_blur3 (y)");
  return MRN_OK;
}

MRN_EXPORT int mrn_aug_rotate_bicubic_rgba_u8(void* pixels, int64_t n_pixels, const int* desc, const void* matrix, int B,
                                              int max_out_w, int max_out_h, void* stream) {
  if (!aug_args_ok(pixels, n_pixels, desc, B, "mrn_aug_rotate_bicubic_rgba_u8")) return MRN_ERR_BAD_ARG;
  MRN_CHECK_ARG(matrix && side_ok(max_out_w) && side_ok(max_out_h),
                "mrn_aug_rotate_bicubic_rgba_u8: matrix %p, output sides %d x %d outside 1..%d", matrix, max_out_w, max_out_h,
                MRN_AUG_MAX_SIDE);
  if (B == 0) return MRN_OK;
  hipLaunchKernelGGL(rotate_bicubic_kernel, dim3(ceil_div((long)max_out_w * max_out_h, 256), B), dim3(256), 0,
                     (hipStream_t)stream, (unsigned*)pixels, (long)n_pixels, desc, (const double*)matrix);
  MRN_LAUNCH_CHECK("rotate_bicubic");
  return MRN_OK;
}

MRN_EXPORT int mrn_aug_resize_normalize_rgba_u8_f32(void* pixels, int64_t n_pixels, const int* desc, int B, int max_w, int max_h,
                                                    float* out, int row0, int out_h, int out_w, void* stream) {
  if (!aug_args_ok(pixels, n_pixels, desc, B, "mrn_aug_resize_normalize_rgba_u8_f32")) return MRN_ERR_BAD_ARG;
  MRN_CHECK_ARG(out && row0 >= 0 && side_ok(max_w) && side_ok(max_h) && side_ok(out_h) && side_ok(out_w),
                "mrn_aug_resize_normalize_rgba_u8_f32: out %p, row0 %d, sources up to %d x %d, output %d x %d (sides 1..%d)",
                (void*)out, row0, max_w, max_h, out_w, out_h, MRN_AUG_MAX_SIDE);
  if (B == 0) return MRN_OK;
  const long tmp_max = (long)max(out_w, max_w) * max(out_h, max_h);
  hipLaunchKernelGGL(resize_normalize_kernel, dim3(ceil_div(tmp_max, 256), B), dim3(256), 0, (hipStream_t)stream,
                     (unsigned*)pixels, (long)n_pixels, desc, out, row0, out_h, out_w, 0);
  MRN_LAUNCH_CHECK("resize_normalize (first pass)");
  hipLaunchKernelGGL(resize_normalize_kernel, dim3(ceil_div((long)out_h * out_w, 256), B), dim3(256), 0, (hipStream_t)stream,
                     (unsigned*)pixels, (long)n_pixels, desc, out, row0, out_h, out_w, 1);
  MRN_LAUNCH_CHECK("resize_normalize");
  return MRN_OK;
}
