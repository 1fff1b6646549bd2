// Producers of HL32 operands (hl32.hpp) for the x3 GEMM / convolution kernels: an fp32 activation split row by row, a convolution or
// Linear weight packed [Cout][Cin/32][tap] (one tensor, or every trained Linear weight of a step in one call), and the Winograd-domain
// weight transform G w of F(R,3).  Pure data movement apart from the power-of-two prescale and, in the last one, the transform itself.
#include "hl32.hpp"

namespace {

// fp32 [rows][C] -> HL32 [rows][C/32][hi 32 | lo 32]; one thread = 8 channels (32 B in, 2 x 16 B out)
__global__ __launch_bounds__(256) void split_hl32_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, long n8,
                                                         const float* __restrict__ scale) {
  const float sc = scale ? scale[0] : 1.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + i * 8) * sc, b = *reinterpret_cast<const f32x4*>(x + i * 8 + 4) * sc;
    f16v8 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      _Float16 hh, ll;
      split_f16(a[e], hh, ll);
      h[e] = hh; l[e] = ll;
      split_f16(b[e], hh, ll);
      h[4 + e] = hh; l[4 + e] = ll;
    }
    const long blk = i >> 2;            // 32-channel block index (4 threads per block)
    unsigned char* o = out + blk * 128 + (i & 3) * 16;
    *reinterpret_cast<f16v8*>(o) = h;
    *reinterpret_cast<f16v8*>(o + 64) = l;
  }
}

// w [Cout][taps][Cin] fp32 (x scale[0]) -> [Cout][Cin/32][taps][hi 32 | lo 32]; one thread = 8 channels
__global__ __launch_bounds__(256) void pack_weight_hl32_kernel(const float* __restrict__ w, unsigned char* __restrict__ out,
                                                               int Cout, int taps, int Cin, const float* __restrict__ scale) {
  const float sc = scale ? scale[0] : 1.f;
  const int Cb = Cin >> 5;
  const long n8 = (long)Cout * taps * (Cin >> 3);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const int c8 = (int)(i % (Cin >> 3));
    const long r = i / (Cin >> 3);
    const int tap = (int)(r % taps);
    const long o_ = r / taps;
    const float* src = w + (o_ * taps + tap) * Cin + c8 * 8;
    f16v8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      _Float16 hh, ll;
      split_f16(src[e] * sc, hh, ll);
      h[e] = hh; l[e] = ll;
    }
    const int cb = c8 >> 2;
    unsigned char* o = out + ((o_ * Cb + cb) * taps + tap) * 128 + (c8 & 3) * 16;
    *reinterpret_cast<f16v8*>(o) = h;
    *reinterpret_cast<f16v8*>(o + 64) = l;
  }
}

}  // namespace

// fp32 [rows][C] (C % 32 == 0) -> HL32 of scale[0] * x (scale: device float[2] from mrn_pow2_scale_f32, or NULL)
MRN_EXPORT int mrn_split_hl32_f32(const float* x, void* out, int64_t rows, int C, const float* scale, void* stream) {
  MRN_CHECK_ARG(x && out && C % 32 == 0, "mrn_split_hl32_f32: bad operands (C=%d)", C);
  const long n8 = rows * (C / 8);
  if (n8 == 0) return MRN_OK;
  long grid = (n8 + 255) / 256;
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(split_hl32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (unsigned char*)out, n8, scale);
  MRN_LAUNCH_CHECK("split_hl32");
  return MRN_OK;
}

// w [Cout][kh*kw][Cin] fp32 -> HL32 weight [Cout][Cin/32][kh*kw][128 B], multiplied by scale[0] (device) when given
MRN_EXPORT int mrn_pack_weight_hl32(const float* w_ohwi, void* out, int Cout, int taps, int Cin, const float* scale,
                                    void* stream) {
  MRN_CHECK_ARG(w_ohwi && out && Cin % 32 == 0, "mrn_pack_weight_hl32: bad operands (Cin=%d)", Cin);
  const long n8 = (long)Cout * taps * (Cin / 8);
  if (n8 == 0) return MRN_OK;
  long grid = (n8 + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(pack_weight_hl32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, w_ohwi,
                     (unsigned char*)out, Cout, taps, Cin, scale);
  MRN_LAUNCH_CHECK("pack_weight_hl32");
  return MRN_OK;
}

// Every trained Linear weight's operands for the coming step in ONE call (3 stream operations): the per-weight sequence max|W| ->
// power-of-two prescale -> HL32 pack [-> the same for W^T, the data gradient's operand] was 6 launches per layer, ~310 per SVTR loop-A
// step, issued by the host while the forward pass waited (a host-bound step: 1287 dispatches in 27 ms of host time).
// desc: n x 8 int64 on the device {W (fp32 [N][K]), out, scale (float[2]), N, K, transposed, first_tile, tiles_i}: the operand is
// L = W (O = N, I = K) or L = W^T (O = K, I = N), out [O][I/32][128 B] = HL32 of s * L, s = 2^floor(log2(target / max|W|)) exactly as
// mrn_pow2_scale_f32 + mrn_pack_weight_hl32 produce it.  amax: n zeroed-by-this-call words.  One block = one 32 x 32 tile of L.
namespace {
struct MultiPackDesc { const float* w; unsigned char* out; float* scale; long N, K, transposed, first_tile, tiles_i; };

__device__ __forceinline__ int multi_pack_find(const MultiPackDesc* __restrict__ d, int n, long tile) {
  int lo = 0, hi = n - 1;                       // last descriptor with first_tile <= tile
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void multi_pack_amax_kernel(const MultiPackDesc* __restrict__ desc, int n, unsigned* __restrict__ amax) {
  __shared__ float scratch[4];
  const int di = multi_pack_find(desc, n, blockIdx.x);
  const MultiPackDesc d = desc[di];
  const long tl = blockIdx.x - d.first_tile;
  const long to = tl / d.tiles_i, ti = tl - to * d.tiles_i;
  // the tile of L as a 32 x 32 region of the SOURCE matrix [N][K]: rows = o (plain) or i (transposed), columns the other index
  const long r0 = (d.transposed ? ti : to) * 32, c0 = (d.transposed ? to : ti) * 32;
  const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
  float m = 0.f;
  if (r0 + r < d.N && c0 + c4 < d.K) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(d.w + (r0 + r) * d.K + c0 + c4);
    m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
  }
  m = block_max<256>(m, scratch);
  if (threadIdx.x == 0 && !(m <= 0.f)) atomicMax(amax + di, __float_as_uint(m));      // NaN / inf pass through
}

__global__ __launch_bounds__(256) void multi_pack_kernel(const MultiPackDesc* __restrict__ desc, int n, const unsigned* __restrict__ amax,
                                                         float target) {
  __shared__ float tile[32][33];
  const int di = multi_pack_find(desc, n, blockIdx.x);
  const MultiPackDesc d = desc[di];
  const long tl = blockIdx.x - d.first_tile;
  const long to = tl / d.tiles_i, ti = tl - to * d.tiles_i;
  const float mm = __uint_as_float(amax[di]);
  float sc = 1.f;
  if (mm > 0.f && isfinite(mm)) sc = exp2f(floorf(log2f(target / mm)));
  if (tl == 0 && threadIdx.x == 0) {
    d.scale[0] = sc;
    d.scale[1] = 1.f / sc;
  }
  const long O = d.transposed ? d.K : d.N, Cb = (d.transposed ? d.N : d.K) >> 5;
  const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!d.transposed) {
    if (to * 32 + r < O) v = *reinterpret_cast<const f32x4*>(d.w + (to * 32 + r) * d.K + ti * 32 + c4);
    tile[r][c4 + 0] = v[0] * sc; tile[r][c4 + 1] = v[1] * sc; tile[r][c4 + 2] = v[2] * sc; tile[r][c4 + 3] = v[3] * sc;
  } else {        // source row = i, source columns = o: lands transposed
    if (to * 32 + c4 < O) v = *reinterpret_cast<const f32x4*>(d.w + (ti * 32 + r) * d.K + to * 32 + c4);
    tile[c4 + 0][r] = v[0] * sc; tile[c4 + 1][r] = v[1] * sc; tile[c4 + 2][r] = v[2] * sc; tile[c4 + 3][r] = v[3] * sc;
  }
  __syncthreads();
  const int o = threadIdx.x >> 3, seg = threadIdx.x & 7;          // row o of the tile, elements seg*4 .. +3 of its 32-channel line
  if (to * 32 + o < O)
    split_hl4([&](int e) { return tile[o][seg * 4 + e]; }).store(d.out + ((to * 32 + o) * Cb + ti) * 128 + seg * 8);
}
}  // namespace

MRN_EXPORT int mrn_multi_pack_linear_hl32(const void* desc, int n, int64_t tiles, void* amax, float target, void* stream) {
  MRN_CHECK_ARG(desc && amax && n > 0 && tiles > 0 && tiles < (1L << 31) && target > 0.f, "mrn_multi_pack_linear_hl32: bad operands (n=%d)", n);
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(amax, 0, sizeof(unsigned) * (size_t)n, st);
  MRN_CHECK_ARG(e == hipSuccess, "mrn_multi_pack_linear_hl32: memset failed (%s)", hipGetErrorString(e));
  hipLaunchKernelGGL(multi_pack_amax_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const MultiPackDesc*)desc, n, (unsigned*)amax);
  hipLaunchKernelGGL(multi_pack_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const MultiPackDesc*)desc, n, (const unsigned*)amax, target);
  MRN_LAUNCH_CHECK("multi_pack_linear_hl32");
  return MRN_OK;
}

// ---- Winograd F(R,3) along W: the weight transform (the convolution is conv_x3.hip WINO / conv_wino.hip) --------------------------
namespace {

// rows of G (F(4,3): interpolation points 0, +-1, +-2, inf; F(2,3): 0, +-1, inf) times the power-of-two row scale whose inverse
// WinoAT folds into A^T, so that every transformed row sum of |.| stays <= 1.5 and ONE per-tensor prescale serves all components
__device__ __forceinline__ double wino_g(int R, int m, int kx) {
  if (R == 2) {
    const double g[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
    return g[m][kx];
  }
  const double g[6][3] = {{1, 0, 0},
                          {-1. / 3, -1. / 3, -1. / 3},
                          {-1. / 3, 1. / 3, -1. / 3},
                          {1. / 12, 1. / 6, 1. / 3},
                          {1. / 12, -1. / 6, 1. / 3},
                          {0, 0, 1}};
  return g[m][kx];
}

// w [Cout][3][3][Cin] fp32 (OHWI) -> U [Cout][NC][Cin/32][3 (ky)][hi 32 | lo 32] with U_m = scale * sum_kx G[m][kx] * w[.][ky][kx][.],
// the sum in double, split to hi + lo from the double; one thread = 8 channels of one (cout, component, ky)
__global__ __launch_bounds__(256) void pack_weight_wino_hl32_kernel(const float* __restrict__ w, unsigned char* __restrict__ out,
                                                                    int Cout, int Cin, int R, const float* __restrict__ scale, int dense) {
  const double sc = scale ? (double)scale[0] : 1.0;
  const int Cb = Cin >> 5, NC = R + 2;
  const long n8 = (long)Cout * NC * 3 * (Cin >> 3);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const int c8 = (int)(i % (Cin >> 3));
    long r = i / (Cin >> 3);
    const int ky = (int)(r % 3);
    r /= 3;
    const int m = (int)(r % NC);
    const long o_ = r / NC;
    const float* src = w + ((o_ * 3 + ky) * 3) * Cin + c8 * 8;       // [kx][Cin]
    f16v8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      double u = 0.0;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) u += wino_g(R, m, kx) * (double)src[kx * Cin + e];
      u *= sc;
      const _Float16 hh = (_Float16)u;
      const _Float16 ll = (_Float16)(u - (double)hh);
      h[e] = hh; l[e] = ll;
    }
    if (dense) {           // plain fp16 (dense == 2: bfloat16), 64 channels per line: [Cout][NC][Cin/64][3][128 B]
      unsigned char* dst = out + (((o_ * NC + m) * (Cin >> 6) + (c8 >> 3)) * 3 + ky) * 128 + (c8 & 7) * 16;
      if (dense == 2) {
        typedef unsigned short u16v8 __attribute__((ext_vector_type(8)));
        u16v8 b;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          double u = 0.0;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) u += wino_g(R, m, kx) * (double)src[kx * Cin + e];
          const unsigned bits = __float_as_uint((float)(u * sc));
          b[e] = (unsigned short)((bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16);
        }
        *reinterpret_cast<u16v8*>(dst) = b;
      } else {
        *reinterpret_cast<f16v8*>(dst) = h;
      }
      continue;
    }
    const int cb = c8 >> 2;
    unsigned char* o = out + (((o_ * NC + m) * Cb + cb) * 3 + ky) * 128 + (c8 & 3) * 16;
    *reinterpret_cast<f16v8*>(o) = h;
    *reinterpret_cast<f16v8*>(o + 64) = l;
  }
}

}  // namespace

// w [Cout][3][3][Cin] fp32 -> Winograd-domain HL32 weight [Cout][R+2][Cin/32][3][128 B] of scale[0] * (G w) (R = 2 or 4)
MRN_EXPORT int mrn_pack_weight_wino_hl32(const float* w_ohwi, void* out, int Cout, int Cin, int R, const float* scale, void* stream) {
  MRN_CHECK_ARG(w_ohwi && out && Cin % 32 == 0 && (R == 2 || R == 4), "mrn_pack_weight_wino_hl32: bad operands (Cin=%d R=%d)", Cin, R);
  const long n8 = (long)Cout * (R + 2) * 3 * (Cin / 8);
  if (n8 == 0) return MRN_OK;
  long grid = (n8 + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(pack_weight_wino_hl32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, w_ohwi, (unsigned char*)out,
                     Cout, Cin, R, scale, 0);
  MRN_LAUNCH_CHECK("pack_weight_wino_hl32");
  return MRN_OK;
}

// the same transform as PLAIN fp16 for the reduced-precision mode: w [Cout][3][3][Cin] fp32 -> [Cout][6][Cin/64][3][128 B] of
// scale[0] * (G w), F(4,3), 64 channels per line (mrn_conv2d_x3_wino_d16's weight operand); Cin % 64 == 0
MRN_EXPORT int mrn_pack_weight_wino_d16(const float* w_ohwi, void* out, int Cout, int Cin, const float* scale, int bf16, void* stream) {
  MRN_CHECK_ARG(w_ohwi && out && Cin % 64 == 0, "mrn_pack_weight_wino_d16: bad operands (Cin=%d)", Cin);
  const long n8 = (long)Cout * 6 * 3 * (Cin / 8);
  if (n8 == 0) return MRN_OK;
  long grid = (n8 + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(pack_weight_wino_hl32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, w_ohwi, (unsigned char*)out,
                     Cout, Cin, 4, scale, bf16 ? 2 : 1);
  MRN_LAUNCH_CHECK("pack_weight_wino_d16");
  return MRN_OK;
}
