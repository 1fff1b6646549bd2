// Operand passes of the weight gradients on the x3 GEMM kernel (conv_x3.hip): dW reduces over ROWS (pixels, tokens), so both operands
// are written TRANSPOSED as HL32 lines (hl32.hpp) along the reduction axis -- the plain transposed split (optionally with the column
// sums that are the bias gradient), the transposed im2col, the image-row-major transposes whose kernel-row offset is a whole number of
// lines, their Winograd-domain forms, and the final reduction of the Winograd-domain partial sums.
#include "hl32.hpp"

namespace {

// Transposed split for weight-gradient GEMMs (dW = dy^T x reduces over ROWS): fp32 x[rows][C] -> `splits` HL32 matrices
// out[s][c][rps/32][hi 32 | lo 32] with rps = rows / splits, element (c, r) = scale * x[s*rps + r][c].  One block moves a
// 32-row x 32-column tile through LDS: coalesced 128-byte row reads, one 128-byte HL32 line per column written.
__global__ __launch_bounds__(256) void split_hl32_t_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int C,
                                                           long rows, long rps32, long tiles_c, long ntiles,
                                                           const float* __restrict__ scale) {
  __shared__ float tile[32][33];
  const float sc = scale ? scale[0] : 1.f;
  const int t = threadIdx.x;
  for (long id = blockIdx.x; id < ntiles; id += gridDim.x) {
    const long rb = id / tiles_c;                 // 32-row block (global)
    const int c0 = (int)(id - rb * tiles_c) * 32;
    {
      const int r = t >> 3, c4 = (t & 7) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (c0 + c4 < C && rb * 32 + r < rows) v = *reinterpret_cast<const f32x4*>(x + (rb * 32 + r) * C + c0 + c4);
      tile[r][c4 + 0] = v[0] * sc; tile[r][c4 + 1] = v[1] * sc; tile[r][c4 + 2] = v[2] * sc; tile[r][c4 + 3] = v[3] * sc;
    }
    __syncthreads();
    {
      const int c = t >> 3, seg = t & 7;          // column c, rows seg*4 .. +3
      if (c0 + c < C) {
        const long s_ = rb / rps32, rl = rb - s_ * rps32;
        unsigned char* o = out + ((s_ * C + c0 + c) * rps32 + rl) * 128 + seg * 8;
        f16v4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          _Float16 hh, ll;
          split_f16(tile[seg * 4 + e][c], hh, ll);
          h[e] = hh; l[e] = ll;
        }
        *reinterpret_cast<f16v4*>(o) = h;
        *reinterpret_cast<f16v4*>(o + 64) = l;
      }
    }
    __syncthreads();
  }
}

// The same transposed split WITH the column sums of x (the bias gradient of a Linear layer is the column sum of the very dy this pass
// transposes for the weight gradient: two more passes over dy, 100 launches and 2.5 ms of an SVTR loop-A step's weight-gradient stream).
// grid (column tiles, chunks): a block keeps ONE 32-column tile and walks the 32-row blocks of its chunk four at a time (four 16-byte
// loads in flight per lane); its column sums (of the scaled values: the scale is a power of two, so 1/s * sum(s x) == sum(x) in the
// same order) go to partial[chunk][C] (one chunk: straight into colsum); a column-sum pass over those <= 256 rows finishes.  [Measured:
// the finish inside this kernel -- last block to arrive per column tile, __threadfence() + ticket -- made it 8-15 x slower, 39 -> 324 us
// at 131072 x 256: every block's agent-scope release writes back an L2 that 2048 blocks keep dirtying with 134 MB of operand lines.]
__global__ __launch_bounds__(256) void split_hl32_t_colsum_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int C,
                                                                  long rows, long rps32, long rblocks, long rb_per_chunk,
                                                                  const float* __restrict__ scale, float* __restrict__ partial,
                                                                  float* __restrict__ colsum, int accumulate) {
  __shared__ float tile[4][32][33];
  const float sc = scale ? scale[0] : 1.f, inv = scale ? scale[1] : 1.f;
  const int t = threadIdx.x;
  const int c0 = blockIdx.x * 32, chunk = blockIdx.y, nchunks = gridDim.y;
  const long rb0 = chunk * rb_per_chunk, rb1 = min(rblocks, rb0 + rb_per_chunk);
  const int r = t >> 3, c4 = (t & 7) * 4;          // load role: row r of a row block, columns c4 .. +3
  const int c = t >> 3, seg = t & 7;               // store role: column c, rows seg*4 .. +3
  float acc = 0.f;
  for (long rb = rb0; rb < rb1; rb += 4) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      const long row = (rb + u) * 32 + r;
      if (rb + u < rb1 && c0 + c4 < C && row < rows) v[u] = *reinterpret_cast<const f32x4*>(x + row * C + c0 + c4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      tile[u][r][c4 + 0] = v[u][0] * sc; tile[u][r][c4 + 1] = v[u][1] * sc;
      tile[u][r][c4 + 2] = v[u][2] * sc; tile[u][r][c4 + 3] = v[u][3] * sc;
    }
    __syncthreads();
    if (c0 + c < C) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (rb + u >= rb1) break;
        const long s_ = (rb + u) / rps32, rl = (rb + u) - s_ * rps32;
        unsigned char* o = out + ((s_ * C + c0 + c) * rps32 + rl) * 128 + seg * 8;
        f16v4 h, l;
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float f = tile[u][seg * 4 + e][c];
          _Float16 hh, ll;
          split_f16(f, hh, ll);
          h[e] = hh; l[e] = ll;
          a += f;
        }
        acc += a;
        *reinterpret_cast<f16v4*>(o) = h;
        *reinterpret_cast<f16v4*>(o + 64) = l;
      }
    }
    __syncthreads();
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  acc += __shfl_xor(acc, 4);
  acc *= inv;
  if (nchunks == 1) {
    if (seg == 0 && c0 + c < C) colsum[c0 + c] = accumulate ? colsum[c0 + c] + acc : acc;
    return;
  }
  if (seg == 0 && c0 + c < C) partial[(long)chunk * C + c0 + c] = acc;
}

struct Im2colT {
  const float* x; unsigned char* out; const float* scale;
  int B, H, W, C, Ho, Wo, kw, taps, sh, sw, ph, pw;
  long P, rps32, tiles_c, ntiles;
};

// one block = (32 output pixels) x (32 channels) of ONE tap; the tap index runs fastest over the grid so the nine taps of a
// pixel block re-read the same input lines from L2
__global__ __launch_bounds__(256) void im2col_t_hl32_kernel(const Im2colT p) {
  __shared__ float tile[32][33];
  const float sc = p.scale ? p.scale[0] : 1.f;
  const int t = threadIdx.x;
  for (long id = blockIdx.x; id < p.ntiles; id += gridDim.x) {
    const int tap = (int)(id % p.taps);
    const long id2 = id / p.taps;
    const long rb = id2 / p.tiles_c;                 // 32-pixel block (global over the padded pixel axis)
    const int c0 = (int)(id2 - rb * p.tiles_c) * 32;
    const int ky = tap / p.kw, kx = tap - ky * p.kw;
    {
      const int r = t >> 3, c4 = (t & 7) * 4;
      const long pix = rb * 32 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pix < p.P && c0 + c4 < p.C) {
        const int hw = p.Ho * p.Wo;
        const int b = (int)(pix / hw);
        const int rem = (int)(pix - (long)b * hw);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        const int iy = oy * p.sh - p.ph + ky, ix = ox * p.sw - p.pw + kx;
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
          v = *reinterpret_cast<const f32x4*>(p.x + (((long)b * p.H + iy) * p.W + ix) * p.C + c0 + c4);
      }
      tile[r][c4 + 0] = v[0] * sc; tile[r][c4 + 1] = v[1] * sc; tile[r][c4 + 2] = v[2] * sc; tile[r][c4 + 3] = v[3] * sc;
    }
    __syncthreads();
    {
      const int c = t >> 3, seg = t & 7;
      if (c0 + c < p.C) {
        const long s_ = rb / p.rps32, rl = rb - s_ * p.rps32;
        unsigned char* o = p.out + ((((s_ * p.taps + tap) * p.C) + c0 + c) * p.rps32 + rl) * 128 + seg * 8;
        f16v4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          _Float16 hh, ll;
          split_f16(tile[seg * 4 + e][c], hh, ll);
          h[e] = hh; l[e] = ll;
        }
        *reinterpret_cast<f16v4*>(o) = h;
        *reinterpret_cast<f16v4*>(o + 64) = l;
      }
    }
    __syncthreads();
  }
}

// Transposed split in IMAGE-ROW-MAJOR pixel order, optionally shifted along x: NHWC fp32 x[b][y][xx][c] -> out[c][k / 32][hi 32 | lo 32]
// with k = (y * B + b) * W + xx and element (c, k) = scale * x[b][y][xx + shift][c] (0 outside the row; k >= P: 0).  The operand layout
// of the convolution weight gradient without an im2col (mrn_gemm_x3_windows_hl32): in this order a kernel-row offset ky - 1 is
// a whole number of lines (B * W pixels) and only the THREE horizontal shifts need their own copy.  One block = 32 pixels x 32 channels.
__global__ __launch_bounds__(256) void transpose_oy_hl32_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int B,
                                                                int H, int W, int C, int shift, long P, long lines, long tiles_c,
                                                                long ntiles, const float* __restrict__ scale) {
  __shared__ float tile[32][33];
  const float sc = scale ? scale[0] : 1.f;
  const int t = threadIdx.x;
  for (long id = blockIdx.x; id < ntiles; id += gridDim.x) {
    const long kb = id / tiles_c;                 // 32-pixel block along k
    const int c0 = (int)(id - kb * tiles_c) * 32;
    {
      const int r = t >> 3, c4 = (t & 7) * 4;
      const long k = kb * 32 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k < P && c0 + c4 < C) {
        const long row = k / W;                   // = y * B + b
        const int xx = (int)(k - row * W) + shift;
        const int y = (int)(row / B), b = (int)(row - (long)y * B);
        if ((unsigned)xx < (unsigned)W) v = *reinterpret_cast<const f32x4*>(x + (((long)b * H + y) * W + xx) * C + c0 + c4);
      }
      tile[r][c4 + 0] = v[0] * sc; tile[r][c4 + 1] = v[1] * sc; tile[r][c4 + 2] = v[2] * sc; tile[r][c4 + 3] = v[3] * sc;
    }
    __syncthreads();
    {
      const int c = t >> 3, seg = t & 7;          // column c, pixels seg*4 .. +3
      if (c0 + c < C) {
        unsigned char* o = out + ((long)(c0 + c) * lines + kb) * 128 + seg * 8;
        f16v4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          _Float16 hh, ll;
          split_f16(tile[seg * 4 + e][c], hh, ll);
          h[e] = hh; l[e] = ll;
        }
        *reinterpret_cast<f16v4*>(o) = h;
        *reinterpret_cast<f16v4*>(o + 64) = l;
      }
    }
    __syncthreads();
  }
}

// The three horizontal shifts (-1, 0, +1) of transpose_oy_hl32_kernel from ONE read of the activation: out[s][c][k / 32][...] for
// s = 0, 1, 2 (copy stride `copy_bytes`).  A block stages pixels k0 - 1 .. k0 + 32 (34 rows) x 32 channels.
__global__ __launch_bounds__(256) void transpose_oy3_hl32_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int B,
                                                                 int H, int W, int C, long P, long lines, long tiles_c, long ntiles,
                                                                 long copy_bytes, const float* __restrict__ scale) {
  __shared__ float tile[34][33];
  __shared__ int xpos[34];
  const float sc = scale ? scale[0] : 1.f;
  const int t = threadIdx.x;
  for (long id = blockIdx.x; id < ntiles; id += gridDim.x) {
    const long kb = id / tiles_c;
    const int c0 = (int)(id - kb * tiles_c) * 32;
    for (int i = t; i < 34 * 8; i += 256) {
      const int r = i >> 3, c4 = (i & 7) * 4;
      const long k = kb * 32 + r - 1;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      int xx = -1000;
      if (k >= 0 && k < P) {
        const long row = k / W;
        xx = (int)(k - row * W);
        const int y = (int)(row / B), b = (int)(row - (long)y * B);
        if (c0 + c4 < C) v = *reinterpret_cast<const f32x4*>(x + (((long)b * H + y) * W + xx) * C + c0 + c4);
      }
      if (c4 == 0) xpos[r] = xx;
      tile[r][c4 + 0] = v[0] * sc; tile[r][c4 + 1] = v[1] * sc; tile[r][c4 + 2] = v[2] * sc; tile[r][c4 + 3] = v[3] * sc;
    }
    __syncthreads();
    {
      const int c = t >> 3, seg = t & 7;
      if (c0 + c < C) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {              // shift = s - 1: destination pixel j takes source pixel j + shift of the SAME image row
          f16v4 h, l;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int j = seg * 4 + e;             // destination row of the tile is j + 1, its source j + s
            const int xd = xpos[j + 1];
            const bool ok = xd >= 0 && (unsigned)(xd + s - 1) < (unsigned)W;
            _Float16 hh, ll;
            split_f16(ok ? tile[j + s][c] : 0.f, hh, ll);
            h[e] = hh; l[e] = ll;
          }
          unsigned char* o = out + s * copy_bytes + ((long)(c0 + c) * lines + kb) * 128 + seg * 8;
          *reinterpret_cast<f16v4*>(o) = h;
          *reinterpret_cast<f16v4*>(o + 64) = l;
        }
      }
    }
    __syncthreads();
  }
}

// Transposed operands of the Winograd-domain weight gradient (mrn_conv_wgrad_wino...): NHWC fp32 t[b][y][xx][c] -> out[m][c][kq / 32][hi 32 | lo 32]
// over GROUPS of 4 columns in image-row-major order kq = (y * B + b) * Wq + q (Wq = ceil(W / 4)), six components m per group:
//   MODE 0 (the layer input x):       V_m  = sum_j B^T[m][j] * x[.., 4q - 1 + j]   (j = 0..5, zero outside the row)
//   MODE 1 (the output gradient dy):  dY_m = sum_r A^T[r][m] * dy[.., 4q + r]      (r = 0..3, zero beyond W)
// times scale[0].  With these, dU_m[ky] = sum over groups of dY_m (x) V_m (row-shifted by ky - 1) and dW[ky][kx] = sum_m G[m][kx] dU_m[ky]:
// 18 K-windows of length P/4 instead of 9 of length P -- half the matrix work -- and ONE 1.5x copy of x^T instead of three shifted copies.
// One block = 32 groups x 32 channels through LDS.
template <int MODE>
__global__ __launch_bounds__(256) void transpose_oy_wino_hl32_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int B, int H,
                                                                     int W, int Wq, int C, long Pq, long lines, long tiles_c, long ntiles,
                                                                     const float* __restrict__ scale) {
  constexpr int NCOL = MODE == 0 ? 6 : 4;
  __shared__ float tile[32 * NCOL][33];
  const float sc = scale ? scale[0] : 1.f;
  const int t = threadIdx.x;
  for (long id = blockIdx.x; id < ntiles; id += gridDim.x) {
    const long kb = id / tiles_c;
    const int c0 = (int)(id - kb * tiles_c) * 32;
    for (int i = t; i < 32 * NCOL * 8; i += 256) {
      const int rr = i >> 3, c4 = (i & 7) * 4;          // rr = group-in-block * NCOL + column
      const int gq = rr / NCOL, j = rr - gq * NCOL;
      const long kq = kb * 32 + gq;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (kq < Pq && c0 + c4 < C) {
        const long row = kq / Wq;                        // = y * B + b
        const int q = (int)(kq - row * Wq);
        const int xx = 4 * q + j - (MODE == 0 ? 1 : 0);
        const int y = (int)(row / B), b = (int)(row - (long)y * B);
        if ((unsigned)xx < (unsigned)W) v = *reinterpret_cast<const f32x4*>(x + (((long)b * H + y) * W + xx) * C + c0 + c4);
      }
      tile[rr][c4 + 0] = v[0]; tile[rr][c4 + 1] = v[1]; tile[rr][c4 + 2] = v[2]; tile[rr][c4 + 3] = v[3];
    }
    __syncthreads();
    {
      const int c = t >> 3, seg = t & 7;                 // channel c, groups seg*4 .. +3 of the block
      if (c0 + c < C) {
        f16v4 h[6], l[6];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int gq = seg * 4 + e;
          float m_[6];
          if constexpr (MODE == 0) {
            const float d0 = tile[gq * 6 + 0][c], d1 = tile[gq * 6 + 1][c], d2 = tile[gq * 6 + 2][c], d3 = tile[gq * 6 + 3][c],
                        d4 = tile[gq * 6 + 4][c], d5 = tile[gq * 6 + 5][c];
            m_[0] = 4.f * d0 - 5.f * d2 + d4;
            m_[1] = -4.f * (d1 + d2) + d3 + d4;
            m_[2] = 4.f * (d1 - d2) - d3 + d4;
            m_[3] = 2.f * (d3 - d1) - d2 + d4;
            m_[4] = 2.f * (d1 - d3) - d2 + d4;
            m_[5] = 4.f * d1 - 5.f * d3 + d5;
          } else {
            const float y0 = tile[gq * 4 + 0][c], y1 = tile[gq * 4 + 1][c], y2 = tile[gq * 4 + 2][c], y3 = tile[gq * 4 + 3][c];
            m_[0] = y0;                                  // columns of A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
            m_[1] = y0 + y1 + y2 + y3;
            m_[2] = y0 - y1 + y2 - y3;
            m_[3] = y0 + 2.f * y1 + 4.f * y2 + 8.f * y3;
            m_[4] = y0 - 2.f * y1 + 4.f * y2 - 8.f * y3;
            m_[5] = y3;
          }
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            _Float16 hh, ll;
            split_f16(m_[k] * sc, hh, ll);
            h[k][e] = hh; l[k][e] = ll;
          }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          unsigned char* o = out + (((long)k * C + c0 + c) * lines + kb) * 128 + seg * 8;
          *reinterpret_cast<f16v4*>(o) = h[k];
          *reinterpret_cast<f16v4*>(o + 64) = l[k];
        }
      }
    }
    __syncthreads();
  }
}

// dW [Cout][3][3][Cin] = sum over split-K chunks s and components m of G[m][kx] * part[s][m * 3 + ky][co][ci]  (G of F(4,3), unfolded);
// one lane = 4 consecutive input channels (Cin % 4 == 0) of ONE kernel row (blockIdx.y = ky: the three rows are independent, and a
// 512 x 512 layer has only 65536 channel quads -- one wave per SIMD without the split): 6 accumulators, two split-K slabs in flight
// OIHW_ACC: dW is ADDED into the parameter's own [Cout][Cin][3][3] gradient (the flat-gradient slice)
template <bool OIHW_ACC>
__global__ __launch_bounds__(256) void wino_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ dw, int S, long CC4, int Cin4) {
  const float G[6][3] = {{0.25f, 0.f, 0.f}, {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                         {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
  const f32x4* p4 = reinterpret_cast<const f32x4*>(part);
  const int ky = blockIdx.y;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < CC4; i += (long)gridDim.x * 256) {      // i = (co * Cin + ci) / 4
    const long co = i / Cin4;
    const int c4 = (int)(i - co * Cin4);
    f32x4 u[6], w[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) u[m] = w[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    int s_ = 0;
    for (; s_ + 1 < S; s_ += 2) {
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        u[m] += p4[((long)s_ * 18 + m * 3 + ky) * CC4 + i];
        w[m] += p4[((long)(s_ + 1) * 18 + m * 3 + ky) * CC4 + i];
      }
    }
    if (s_ < S) {
#pragma unroll
      for (int m = 0; m < 6; ++m) u[m] += p4[((long)s_ * 18 + m * 3 + ky) * CC4 + i];
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) u[m] += w[m];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < 6; ++m) v += G[m][kx] * u[m];
      if constexpr (OIHW_ACC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) dw[((co * Cin4 + c4) * 4 + j) * 9 + ky * 3 + kx] += v[j];
      } else {
        reinterpret_cast<f32x4*>(dw)[((co * 3 + ky) * 3 + kx) * Cin4 + c4] = v;
      }
    }
  }
}

}  // namespace

// fp32 x[rows][C] (C % 4 == 0) -> `splits` transposed HL32 matrices [splits][C][rows_padded/splits/32][128 B] of scale[0] * x
// (rows_padded % (32 * splits) == 0, rows beyond `rows` are zero): the operand layout of a weight-gradient GEMM that
// reduces over rows, split-K = groups.
MRN_EXPORT int mrn_split_hl32_t_f32(const float* x, void* out, int64_t rows, int64_t rows_padded, int C, int splits,
                                    const float* scale, void* stream) {
  MRN_CHECK_ARG(x && out && splits >= 1 && C % 4 == 0 && rows_padded >= rows && rows_padded % (32L * splits) == 0,
                "mrn_split_hl32_t_f32: bad operands (rows=%ld padded=%ld C=%d splits=%d)", (long)rows, (long)rows_padded, C, splits);
  if (rows_padded == 0 || C == 0) return MRN_OK;
  const long tiles_c = (C + 31) / 32, ntiles = rows_padded / 32 * tiles_c;
  long grid = ntiles > 65536 ? 65536 : ntiles;
  hipLaunchKernelGGL(split_hl32_t_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (unsigned char*)out, C,
                     (long)rows, (long)(rows_padded / splits / 32), tiles_c, ntiles, scale);
  MRN_LAUNCH_CHECK("split_hl32_t");
  return MRN_OK;
}

// mrn_split_hl32_t_f32 that also leaves colsum[c] (+)= sum over rows of x[r][c].  partial: mrn_split_hl32_t_colsum_chunks(rows_padded, C) * C
// floats of scratch (unused with one chunk).
extern "C" int mrn_colsum_f32(const float* in, int64_t ld, float* out, float* workspace, int64_t rows, int C, int accumulate, void* stream);

MRN_EXPORT int64_t mrn_split_hl32_t_colsum_chunks(int64_t rows_padded, int C) {
  const long rblocks = rows_padded / 32, tiles_c = (C + 31) / 32;
  long want = 4096 / (tiles_c < 1 ? 1 : tiles_c);
  want = want < 1 ? 1 : (want > 256 ? 256 : want);
  long per = (rblocks + want - 1) / want;
  per = (per + 3) / 4 * 4;                             // (four row blocks per iteration)
  const long chunks = per > 0 ? (rblocks + per - 1) / per : 1;
  return chunks < 1 ? 1 : chunks;
}

MRN_EXPORT int mrn_split_hl32_t_colsum_f32(const float* x, void* out, int64_t rows, int64_t rows_padded, int C, int splits,
                                           const float* scale, float* colsum, int accumulate, float* partial, void* stream) {
  MRN_CHECK_ARG(x && out && colsum && splits >= 1 && C % 4 == 0 && rows_padded >= rows && rows_padded % (32L * splits) == 0,
                "mrn_split_hl32_t_colsum_f32: bad operands (rows=%ld padded=%ld C=%d splits=%d)", (long)rows, (long)rows_padded, C, splits);
  if (rows_padded == 0 || C == 0) return MRN_OK;
  const long rblocks = rows_padded / 32, tiles_c = (C + 31) / 32;
  const long chunks = mrn_split_hl32_t_colsum_chunks(rows_padded, C);
  const long per = (((rblocks + chunks - 1) / chunks) + 3) / 4 * 4;
  MRN_CHECK_ARG(chunks == 1 || partial, "mrn_split_hl32_t_colsum_f32: %ld chunks need the scratch rows", chunks);
  MRN_CHECK_ARG(per * chunks >= rblocks && chunks <= 512, "mrn_split_hl32_t_colsum_f32: bad chunking (%ld x %ld < %ld)", per, chunks, rblocks);
  hipLaunchKernelGGL(split_hl32_t_colsum_kernel, dim3((unsigned)tiles_c, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, x,
                     (unsigned char*)out, C, (long)rows, (long)(rows_padded / splits / 32), rblocks, per, scale, partial, colsum, accumulate);
  MRN_LAUNCH_CHECK("split_hl32_t_colsum");
  if (chunks > 1) return mrn_colsum_f32(partial, C, colsum, nullptr, chunks, C, accumulate, stream);     // (<= 512 rows: one pass)
  return MRN_OK;
}

// Transposed im2col for the convolution weight gradient dW[co][tap][ci] = sum_p dy[p][co] * x[pixel(p, tap)][ci]:
//   out[s][tap][ci][rps/32][hi 32 | lo 32], element (tap, ci, p) = scale * x[b][oy*sh + ky - ph][ox*sw + kx - pw][ci]
// (zero outside the image / beyond P = B*Ho*Wo), p = s*rps + r the output pixel.  x NHWC [B][H][W][C], C % 4 == 0.
MRN_EXPORT int mrn_im2col_t_hl32_f32(const float* x, void* out, int B, int H, int W, int C, int kh, int kw, int sh, int sw,
                                     int ph, int pw, int64_t rows_padded, int splits, const float* scale, void* stream) {
  MRN_CHECK_ARG(x && out && splits >= 1 && C % 4 == 0 && rows_padded % (32L * splits) == 0, "mrn_im2col_t_hl32_f32: bad operands");
  const int Ho = (H + 2 * ph - kh) / sh + 1, Wo = (W + 2 * pw - kw) / sw + 1;
  MRN_CHECK_ARG(Ho > 0 && Wo > 0 && rows_padded >= (long)B * Ho * Wo, "mrn_im2col_t_hl32_f32: bad geometry");
  if (rows_padded == 0 || C == 0) return MRN_OK;
  Im2colT p;
  p.x = x; p.out = (unsigned char*)out; p.scale = scale;
  p.B = B; p.H = H; p.W = W; p.C = C; p.Ho = Ho; p.Wo = Wo; p.kw = kw; p.taps = kh * kw;
  p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw;
  p.P = (long)B * Ho * Wo; p.rps32 = rows_padded / splits / 32; p.tiles_c = (C + 31) / 32;
  p.ntiles = rows_padded / 32 * p.tiles_c * p.taps;
  long grid = p.ntiles > 262144 ? 262144 : p.ntiles;
  hipLaunchKernelGGL(im2col_t_hl32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p);
  MRN_LAUNCH_CHECK("im2col_t_hl32");
  return MRN_OK;
}

// x NHWC [B][H][W][C] fp32 -> transposed HL32 matrix [C][lines][128 B] (lines = ceil(B*H*W / 32)) in image-row-major pixel order
// k = (y*B + b)*W + xx, shifted by shift_x pixels along x with zero fill: see transpose_oy_hl32_kernel
MRN_EXPORT int mrn_transpose_oy_hl32_f32(const float* x, void* out, int B, int H, int W, int C, int shift_x, const float* scale,
                                         void* stream) {
  MRN_CHECK_ARG(x && out && C % 4 == 0 && B > 0 && H > 0 && W > 0, "mrn_transpose_oy_hl32_f32: bad operands");
  const long P = (long)B * H * W, lines = (P + 31) / 32, tiles_c = (C + 31) / 32, ntiles = lines * tiles_c;
  long grid = ntiles > 65536 ? 65536 : ntiles;
  hipLaunchKernelGGL(transpose_oy_hl32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (unsigned char*)out, B, H, W,
                     C, shift_x, P, lines, tiles_c, ntiles, scale);
  MRN_LAUNCH_CHECK("transpose_oy_hl32");
  return MRN_OK;
}

// the three copies shift_x = -1, 0, +1 of mrn_transpose_oy_hl32_f32 in one pass: out [3][C][lines][128 B]
MRN_EXPORT int mrn_transpose_oy3_hl32_f32(const float* x, void* out, int B, int H, int W, int C, const float* scale, void* stream) {
  MRN_CHECK_ARG(x && out && C % 4 == 0 && B > 0 && H > 0 && W > 0, "mrn_transpose_oy3_hl32_f32: bad operands");
  const long P = (long)B * H * W, lines = (P + 31) / 32, tiles_c = (C + 31) / 32, ntiles = lines * tiles_c;
  long grid = ntiles > 65536 ? 65536 : ntiles;
  hipLaunchKernelGGL(transpose_oy3_hl32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (unsigned char*)out, B, H,
                     W, C, P, lines, tiles_c, ntiles, (long)C * lines * 128, scale);
  MRN_LAUNCH_CHECK("transpose_oy3_hl32");
  return MRN_OK;
}

// The two operand passes and the final reduction of the Winograd-domain weight gradient of a 3x3 / stride 1 / pad 1 convolution
// (transpose_oy_wino_hl32_kernel, wino_wgrad_finish_kernel): t NHWC [B][H][W][C] fp32 -> out [6][C][ceil(B*H*ceil(W/4) / 32)][128 B];
// mode 0 = layer input (B^T over 6 columns), mode 1 = output gradient (A over 4 columns).
MRN_EXPORT int mrn_transpose_oy_wino_hl32_f32(const float* t, void* out, int B, int H, int W, int C, int mode, const float* scale,
                                              void* stream) {
  MRN_CHECK_ARG(t && out && C % 4 == 0 && B > 0 && H > 0 && W > 0 && (mode == 0 || mode == 1), "mrn_transpose_oy_wino_hl32_f32: bad operands");
  const int Wq = (W + 3) / 4;
  const long Pq = (long)B * H * Wq, lines = (Pq + 31) / 32, tiles_c = (C + 31) / 32, ntiles = lines * tiles_c;
  long grid = ntiles > 65536 ? 65536 : ntiles;
  if (mode == 0)
    hipLaunchKernelGGL(transpose_oy_wino_hl32_kernel<0>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, t, (unsigned char*)out, B,
                       H, W, Wq, C, Pq, lines, tiles_c, ntiles, scale);
  else
    hipLaunchKernelGGL(transpose_oy_wino_hl32_kernel<1>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, t, (unsigned char*)out, B,
                       H, W, Wq, C, Pq, lines, tiles_c, ntiles, scale);
  MRN_LAUNCH_CHECK("transpose_oy_wino_hl32");
  return MRN_OK;
}

// part [S][18][Cout][Cin] (group (m, ky) = m * 3 + ky of split-K chunk s, from mrn_gemm_x3_windows_hl32) -> dW [Cout][3][3][Cin]
// (oihw_accumulate 0), or ADDED into dW [Cout][Cin][3][3], the parameter's own layout (oihw_accumulate 1)
MRN_EXPORT int mrn_wino_wgrad_finish_f32(const float* part, float* dw, int S, int Cout, int Cin, int oihw_accumulate, void* stream) {
  MRN_CHECK_ARG(part && dw && S >= 1 && Cout >= 1 && Cin >= 4 && Cin % 4 == 0, "mrn_wino_wgrad_finish_f32: bad operands (Cin %% 4 == 0)");
  const long CC4 = (long)Cout * Cin / 4;
  long grid = (CC4 + 255) / 256;
  if (grid > 16384) grid = 16384;
  if (oihw_accumulate)
    hipLaunchKernelGGL(wino_wgrad_finish_kernel<true>, dim3((unsigned)grid, 3), dim3(256), 0, (hipStream_t)stream, part, dw, S, CC4, Cin / 4);
  else
    hipLaunchKernelGGL(wino_wgrad_finish_kernel<false>, dim3((unsigned)grid, 3), dim3(256), 0, (hipStream_t)stream, part, dw, S, CC4, Cin / 4);
  MRN_LAUNCH_CHECK("wino_wgrad_finish");
  return MRN_OK;
}
