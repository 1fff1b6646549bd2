// Bidirectional LSTM layer: the exact-fp32 and split-fp16 x3 layer kernels, templates over the hidden size (LstmGeom), and their launchers.
//
// Reference: modules/sequence_modeling.py:7-21 (nn.LSTM bidirectional, gate order i,f,g,o).  The workgroup geometry and the MFMA
// helpers are recurrent.hpp's, shared with the backward through time (lstm_bwd.hip) and the attention decoders (attn_decode.hip).
#include "hl32.hpp"
#include "recurrent.hpp"
#include <stdlib.h>

namespace {

// ---------------------------------------------------------------------------------------------
// Bidirectional LSTM layer.  xproj[b][t][dir*4H + gate*H + j] holds W_ih x + b_ih.
// grid = sets x ceil(B/16) workgroups (group_grid); out[b][t][dir*H + j].
// ---------------------------------------------------------------------------------------------
struct LstmParams {
  const float* xproj;
  const void* w_hh;      // fragment-major W_hh per direction: fp32 (pack_fragment_major), or the fp16 hi / lo stream of the x3 kernel
  const float* w_inv;    // x3: float[ndir] = 1 / prescale of each direction's stream; null in the fp32 form
  const float* b_hh; float* out;
  float* gates_out;   // optional training saves: [B][T][ndir][4H] post-activation gates
  float* c_out;       //                          [B][T][ndir][H] cell state
};
struct LstmGroup {
  LstmParams g[MAX_GROUPS];
  int tiles, B, T, ndir, nsets, pinned;
};

template <int HS>
__global__ __launch_bounds__(LstmGeom<HS>::NTH) void lstm_layer_kernel(const LstmGroup grp) {
  constexpr int HID = HS, NW = LstmGeom<HS>::NW, NP = LstmGeom<HS>::NP, NTH = LstmGeom<HS>::NTH, HLD = LstmGeom<HS>::HLD;
  // two h buffers of [BT][HLD] floats: static up to 256, dynamic at 512 (66 048 bytes, past the 64 KiB of a static allocation)
  extern __shared__ __attribute__((aligned(16))) float lstm_f32_dyn[];
  __shared__ __attribute__((aligned(16))) float h_static[HS <= 256 ? 2 * BT * HLD : 4];
  float* const h_lds0 = HS <= 256 ? h_static : lstm_f32_dyn;
  // set = (group, direction) owns one W_hh stream (4 * HS * HS floats: 1 MiB at 256); pinned, all tiles of a set run on ONE XCD
  int set, tile;
  group_tile(grp.nsets, grp.tiles, grp.pinned, set, tile);
  if (set >= grp.nsets) return;
  const int gi = set / grp.ndir;
  const float* __restrict__ xproj = grp.g[gi].xproj;
  const float* __restrict__ w_hh = static_cast<const float*>(grp.g[gi].w_hh);
  const float* __restrict__ b_hh = grp.g[gi].b_hh;
  float* __restrict__ out = grp.g[gi].out;
  float* __restrict__ gates_out = grp.g[gi].gates_out;
  float* __restrict__ c_out = grp.g[gi].c_out;
  const int B = grp.B, T = grp.T, ndir = grp.ndir;
  const int dir = set - gi * grp.ndir;
  const int b0 = tile * BT;
  const int t_ = threadIdx.x, lane = t_ & 63, wave = t_ >> 6;
  const float* W = w_hh + (long)dir * 4 * HID * HID;
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  const int j0 = wave * 16 + col;              // this lane's hidden unit of pass 0 (pass p: + 16 * NW * p)

  for (int i = t_; i < BT * HLD; i += NTH) h_lds0[i] = 0.f;
  float c[NP][4], bh[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      c[p][g] = 0.f;
      bh[p][g] = b_hh ? b_hh[dir * 4 * HID + g * HID + j0 + 16 * NW * p] : 0.f;
    }
  __syncthreads();

  // Two passes: the sample index goes through an empty asm inside the step, so the row addresses of the five arrays are formed per step
  // (a few VALU ops) instead of being hoisted as 64-bit pointers per row, array and pass -- hoisted, they put the kernel 13 registers over
  // the 128 of a 1024-thread workgroup.  One pass (128, 256): the plain index, the kernel as it was.
  auto row_of = [](int b) -> int {
    if constexpr (NP > 1) asm volatile("" : "+v"(b));
    return b;
  };
  for (int step = 0; step < T; ++step) {
    const int t = dir == 0 ? step : T - 1 - step;
    const int cur = step & 1;
    const float* h_cur = h_lds0 + cur * (BT * HLD);
    float* h_new = h_lds0 + (cur ^ 1) * (BT * HLD);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int JP = 16 * NW * p;                // pass p's units sit JP floats behind pass 0's in every row: a constant on pass 0's addresses
      // input projections of this step: issued first, they land while the recurrent product runs
      float xg[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + rbase + r;
        const float* xp = xproj + ((long)row_of(b < B ? b : 0) * T + t) * (ndir * 4 * HID) + dir * 4 * HID + j0;
#pragma unroll
        for (int g = 0; g < 4; ++g) xg[g][r] = xp[g * HID + JP];
      }
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma_rows<4>(acc, h_cur, HLD, W, HID, wave + NW * p, lane);
      float h[4], act[4][4];
      lstm_pointwise(acc, xg, bh[p], c[p], h, act);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rbase + r, b = b0 + row;
        if (b < B) {
          const int bs = row_of(b);
          (out + ((long)bs * T + t) * (ndir * HID) + dir * HID + j0)[JP] = h[r];
          if (gates_out) {
            const long base = ((long)bs * T + t) * ndir + dir;
#pragma unroll
            for (int g = 0; g < 4; ++g) (gates_out + base * 4 * HID + j0)[g * HID + JP] = act[g][r];
            (c_out + base * HID + j0)[JP] = c[p][r];
          }
        }
        (h_new + row * HLD + j0)[JP] = b < B ? h[r] : 0.f;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// The layer with the recurrent product as split-fp16 x3 on v_mfma_f32_16x16x32_f16 (h = hi + lo written to LDS as two fp16 planes by
// the pointwise stage, W_hh pre-split with a power-of-two prescale into a fragment-major fp16 stream of the same byte size), 96 MFMAs
// of 16 cycles per wave and step instead of 256 MFMAs of 32 cycles on the exact-fp32 matrix pipe: the frozen experts of the router
// phase, and a layer being trained (with the saves).  Same launch geometry and grouping as lstm_layer_kernel.
//
// A workgroup streams the whole W_hh of its (expert, direction) set through one CU every step (1 MiB; 64 B / clk / CU from L2 = 7.8 us),
// with little MFMA work behind each fragment (96 MFMAs of 16 cycles per wave).  A 32-sample tile -- the same stream for twice the
// samples, half as many workgroups per L2 -- was built and measured SLOWER (tools/bench_lstm.py, B = 256, T = 65: G = 1 17.1 us / step
// against 11.8, G = 3 21.3 / 14.8, G = 6 22.9 / 15.3): with registers for the next hi fragments only, the second row block's MFMAs wait
// on the lo fragments instead of hiding them.  It is gone; DESIGN.md section 7 keeps the measurements.
// The input projection is the accumulators' INITIAL value, scaled by the weights' power-of-two prescale (exact): no registers of its own.
// Every global access is a buffer instruction (resource + scalar offset + a 32-bit lane offset): the form with 64-bit row and fragment
// pointers in vector registers ran at the 128-register cap; this one takes 100 and is 12-24 % faster (G = 1 13.3 -> 11.8 us / step,
// G = 3 17.9 -> 14.8, G = 6 20.3 -> 15.3).
// ---------------------------------------------------------------------------------------------
template <int HS>
__global__ __launch_bounds__(LstmGeom<HS>::NTH) void lstm_layer_x3_kernel(const LstmGroup grp) {
  constexpr int HID = HS, NW = LstmGeom<HS>::NW, NP = LstmGeom<HS>::NP, NTH = LstmGeom<HS>::NTH, LDH = LstmGeom<HS>::LDH;
  extern __shared__ __attribute__((aligned(16))) unsigned char lstm_lds[];
  _Float16* const h_hi = reinterpret_cast<_Float16*>(lstm_lds);        // [2][BT * LDH]
  _Float16* const h_lo = h_hi + 2 * BT * LDH;                          // [2][BT * LDH]
  // pinned == 1: all tiles of a (expert, direction) set run on XCD (set % 8), whose L2 then holds that set's W_hh stream (4 * HS * HS * 4 bytes: 1 MiB at 256).
  // pinned == 2: the (set, tile) pairs in set-major order are cut into eight equal runs, one per XCD (workgroup b runs on XCD b % 8): every
  // L2 serves the same number of workgroups and at most two or three sets' weights.  The step time follows the number of workgroups
  // streaming through one L2 (13.1 us at 4, 17.4 at 16, 21.9 at 32): 12 sets = 24 per XCD instead of 32 / 16, 6 sets = 12 instead of 16 / 0.
  int set, tile;
  group_tile(grp.nsets, grp.tiles, grp.pinned, set, tile);
  if (set >= grp.nsets) return;
  const int gi = set / grp.ndir;
  const float* __restrict__ xproj = grp.g[gi].xproj;
  const float* __restrict__ b_hh = grp.g[gi].b_hh;
  float* __restrict__ out = grp.g[gi].out;
  float* __restrict__ gates_out = grp.g[gi].gates_out;
  float* __restrict__ c_out = grp.g[gi].c_out;
  const int B = grp.B, T = grp.T, ndir = grp.ndir;
  const int dir = set - gi * grp.ndir;
  const int b0 = tile * BT;
  const int t_ = threadIdx.x, lane = t_ & 63, wave = t_ >> 6;
  const unsigned char* W = static_cast<const unsigned char*>(grp.g[gi].w_hh) + (long)dir * 4 * HID * HID * 4;     // hi + lo fp16 = 4 bytes per weight
  const float inv = grp.g[gi].w_inv[dir];
  const float pre = 1.f / inv;                                                 // the prescale itself (a power of two: exact)
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  const int j = wave * 16 + col;                 // this lane's hidden unit of pass 0 (pass p: + 16 * NW * p)

  for (int i = t_; i < BT * LDH; i += NTH) {
    h_hi[i] = (_Float16)0.f;
    h_lo[i] = (_Float16)0.f;
  }
  float c[NP][4], bh[NP][4];
  // per-lane BYTE offsets of this lane's rows in xproj / the gate saves ([B][T][ndir][4H]); the (t, direction) part of an address is
  // wave-uniform and goes into the scalar base, and the [B][T][ndir][H] arrays' offsets follow from the same registers -- four
  // loop-invariant registers instead of a 64-bit pointer per row and array.
  // The launcher keeps B * T * ndir * 4H * 4 bytes below 2^32 (larger batches go in several launches)
  unsigned xoff[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + rbase + r;
#pragma unroll
    for (int p = 0; p < NP; ++p) c[p][r] = 0.f;
    xoff[r] = ((unsigned)(b < B ? b : 0) * (unsigned)(T * ndir * 4 * HID) + (unsigned)j) * 4u;
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int g = 0; g < 4; ++g) bh[p][g] = b_hh ? b_hh[dir * 4 * HID + g * HID + j + 16 * NW * p] : 0.f;
  __syncthreads();

  // fragment-major weight stream of this wave: [g][q][lane][hi 8 | lo 8 halves] (mma_rows_h's layout)
  constexpr int Q = HID / 32;
  // every global access is a buffer instruction -- resource + scalar offset + one 32-bit lane offset: no address lives in the vector file
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(W, 4 * HID * HID * 4);
  const int wwave = __builtin_amdgcn_readfirstlane(wave) * (4 * Q * 64 * 32);
  const int wlane = lane * 32;
  constexpr int WPASS = NW * (4 * Q * 64 * 32);        // bytes between the unit tiles of two passes of a wave
  constexpr int UPASS = 16 * NW * 4;                  // bytes between their hidden units in a row of floats
  const unsigned xbytes = (unsigned)B * (unsigned)(T * ndir * 4 * HID) * 4u;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(xproj, xbytes);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, xbytes / 4);
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(gates_out, gates_out ? xbytes : 0);
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(c_out, gates_out ? xbytes / 4 : 0);
  const int n = lane & 15, kg = lane >> 4;

  for (int step = 0; step < T; ++step) {
    const int t = dir == 0 ? step : T - 1 - step;
    const int cur = step & 1;
    const int tq = (t * ndir + dir) * HID * 4;                                     // (wave-uniform) byte offset in a [..][T][ndir][H] row
    _Float16* const nhi = h_hi + (cur ^ 1) * BT * LDH;
    _Float16* const nlo = h_lo + (cur ^ 1) * BT * LDH;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      // pass p: unit tile wave + NW * p -- its weight fragments, its columns of every row (a scalar offset on top of pass 0's)
      auto wfrag = [&](int g, int q, int plane) -> f16v8 {
        return __builtin_bit_cast(f16v8, __builtin_amdgcn_raw_buffer_load_b128(rw, wlane, wwave + p * WPASS + ((g * Q + q) * 128 + plane) * 16, 0));
      };
      f32x4 acc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          acc[g][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (int)xoff[r], 4 * tq + g * HID * 4 + p * UPASS, 0)) * pre;
      }
      {
        const _Float16* ah = h_hi + cur * BT * LDH + n * LDH + kg * 8;
        const _Float16* al = h_lo + cur * BT * LDH + n * LDH + kg * 8;
        // the hi and lo fragments of k-step q + 1 are fetched before the MFMAs of step q issue
        f16v8 wh[4], wl[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          wh[g] = wfrag(g, 0, 0);
          wl[g] = wfrag(g, 0, 1);
        }
#pragma unroll 1
        for (int q = 0; q < Q; ++q) {
          f16v8 nh[4], nl[4];
          const int qn = (q + 1 < Q) ? q + 1 : q;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            nh[g] = wfrag(g, qn, 0);
            nl[g] = wfrag(g, qn, 1);
          }
          const f16v8 xh = *reinterpret_cast<const f16v8*>(ah + q * 32), xl = *reinterpret_cast<const f16v8*>(al + q * 32);
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wh[g], acc[g], 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wh[g], acc[g], 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wl[g], acc[g], 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            wh[g] = nh[g];
            wl[g] = nl[g];
          }
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] *= inv;        // undo the power-of-two weight prescale (exact): x-projection + W_hh . h
      float h[4], act[4][4];
      lstm_pointwise0(acc, bh[p], c[p], h, act);
      // (The outer loop makes one trip and is for the compiler alone: the row loop is then unrolled and simplified as a loop body of its
      // own before the two passes are unrolled around it.  Without it the two-pass kernel comes out with another schedule and 114
      // registers instead of 110; with it all three sizes keep the code they had with the one-row-block tile loop in this place.)
#pragma unroll
      for (int once = 0; once < 1; ++once) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rbase + r, b = b0 + row;
          if (b < B) {
            const int ooff = (int)(((xoff[r] - 4u * (unsigned)j) >> 2) + 4u * (unsigned)j);       // the same row of a [B][T][ndir][H] array
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h[r]), ro, ooff, tq + p * UPASS, 0);
            if (gates_out) {
#pragma unroll
              for (int g = 0; g < 4; ++g) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, act[g][r]), rg, (int)xoff[r], 4 * tq + g * HID * 4 + p * UPASS, 0);
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, c[p][r]), rc, ooff, tq + p * UPASS, 0);
            }
          }
          store_h_split(nhi, nlo, row * LDH + j + 16 * NW * p, b < B ? h[r] : 0.f);
        }
      }
    }
    __syncthreads();
  }
}

// one launch of a filled group: the placement of its (group, direction) sets, the kernel of the form and its LDS
template <int HS>
static void lstm_launch_hs(LstmGroup& grp, int n, bool x3, bool balance, hipStream_t st) {
  using Geom = LstmGeom<HS>;
  grp.tiles = ceil_div(grp.B, BT);
  grp.nsets = n * grp.ndir;
  // pinned from three sets on (the two of a single layer already fit every L2)
  const dim3 grid = group_grid(grp.nsets, grp.tiles, 3, balance, grp.pinned);
  // x3: two fp16 planes of two h buffers; fp32: two h buffers, static in the kernel up to 256
  const size_t lds = x3 ? sizeof(_Float16) * 4 * BT * Geom::LDH : HS <= 256 ? 0 : sizeof(float) * 2 * BT * Geom::HLD;
  const auto kernel = x3 ? lstm_layer_x3_kernel<HS> : lstm_layer_kernel<HS>;
  static bool once[2] = {false, false};
  if (lds && !once[x3]) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    once[x3] = true;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(Geom::NTH), lds, st, grp);
}

// The x3 kernel's row offsets are 32-bit byte offsets into [B][T][ndir][4H] floats: batches beyond that go in chunks of whole multiples
// of 2 * BT samples (a row is 4 * HS floats per direction and step, so at 512 the chunk boundary falls at half the batch of 256).
// The fp32 kernel forms 64-bit addresses: one launch.  The eight-run placement (pinned == 2) was measured on the x3 kernel only
static int lstm_launch(LstmGroup& all, int n, bool x3, int hidden, hipStream_t st) {
  static const bool balance = !(getenv("MRN_LSTM_BALANCE") && atoi(getenv("MRN_LSTM_BALANCE")) == 0);     // (A/B switch, read once)
  const long row_bytes = (long)all.T * all.ndir * 4 * hidden * 4;
  const long fit = x3 ? 0xffffffffL / row_bytes / (2 * BT) * (2 * BT) : all.B;
  MRN_CHECK_ARG(!x3 || fit >= 2 * BT, "lstm x3 layer: T=%d is beyond the kernel's 32-bit row offsets", all.T);
  for (long s0 = 0; s0 < all.B; s0 += fit) {
    LstmGroup grp = all;
    grp.B = (int)(all.B - s0 < fit ? all.B - s0 : fit);
    for (int i = 0; i < n; ++i) {
      LstmParams& q = grp.g[i];
      q.xproj += s0 * (row_bytes / 4);
      q.out += s0 * (row_bytes / 16);
      if (q.gates_out) q.gates_out += s0 * (row_bytes / 4);
      if (q.c_out) q.c_out += s0 * (row_bytes / 16);
    }
    switch (hidden) {
      case 128: lstm_launch_hs<128>(grp, n, x3, x3 && balance, st); break;
      case 256: lstm_launch_hs<256>(grp, n, x3, x3 && balance, st); break;
      default: lstm_launch_hs<512>(grp, n, x3, x3 && balance, st);
    }
  }
  return MRN_OK;
}

// (A weight-stationary variant -- W_hh slices in the LDS of 16 workgroups per (expert, direction), h exchanged through L2 every step --
// was built, bit-identical and measured slower in round 2: G = 3 22.3 us / step against 17.1 streaming, G = 6 23.9 against 22.4; the
// hand-over of h at agent scope costs more than streaming W_hh.  Removed in round 4; DESIGN.md section 7 keeps the measurements.)

}  // namespace

// The four forward entry points: `groups` layers of identical geometry, one launch per MAX_GROUPS of them.  xproj / w_hh / w_inv / b_hh /
// out are HOST arrays of `groups` device pointers (b_hh may be NULL or hold NULL entries); x3 == false: w_inv is ignored.  The
// single-layer entry points (`single`) pass arrays of one and may give the training saves, which the x3 one always does
static int lstm_fwd(const char* who, bool x3, bool single, const void* const* xproj, const void* const* w_hh, const void* const* w_inv,
                    const void* const* b_hh, const void* const* out, float* gates_out, float* c_out, int groups, int B, int T, int hidden,
                    int ndir, void* stream) {
  auto given = [&](int g) { return xproj[g] && w_hh[g] && (!x3 || w_inv[g]) && out[g]; };
  MRN_CHECK_ARG(xproj && w_hh && (!x3 || w_inv) && out && groups >= 1 && (!single || (given(0) && (!x3 || (gates_out && c_out)))),
                "%s: null operand", who);
  MRN_CHECK_ARG(lstm_hidden_ok(hidden), "%s: hidden=%d unsupported (the LSTM layer kernels are built for 128, 256 and 512)", who, hidden);
  MRN_CHECK_ARG(ndir == 1 || ndir == 2, "%s: ndir=%d", who, ndir);
  MRN_CHECK_ARG((gates_out == nullptr) == (c_out == nullptr), "%s: gates_out / c_out must come together", who);
  if (B == 0 || T == 0) return MRN_OK;
  for (int g0 = 0; g0 < groups; g0 += MAX_GROUPS) {
    const int n = groups - g0 < MAX_GROUPS ? groups - g0 : MAX_GROUPS;
    LstmGroup grp;
    memset(&grp, 0, sizeof(grp));
    for (int i = 0; i < n; ++i) {
      const int g = g0 + i;
      MRN_CHECK_ARG(given(g), "%s: null operand in group %d", who, g);
      grp.g[i] = LstmParams{(const float*)xproj[g], w_hh[g], x3 ? (const float*)w_inv[g] : nullptr, b_hh ? (const float*)b_hh[g] : nullptr,
                            (float*)out[g], gates_out, c_out};
    }
    grp.B = B; grp.T = T; grp.ndir = ndir;
    const int rc = lstm_launch(grp, n, x3, hidden, (hipStream_t)stream);
    if (rc) return rc;
    MRN_LAUNCH_CHECK(!x3 ? "lstm_layer" : single ? "lstm_layer_x3_save" : "lstm_layer_x3");
  }
  return MRN_OK;
}

MRN_EXPORT int mrn_lstm_layer_fwd_f32(const float* xproj, const float* w_hh, const float* b_hh, float* out,
                                      float* gates_out, float* c_out, int B, int T, int hidden, int ndir, void* stream) {
  const void* const a[] = {xproj, w_hh, b_hh, out};
  return lstm_fwd("mrn_lstm_layer_fwd_f32", false, true, a, a + 1, nullptr, a + 2, a + 3, gates_out, c_out, 1, B, T, hidden, ndir, stream);
}

// `groups` independent layers of identical geometry in one launch.  xproj / w_hh / b_hh / out are HOST arrays of
// `groups` device pointers (b_hh may be NULL or hold NULL entries).
MRN_EXPORT int mrn_lstm_layer_fwd_grouped_f32(const void* const* xproj, const void* const* w_hh, const void* const* b_hh,
                                              const void* const* out, int groups, int B, int T, int hidden, int ndir,
                                              void* stream) {
  return lstm_fwd("mrn_lstm_layer_fwd_grouped_f32", false, false, xproj, w_hh, nullptr, b_hh, out, nullptr, nullptr, groups, B, T, hidden,
                  ndir, stream);
}

// Inference-only LSTM layers of `groups` frozen experts with the recurrent product on the f16 MFMA (split-fp16 x3).
// w_hh: HOST array of device pointers to the fragment-major fp16 streams ([ndir][H/16][4][H/32][64][hi 8 | lo 8 halves],
// ops.pack_fragment_major_h), w_inv: HOST array of device float[ndir] = 1 / prescale of each direction's weights.
MRN_EXPORT int mrn_lstm_layer_fwd_x3_grouped(const void* const* xproj, const void* const* w_hh, const void* const* w_inv,
                                             const void* const* b_hh, const void* const* out, int groups, int B, int T,
                                             int hidden, int ndir, void* stream) {
  return lstm_fwd("mrn_lstm_layer_fwd_x3_grouped", true, false, xproj, w_hh, w_inv, b_hh, out, nullptr, nullptr, groups, B, T, hidden, ndir,
                  stream);
}

// One layer being TRAINED with the recurrent product as split-fp16 x3 (the arithmetic of the trained convolutions, fp16x3s): the
// forward of mrn_lstm_layer_fwd_x3_grouped for one network, plus the saves mrn_lstm_layer_bwd_f32 reads (gates [B][T][ndir][4H]
// post-activation, cseq [B][T][ndir][H]).  Half the time per step of the exact-fp32 kernel (96 MFMAs of 16 cycles instead of 256 of 32).
MRN_EXPORT int mrn_lstm_layer_fwd_x3_save(const float* xproj, const void* w_hh, const float* w_inv, const float* b_hh, float* out,
                                          float* gates_out, float* c_out, int B, int T, int hidden, int ndir, void* stream) {
  const void* const a[] = {xproj, w_hh, w_inv, b_hh, out};
  return lstm_fwd("mrn_lstm_layer_fwd_x3_save", true, true, a, a + 1, a + 2, a + 3, a + 4, gates_out, c_out, 1, B, T, hidden, ndir, stream);
}
