// Bidirectional LSTM layer: the exact-fp32 and split-fp16 x3 layer kernels, templates over the hidden size (LstmGeom), and their launchers.
//
// Reference: modules/sequence_modeling.py:7-21 (nn.LSTM bidirectional, gate order i,f,g,o).  The workgroup geometry and the MFMA
// helpers are recurrent.hpp's, shared with the attention decoders (attn_decode.hip).
#include "hl32.hpp"
#include "recurrent.hpp"
#include <stdlib.h>

namespace {

// ---------------------------------------------------------------------------------------------
// Bidirectional LSTM layer.  xproj[b][t][dir*4H + gate*H + j] holds W_ih x + b_ih.
// grid = (ceil(B/16), ndir); out[b][t][dir*H + j].
// ---------------------------------------------------------------------------------------------
struct LstmParams {
  const float* xproj; const float* w_hh; const float* b_hh; float* out;
  float* gates_out;   // optional [B][T][ndir][4H]
  float* c_out;       // optional [B][T][ndir][H]
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
  // set = (group, direction) owns one W_hh stream (4 * HS * HS floats: 1 MiB at 256); all tiles of a set run on ONE XCD (block b lands on
  // XCD b % 8) so the stream stays resident in that XCD's 4 MiB L2 instead of every XCD cycling through every set's weights
  // (only while a set's tiles fit the 32 CUs of an XCD; larger batches keep the plain block order)
  const int set = grp.pinned ? (int)(blockIdx.x % 8) + 8 * (int)((blockIdx.x / 8) / grp.tiles) : (int)blockIdx.x / grp.tiles;
  if (set >= grp.nsets) return;
  const int gi = set / grp.ndir;
  const float* __restrict__ xproj = grp.g[gi].xproj;
  const float* __restrict__ w_hh = grp.g[gi].w_hh;
  const float* __restrict__ b_hh = grp.g[gi].b_hh;
  float* __restrict__ out = grp.g[gi].out;
  float* __restrict__ gates_out = grp.g[gi].gates_out;
  float* __restrict__ c_out = grp.g[gi].c_out;
  const int B = grp.B, T = grp.T, ndir = grp.ndir;
  const int dir = set - gi * grp.ndir;
  const int b0 = (grp.pinned ? (int)((blockIdx.x / 8) % grp.tiles) : (int)blockIdx.x % grp.tiles) * BT;
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
// Inference variant of the LSTM layer for the FROZEN experts of the router phase: the recurrent product runs as
// split-fp16 x3 on v_mfma_f32_16x16x32_f16 (h = hi + lo written to LDS as two fp16 planes by the pointwise stage, W_hh
// pre-split with a power-of-two prescale into a fragment-major fp16 stream of the same byte size), 96 MFMAs of 16 cycles
// per wave and step instead of 256 MFMAs of 32 cycles on the exact-fp32 matrix pipe.  Same launch geometry, grouping and
// XCD pinning as lstm_layer_kernel; no training saves.
// ---------------------------------------------------------------------------------------------
struct LstmX3Params {
  const float* xproj; const unsigned char* w_hh; const float* w_inv; const float* b_hh; float* out;
  float* gates_out;   // optional training saves, as in LstmParams: [B][T][ndir][4H] post-activation gates
  float* c_out;       //                                          [B][T][ndir][H] cell state
};
struct LstmX3Group {
  LstmX3Params g[MAX_GROUPS];
  int tiles, B, T, ndir, nsets, pinned;
};

// RB: 16-sample row blocks per workgroup.  A workgroup streams the whole W_hh of its (expert, direction) set through one CU every step
// (1 MiB; 64 B / clk / CU from L2 = 7.8 us), with little MFMA work behind each fragment (96 MFMAs of 16 cycles per wave).  RB = 2 -- the same
// stream for twice the samples, half as many workgroups per L2 -- was built and measured SLOWER (round 6, tools/bench_lstm.py, B = 256,
// T = 65: G = 1 17.1 us / step against 11.8, G = 3 21.3 / 14.8, G = 6 22.9 / 15.3): with registers for the next hi fragments only, the
// second row block's MFMAs wait on the lo fragments instead of hiding them.  RB = 1 is the product form; MRN_LSTM_RB=2 selects the other
// for an A/B (bit-identical results).
// The input projection is the accumulators' INITIAL value, scaled by the weights' power-of-two prescale (exact): no registers of its own.
// Every global access is a buffer instruction (resource + scalar offset + a 32-bit lane offset).  Both changes are round 6's: the form
// with 64-bit row and fragment pointers in vector registers ran at the 128-register cap; this one takes 100 and is 12-24 % faster
// (G = 1 13.3 -> 11.8 us / step, G = 3 17.9 -> 14.8, G = 6 20.3 -> 15.3).
template <int HS, int RB>
__global__ __launch_bounds__(LstmGeom<HS>::NTH) void lstm_layer_x3_kernel(const LstmX3Group grp) {
  constexpr int HID = HS, NW = LstmGeom<HS>::NW, NP = LstmGeom<HS>::NP, NTH = LstmGeom<HS>::NTH, LDH = LstmGeom<HS>::LDH;
  constexpr int BTX = BT * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char lstm_lds[];
  _Float16* const h_hi = reinterpret_cast<_Float16*>(lstm_lds);        // [2][BTX * LDH]
  _Float16* const h_lo = h_hi + 2 * BTX * LDH;                         // [2][BTX * LDH]
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
  const int b0 = tile * BTX;
  const int t_ = threadIdx.x, lane = t_ & 63, wave = t_ >> 6;
  const unsigned char* W = grp.g[gi].w_hh + (long)dir * 4 * HID * HID * 4;     // hi + lo fp16 = 4 bytes per weight
  const float inv = grp.g[gi].w_inv[dir];
  const float pre = 1.f / inv;                                                 // the prescale itself (a power of two: exact)
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  const int j = wave * 16 + col;                 // this lane's hidden unit of pass 0 (pass p: + 16 * NW * p)

  for (int i = t_; i < BTX * LDH; i += NTH) {
    h_hi[i] = (_Float16)0.f;
    h_lo[i] = (_Float16)0.f;
  }
  float c[NP][RB][4], bh[NP][4];
  // per-lane BYTE offsets of this lane's rows in xproj / the gate saves ([B][T][ndir][4H]); the (t, direction) part of an address is
  // wave-uniform and goes into the scalar base, and the [B][T][ndir][H] arrays' offsets follow from the same registers -- eight
  // loop-invariant registers instead of a 64-bit pointer per row and array (which the compiler hoisted and, at RB = 2, spilled).
  // The launcher keeps B * T * ndir * 4H * 4 bytes below 2^32 (larger batches go in several launches)
  unsigned xoff[RB][4];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + rb * BT + rbase + r;
#pragma unroll
      for (int p = 0; p < NP; ++p) c[p][rb][r] = 0.f;
      xoff[rb][r] = ((unsigned)(b < B ? b : 0) * (unsigned)(T * ndir * 4 * HID) + (unsigned)j) * 4u;
    }
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int g = 0; g < 4; ++g) bh[p][g] = b_hh ? b_hh[dir * 4 * HID + g * HID + j + 16 * NW * p] : 0.f;
  __syncthreads();

  // fragment-major weight stream of this wave: [g][q][lane][hi 8 | lo 8 halves] (mma_rows_h's layout)
  constexpr int Q = HID / 32;
  // every global access is a buffer instruction -- resource + scalar offset + one 32-bit lane offset: no address lives in the vector file
  // (as 64-bit pointers per gate / row the compiler hoisted them out of the step loop and, at RB = 2, spilled them)
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
    _Float16* const nhi = h_hi + (cur ^ 1) * BTX * LDH;
    _Float16* const nlo = h_lo + (cur ^ 1) * BTX * LDH;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      // pass p: unit tile wave + NW * p -- its weight fragments, its columns of every row (a scalar offset on top of pass 0's)
      auto wfrag = [&](int g, int q, int plane) -> f16v8 {
        return __builtin_bit_cast(f16v8, __builtin_amdgcn_raw_buffer_load_b128(rw, wlane, wwave + p * WPASS + ((g * Q + q) * 128 + plane) * 16, 0));
      };
      f32x4 acc[RB][4];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            acc[rb][g][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (int)xoff[rb][r], 4 * tq + g * HID * 4 + p * UPASS, 0)) * pre;
        }
      {
        const _Float16* ah = h_hi + cur * BTX * LDH + n * LDH + kg * 8;
        const _Float16* al = h_lo + cur * BTX * LDH + n * LDH + kg * 8;
        // RB = 1: the hi and lo fragments of k-step q + 1 are fetched before the MFMAs of step q issue.  RB = 2 has registers for the next hi
        // fragments only: the lo fragments of step q are fetched at its top and used by its LAST product group
        constexpr bool PF_LO = RB == 1;
        f16v8 wh[4], wl[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          wh[g] = wfrag(g, 0, 0);
          if (PF_LO) wl[g] = wfrag(g, 0, 1);
        }
#pragma unroll 1
        for (int q = 0; q < Q; ++q) {
          f16v8 nh[4], nl[4];
          const int qn = (q + 1 < Q) ? q + 1 : q;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            if (!PF_LO) wl[g] = wfrag(g, q, 1);
            nh[g] = wfrag(g, qn, 0);
            if (PF_LO) nl[g] = wfrag(g, qn, 1);
          }
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            const f16v8 xh = *reinterpret_cast<const f16v8*>(ah + rb * BT * LDH + q * 32), xl = *reinterpret_cast<const f16v8*>(al + rb * BT * LDH + q * 32);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[rb][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wh[g], acc[rb][g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[rb][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wh[g], acc[rb][g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[rb][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wl[g], acc[rb][g], 0, 0, 0);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            wh[g] = nh[g];
            if (PF_LO) wl[g] = nl[g];
          }
        }
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[rb][g] *= inv;        // undo the power-of-two weight prescale (exact): x-projection + W_hh . h
        float h[4], act[4][4];
        lstm_pointwise0(acc[rb], bh[p], c[p][rb], h, act);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rb * BT + rbase + r, b = b0 + row;
          if (b < B) {
            const int ooff = (int)(((xoff[rb][r] - 4u * (unsigned)j) >> 2) + 4u * (unsigned)j);       // the same row of a [B][T][ndir][H] array
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h[r]), ro, ooff, tq + p * UPASS, 0);
            if (gates_out) {
#pragma unroll
              for (int g = 0; g < 4; ++g) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, act[g][r]), rg, (int)xoff[rb][r], 4 * tq + g * HID * 4 + p * UPASS, 0);
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, c[p][rb][r]), rc, ooff, tq + p * UPASS, 0);
            }
          }
          store_h_split(nhi, nlo, row * LDH + j + 16 * NW * p, b < B ? h[r] : 0.f);
        }
      }
    }
    __syncthreads();
  }
}

// one launch of a filled group
template <int HS, int RB>
static int lstm_x3_launch_rb(LstmX3Group& grp, int n, bool may_pin, hipStream_t stream) {
  constexpr size_t lds = (size_t)4 * BT * RB * LstmGeom<HS>::LDH * sizeof(_Float16);
  static bool once = false;
  if (!once) {
    (void)hipFuncSetAttribute((const void*)lstm_layer_x3_kernel<HS, RB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    once = true;
  }
  grp.tiles = ceil_div(grp.B, BT * RB);
  grp.nsets = n * grp.ndir;
  grp.pinned = 0;
  int blocks = grp.nsets * grp.tiles;
  if (may_pin) {
    grp.pinned = grp.nsets > 2 && grp.tiles * ceil_div(grp.nsets, 8) <= 32;
    if (grp.pinned) blocks = 8 * ceil_div(grp.nsets, 8) * grp.tiles;
    static const bool balance = !(getenv("MRN_LSTM_BALANCE") && atoi(getenv("MRN_LSTM_BALANCE")) == 0);     // (A/B switch, read once)
    if (balance && grp.nsets > 2 && (grp.nsets * grp.tiles) % 8 == 0 && grp.nsets * grp.tiles <= 256) {
      grp.pinned = 2;
      blocks = grp.nsets * grp.tiles;
    }
  }
  hipLaunchKernelGGL((lstm_layer_x3_kernel<HS, RB>), dim3(blocks), dim3(LstmGeom<HS>::NTH), lds, stream, grp);
  return 0;
}
template <int HS>
static int lstm_x3_launch_hs(LstmX3Group& all, int n, bool may_pin, hipStream_t stream) {
  constexpr int HID = HS;
  static const int forced = getenv("MRN_LSTM_RB") ? atoi(getenv("MRN_LSTM_RB")) : 0;
  // the kernel's row offsets are 32-bit byte offsets into [B][T][ndir][4H] floats: batches beyond that go in chunks of whole tiles
  // (a row is 4 * HS floats per direction and step, so at 512 the chunk boundary falls at half the batch of 256)
  const long row_bytes = (long)all.T * all.ndir * 4 * HID * 4;
  const long fit = 0xffffffffL / row_bytes / (2 * BT) * (2 * BT);
  MRN_CHECK_ARG(fit >= 2 * BT, "lstm x3 layer: T=%d is beyond the kernel's 32-bit row offsets", all.T);
  for (long s0 = 0; s0 < all.B; s0 += fit) {
    LstmX3Group grp = all;
    grp.B = (int)(all.B - s0 < fit ? all.B - s0 : fit);
    for (int i = 0; i < n; ++i) {
      LstmX3Params& q = grp.g[i];
      q.xproj += s0 * (row_bytes / 4);
      q.out += s0 * (row_bytes / 16);
      if (q.gates_out) q.gates_out += s0 * (row_bytes / 4);
      if (q.c_out) q.c_out += s0 * (row_bytes / 16);
    }
    int rc;
    if constexpr (HS <= 256) rc = forced == 2 ? lstm_x3_launch_rb<HS, 2>(grp, n, may_pin, stream) : lstm_x3_launch_rb<HS, 1>(grp, n, may_pin, stream);
    else rc = lstm_x3_launch_rb<HS, 1>(grp, n, may_pin, stream);     // (RB = 2 with two passes spills at the 128-register cap: not built)
    if (rc) return rc;
  }
  return 0;
}
static int lstm_x3_launch(LstmX3Group& all, int n, bool may_pin, int hidden, hipStream_t stream) {
  switch (hidden) {
    case 128: return lstm_x3_launch_hs<128>(all, n, may_pin, stream);
    case 256: return lstm_x3_launch_hs<256>(all, n, may_pin, stream);
    default: return lstm_x3_launch_hs<512>(all, n, may_pin, stream);
  }
}

// (A weight-stationary variant -- W_hh slices in the LDS of 16 workgroups per (expert, direction), h exchanged through L2 every step --
// was built, bit-identical and measured slower in round 2: G = 3 22.3 us / step against 17.1 streaming, G = 6 23.9 against 22.4; the
// hand-over of h at agent scope costs more than streaming W_hh.  Removed in round 4; DESIGN.md section 7 keeps the measurements.)

}  // namespace

static int lstm_launch(LstmGroup& grp, int groups, int hidden, hipStream_t st) {
  grp.nsets = groups * grp.ndir;
  grp.pinned = grp.nsets > 2 && grp.tiles * ceil_div(grp.nsets, 8) <= 32;   // (a single layer already fits every L2)
  const int blocks = grp.pinned ? 8 * ceil_div(grp.nsets, 8) * grp.tiles : grp.nsets * grp.tiles;
  switch (hidden) {
    case 128: hipLaunchKernelGGL(lstm_layer_kernel<128>, dim3(blocks), dim3(LstmGeom<128>::NTH), 0, st, grp); break;
    case 256: hipLaunchKernelGGL(lstm_layer_kernel<256>, dim3(blocks), dim3(LstmGeom<256>::NTH), 0, st, grp); break;
    default: {
      constexpr size_t lds = sizeof(float) * 2 * BT * LstmGeom<512>::HLD;
      static bool once = false;
      if (!once) {
        (void)hipFuncSetAttribute((const void*)lstm_layer_kernel<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        once = true;
      }
      hipLaunchKernelGGL(lstm_layer_kernel<512>, dim3(blocks), dim3(LstmGeom<512>::NTH), lds, st, grp);
    }
  }
  MRN_LAUNCH_CHECK("lstm_layer");
  return MRN_OK;
}

static inline bool lstm_hidden_ok(int hidden) { return hidden == 128 || hidden == 256 || hidden == 512; }

MRN_EXPORT int mrn_lstm_layer_fwd_f32(const float* xproj, const float* w_hh, const float* b_hh, float* out,
                                      float* gates_out, float* c_out, int B, int T, int hidden, int ndir, void* stream) {
  MRN_CHECK_ARG(xproj && w_hh && out, "mrn_lstm_layer_fwd_f32: null operand");
  MRN_CHECK_ARG(lstm_hidden_ok(hidden), "mrn_lstm_layer_fwd_f32: hidden=%d unsupported (the LSTM layer kernels are built for 128, 256 and 512)", hidden);
  MRN_CHECK_ARG(ndir == 1 || ndir == 2, "mrn_lstm_layer_fwd_f32: ndir=%d", ndir);
  MRN_CHECK_ARG((gates_out == nullptr) == (c_out == nullptr), "mrn_lstm_layer_fwd_f32: gates_out / c_out must come together");
  if (B == 0 || T == 0) return MRN_OK;
  LstmGroup grp;
  memset(&grp, 0, sizeof(grp));
  grp.g[0] = LstmParams{xproj, w_hh, b_hh, out, gates_out, c_out};
  grp.tiles = ceil_div(B, BT); grp.B = B; grp.T = T; grp.ndir = ndir;
  return lstm_launch(grp, 1, hidden, (hipStream_t)stream);
}

// `groups` independent layers of identical geometry in one launch.  xproj / w_hh / b_hh / out are HOST arrays of
// `groups` device pointers (b_hh may be NULL or hold NULL entries).
MRN_EXPORT int mrn_lstm_layer_fwd_grouped_f32(const void* const* xproj, const void* const* w_hh, const void* const* b_hh,
                                              const void* const* out, int groups, int B, int T, int hidden, int ndir,
                                              void* stream) {
  MRN_CHECK_ARG(xproj && w_hh && out && groups >= 1, "mrn_lstm_layer_fwd_grouped_f32: null operand");
  MRN_CHECK_ARG(lstm_hidden_ok(hidden), "mrn_lstm_layer_fwd_grouped_f32: hidden=%d unsupported (the LSTM layer kernels are built for 128, 256 and 512)", hidden);
  MRN_CHECK_ARG(ndir == 1 || ndir == 2, "mrn_lstm_layer_fwd_grouped_f32: ndir=%d", ndir);
  if (B == 0 || T == 0) return MRN_OK;
  for (int g0 = 0; g0 < groups; g0 += MAX_GROUPS) {
    const int n = groups - g0 < MAX_GROUPS ? groups - g0 : MAX_GROUPS;
    LstmGroup grp;
    memset(&grp, 0, sizeof(grp));
    for (int i = 0; i < n; ++i) {
      MRN_CHECK_ARG(xproj[g0 + i] && w_hh[g0 + i] && out[g0 + i], "mrn_lstm_layer_fwd_grouped_f32: null operand in group %d", g0 + i);
      grp.g[i] = LstmParams{(const float*)xproj[g0 + i], (const float*)w_hh[g0 + i], b_hh ? (const float*)b_hh[g0 + i] : nullptr,
                            (float*)out[g0 + i], nullptr, nullptr};
    }
    grp.tiles = ceil_div(B, BT); grp.B = B; grp.T = T; grp.ndir = ndir;
    const int rc = lstm_launch(grp, n, hidden, (hipStream_t)stream);
    if (rc) return rc;
  }
  return MRN_OK;
}

// Inference-only LSTM layers of `groups` frozen experts with the recurrent product on the f16 MFMA (split-fp16 x3).
// w_hh: HOST array of device pointers to the fragment-major fp16 streams ([ndir][H/16][4][H/32][64][hi 8 | lo 8 halves],
// ops.pack_fragment_major_h), w_inv: HOST array of device float[ndir] = 1 / prescale of each direction's weights.
MRN_EXPORT int mrn_lstm_layer_fwd_x3_grouped(const void* const* xproj, const void* const* w_hh, const void* const* w_inv,
                                             const void* const* b_hh, const void* const* out, int groups, int B, int T,
                                             int hidden, int ndir, void* stream) {
  MRN_CHECK_ARG(xproj && w_hh && w_inv && out && groups >= 1, "mrn_lstm_layer_fwd_x3_grouped: null operand");
  MRN_CHECK_ARG(lstm_hidden_ok(hidden), "mrn_lstm_layer_fwd_x3_grouped: hidden=%d unsupported (the LSTM layer kernels are built for 128, 256 and 512)", hidden);
  MRN_CHECK_ARG(ndir == 1 || ndir == 2, "mrn_lstm_layer_fwd_x3_grouped: ndir=%d", ndir);
  if (B == 0 || T == 0) return MRN_OK;
  for (int g0 = 0; g0 < groups; g0 += MAX_GROUPS) {
    const int n = groups - g0 < MAX_GROUPS ? groups - g0 : MAX_GROUPS;
    LstmX3Group grp;
    memset(&grp, 0, sizeof(grp));
    for (int i = 0; i < n; ++i) {
      MRN_CHECK_ARG(xproj[g0 + i] && w_hh[g0 + i] && w_inv[g0 + i] && out[g0 + i], "mrn_lstm_layer_fwd_x3_grouped: null operand in group %d", g0 + i);
      grp.g[i] = LstmX3Params{(const float*)xproj[g0 + i], (const unsigned char*)w_hh[g0 + i], (const float*)w_inv[g0 + i],
                              b_hh ? (const float*)b_hh[g0 + i] : nullptr, (float*)out[g0 + i]};
    }
    grp.B = B; grp.T = T; grp.ndir = ndir;
    const int rc = lstm_x3_launch(grp, n, true, hidden, (hipStream_t)stream);
    if (rc) return rc;
    MRN_LAUNCH_CHECK("lstm_layer_x3");
  }
  return MRN_OK;
}

// One layer being TRAINED with the recurrent product as split-fp16 x3 (the arithmetic of the trained convolutions, fp16x3s): the
// forward of mrn_lstm_layer_fwd_x3_grouped for one network, plus the saves mrn_lstm_layer_bwd_f32 reads (gates [B][T][ndir][4H]
// post-activation, cseq [B][T][ndir][H]).  Half the time per step of the exact-fp32 kernel (96 MFMAs of 16 cycles instead of 256 of 32).
MRN_EXPORT int mrn_lstm_layer_fwd_x3_save(const float* xproj, const void* w_hh, const float* w_inv, const float* b_hh, float* out,
                                          float* gates_out, float* c_out, int B, int T, int hidden, int ndir, void* stream) {
  MRN_CHECK_ARG(xproj && w_hh && w_inv && out && gates_out && c_out, "mrn_lstm_layer_fwd_x3_save: null operand");
  MRN_CHECK_ARG(lstm_hidden_ok(hidden), "mrn_lstm_layer_fwd_x3_save: hidden=%d unsupported (the LSTM layer kernels are built for 128, 256 and 512)", hidden);
  MRN_CHECK_ARG(ndir == 1 || ndir == 2, "mrn_lstm_layer_fwd_x3_save: ndir=%d", ndir);
  if (B == 0 || T == 0) return MRN_OK;
  LstmX3Group grp;
  memset(&grp, 0, sizeof(grp));
  grp.g[0] = LstmX3Params{xproj, (const unsigned char*)w_hh, w_inv, b_hh, out, gates_out, c_out};
  grp.B = B; grp.T = T; grp.ndir = ndir;
  const int rc = lstm_x3_launch(grp, 1, false, hidden, (hipStream_t)stream);
  if (rc) return rc;
  MRN_LAUNCH_CHECK("lstm_layer_x3_save");
  return MRN_OK;
}
