// What the recurrent translation units share, each thing defined once: lstm.hip (BiLSTM layer), attn_decode.hip (attention decoders:
// teacher-forced, greedy, beam, lexicon-constrained beam) and their backward, lstm_bwd.hip and attn_bwd.hip.
//
// Samples are independent along the time recurrence, so one workgroup owns a 16-sample batch tile for the
// whole sequence: hidden state lives in LDS, cell state in registers, and only the recurrent weights stream
// from L2 each step.  Products run on v_mfma_f32_16x16x4_f32 (exact fp32): M = 16 samples, N = gate columns,
// K = hidden.  Wave w owns hidden units [64w, 64w+64) for all four gates, so the LSTM pointwise update is
// lane-local (the i,f,g,o pre-activations of a unit land in the same lane and register index).
// The k index is permuted (lane group g takes k = 16q+4g+r) so every operand read is one 16-byte access.
#pragma once
#include "hl32.hpp"

namespace {   // (internal to each including unit, as the kernels are)

constexpr int HID = 256;       // hidden size (reference configs: hidden_size=256)
constexpr int BT = 16;         // samples per workgroup
constexpr int HLD = HID + 4;   // padded LDS row
constexpr int NW = 16;         // waves per workgroup: wave w owns hidden units [16w, 16w+16) of every gate
constexpr int NTH = NW * 64;   // 1024 threads -- many waves in flight hide the L2 latency of the weight stream
// (the five constants above are the attention decoder's, which runs hidden = 256 only.)

// The LSTM layer kernels are templates over the hidden size HS in {128, 256, 512}.  A 16-unit tile of every gate belongs to one wave:
//   HS = 128   8 waves (512 threads), one unit tile each
//   HS = 256  16 waves (1024 threads), one unit tile each
//   HS = 512  16 waves, wave w walks unit tiles w and w + 16 one after the other inside a step (NP = 2 passes: the four gate accumulators
//             are reused, cell state and bias are held per pass).  Both passes read h of the step from LDS buffer `cur` and write the new h
//             to buffer `cur ^ 1`, so no pass ever sees a half-updated h; one barrier per step as at the other sizes.
template <int HS>
struct LstmGeom {
  static_assert(HS == 128 || HS == 256 || HS == 512, "LSTM layer kernels: hidden size 128, 256 or 512");
  static constexpr int NW = HS >= 256 ? 16 : HS / 16;   // waves per workgroup
  static constexpr int NP = HS / (16 * NW);             // unit tiles (passes) per wave and step
  static constexpr int NTH = NW * 64;
  static constexpr int HLD = HS + 4;                    // padded fp32 LDS row
  static constexpr int LDH = HS + 8;                    // padded fp16 LDS row (halves)
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc[g] += A(16 x K from LDS rows of stride lda) . W_g^T   for K a multiple of 16.
// W is FRAGMENT-MAJOR: Wp[((wave*NG + g)*Q + q)*64 + lane] is the float4 the lane feeds to the four MFMAs of k-step q,
//   = W[g*HID + 16*wave + (lane&15)][16q + 4*(lane>>4) .. +3]
// so every wave-level load is one contiguous 1 KiB line instead of 16 rows x 64 B (pack_fragment_major on the host).
// Weight fragments of step q+1 are fetched before the MFMAs of step q issue; consecutive MFMAs target different
// accumulators (the 16x16x4 f32 MFMA has a 40-cycle dependent latency vs 32-cycle issue).
// mma_rows_k is the product over the k-steps of the columns [k0, k0 + kn) of the K-wide W, with A holding just those kn columns (from
// its column 0): the wide-context decoder keeps one chunk of the context in LDS at a time.  Chunk after chunk on the same accumulators,
// the MFMAs run in the order of one mma_rows over all of K.
template <int NG>
__device__ __forceinline__ void mma_rows_k(f32x4 (&acc)[NG], const float* __restrict__ a_lds, int lda,
                                           const float* __restrict__ Wp, int K, int k0, int kn, int wave, int lane) {
  const int n = lane & 15, g4 = (lane >> 4) * 4;
  const float* ap = a_lds + n * lda + g4;
  const int Q = K / 16, nq = kn / 16;
  const f32x4* wp = reinterpret_cast<const f32x4*>(Wp) + (long)wave * NG * Q * 64 + (long)(k0 / 16) * 64 + lane;
  f32x4 wv[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) wv[g] = wp[(long)g * Q * 64];
#pragma unroll 1
  for (int q = 0; q < nq; ++q) {
    f32x4 wn[NG];
    const int qn = (q + 1 < nq) ? q + 1 : q;
#pragma unroll
    for (int g = 0; g < NG; ++g) wn[g] = wp[((long)g * Q + qn) * 64];
    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + q * 16);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int g = 0; g < NG; ++g) acc[g] = mfma4(av[r], wv[g][r], acc[g]);
#pragma unroll
    for (int g = 0; g < NG; ++g) wv[g] = wn[g];
  }
}
template <int NG>
__device__ __forceinline__ void mma_rows(f32x4 (&acc)[NG], const float* __restrict__ a_lds, int lda,
                                         const float* __restrict__ Wp, int K, int wave, int lane) {
  mma_rows_k<NG>(acc, a_lds, lda, Wp, K, 0, K, wave, lane);
}

// The LSTM cell on accumulators that hold the input projection plus the recurrent product: c and h of the four samples of a lane;
// act[g][r] receives the post-activation gates (i, f, g, o) for the backward pass
__device__ __forceinline__ void lstm_pointwise0(const f32x4 (&acc)[4], const float (&bh)[4], float (&c)[4], float (&h)[4], float (&act)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float gi = acc[0][r] + bh[0];
    const float gf = acc[1][r] + bh[1];
    const float gg = acc[2][r] + bh[2];
    const float go = acc[3][r] + bh[3];
    const float ig = sigmoidf_acc(gi), fg = sigmoidf_acc(gf), og = sigmoidf_acc(go), cg = tanhf(gg);
    const float cn = fg * c[r] + ig * cg;
    c[r] = cn;
    h[r] = og * tanhf(cn);
    act[0][r] = ig; act[1][r] = fg; act[2][r] = cg; act[3][r] = og;
  }
}

// (the form that gets the input projection xg apart: acc + xg first, then the bias)
__device__ __forceinline__ void lstm_pointwise(const f32x4 (&acc)[4], const float (&xg)[4][4], const float (&bh)[4],
                                               float (&c)[4], float (&h)[4], float (&act)[4][4]) {
  f32x4 sum[4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[g][r] = acc[g][r] + xg[g][r];
  lstm_pointwise0(sum, bh, c, h, act);
}

// Up to MAX_GROUPS independent layers (the frozen experts of the router phase) share one launch: grid.x = groups * tiles.
constexpr int MAX_GROUPS = 8;

constexpr int LDH = HID + 8;   // fp16 LDS row (halves): 528 B, 16 rows hit 16 distinct 16-byte bank groups

// acc[g] += A(16 x K, fp16 hi / lo planes in LDS) . W_g^T with W FRAGMENT-MAJOR fp16:
//   Wp[(((wave*NG + g)*Q + q)*64 + lane)*2 + {0: hi, 1: lo}] = 8 halves W[g*HID + 16*wave + (lane&15)][32q + 8*(lane>>4) .. +7]
template <int NG>
__device__ __forceinline__ void mma_rows_h(f32x4 (&acc)[NG], const _Float16* __restrict__ a_hi, const _Float16* __restrict__ a_lo,
                                           const unsigned char* __restrict__ Wp, int K, int wave, int lane, int ld = LDH) {
  const int n = lane & 15, kg = lane >> 4;
  const int Q = K / 32;
  const f16v8* wp = reinterpret_cast<const f16v8*>(Wp) + ((long)wave * NG * Q * 64 + lane) * 2;
  const _Float16* ah = a_hi + n * ld + kg * 8;
  const _Float16* al = a_lo + n * ld + kg * 8;
  f16v8 wh[NG], wl[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    wh[g] = wp[(long)g * Q * 128];
    wl[g] = wp[(long)g * Q * 128 + 1];
  }
#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    f16v8 nh[NG], nl[NG];
    const int qn = (q + 1 < Q) ? q + 1 : q;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      nh[g] = wp[((long)g * Q + qn) * 128];
      nl[g] = wp[((long)g * Q + qn) * 128 + 1];
    }
    const f16v8 xh = *reinterpret_cast<const f16v8*>(ah + q * 32), xl = *reinterpret_cast<const f16v8*>(al + q * 32);
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wh[g], acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wl[g], acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wh[g], acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      wh[g] = nh[g];
      wl[g] = nl[g];
    }
  }
}

// mma_rows_h with the weight stream behind a buffer resource: scalar (wave, gate, k-step) offsets + one 32-bit lane offset, no 64-bit
// fragment pointers in the vector file (the pointer form put the decoder kernel 60 registers over its 128).
// mma_rows_hb_k is the product over the k-steps of the columns [k0, k0 + kn) of the K-wide stream, A holding just those kn columns
// (see mma_rows_k)
template <int NG>
__device__ __forceinline__ void mma_rows_hb_k(f32x4 (&acc)[NG], const _Float16* __restrict__ a_hi, const _Float16* __restrict__ a_lo,
                                              const __amdgpu_buffer_rsrc_t rw, int K, int k0, int kn, int wave, int lane, int ld) {
  const int n = lane & 15, kg = lane >> 4;
  const int Q = K / 32, q0 = k0 / 32, nq = kn / 32;
  const int wwave = __builtin_amdgcn_readfirstlane(wave) * NG * Q * 2048;
  const int wlane = lane * 32;
  auto wfrag = [&](int g, int q, int plane) -> f16v8 {
    return __builtin_bit_cast(f16v8, __builtin_amdgcn_raw_buffer_load_b128(rw, wlane, wwave + ((g * Q + q0 + q) * 128 + plane) * 16, 0));
  };
  const _Float16* ah = a_hi + n * ld + kg * 8;
  const _Float16* al = a_lo + n * ld + kg * 8;
  f16v8 wh[NG], wl[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    wh[g] = wfrag(g, 0, 0);
    wl[g] = wfrag(g, 0, 1);
  }
#pragma unroll 1
  for (int q = 0; q < nq; ++q) {
    f16v8 nh[NG], nl[NG];
    const int qn = (q + 1 < nq) ? q + 1 : q;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      nh[g] = wfrag(g, qn, 0);
      nl[g] = wfrag(g, qn, 1);
    }
    const f16v8 xh = *reinterpret_cast<const f16v8*>(ah + q * 32), xl = *reinterpret_cast<const f16v8*>(al + q * 32);
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wh[g], acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wl[g], acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wh[g], acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      wh[g] = nh[g];
      wl[g] = nl[g];
    }
  }
}
template <int NG>
__device__ __forceinline__ void mma_rows_hb(f32x4 (&acc)[NG], const _Float16* __restrict__ a_hi, const _Float16* __restrict__ a_lo,
                                            const __amdgpu_buffer_rsrc_t rw, int K, int wave, int lane, int ld = LDH) {
  mma_rows_hb_k<NG>(acc, a_hi, a_lo, rw, K, 0, K, wave, lane, ld);
}

__device__ __forceinline__ void store_h_split(_Float16* hi, _Float16* lo, int idx, float v) {
  _Float16 h, l;
  split_f16(v, h, l);
  hi[idx] = h;
  lo[idx] = l;
}

// (group, tile) of workgroup blockIdx.x among groups x tiles pairs (the sets of the LSTM layers, the experts of the attention decoders).
// pinned == 0: group-major; 1: all tiles of a group on XCD (group % 8) (workgroup b runs on XCD b % 8; groups past the last come out
// >= `groups`: the workgroup returns); 2: the pairs in group-major order cut into eight equal runs, one per XCD
__device__ __forceinline__ void group_tile(int groups, int tiles, int pinned, int& group, int& tile) {
  if (pinned == 2) {
    const int per = groups * tiles / 8;
    const int pair = (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
    group = pair / tiles;
    tile = pair - group * tiles;
  } else {
    group = pinned ? (int)(blockIdx.x % 8) + 8 * (int)((blockIdx.x / 8) / tiles) : (int)blockIdx.x / tiles;
    tile = pinned ? (int)((blockIdx.x / 8) % tiles) : (int)blockIdx.x % tiles;
  }
}

// The host side of group_tile: `pinned` and the grid of a launch of groups x tiles workgroups.  A group owns one weight stream (1 MiB at
// hidden 256): from `pin_from` groups on, and while a group's tiles fit the 32 CUs of an XCD, its tiles share one XCD's 4 MiB L2 instead
// of every XCD cycling through every group's weights (pinned == 1: whole rounds of eight groups; the workgroups past the last group
// return).  `balance` prefers the eight equal runs (pinned == 2) where the pairs divide by eight and fit one workgroup per CU
inline dim3 group_grid(int groups, int tiles, int pin_from, bool balance, int& pinned) {
  pinned = groups >= pin_from && tiles * ceil_div(groups, 8) <= 32;
  if (balance && groups >= pin_from && (groups * tiles) % 8 == 0 && groups * tiles <= 256) pinned = 2;
  return dim3(pinned == 1 ? 8 * ceil_div(groups, 8) * tiles : groups * tiles);
}

// the hidden sizes the LSTM layer kernels, forward and backward, are instantiated for (LstmGeom)
inline bool lstm_hidden_ok(int hidden) { return hidden == 128 || hidden == 256 || hidden == 512; }

__device__ __forceinline__ float fast_tanh(float x) {
  // tanh(x) = 1 - 2/(exp(2x)+1); saturates correctly through inf / 0
  const float e = __expf(2.f * x);
  return 1.f - 2.f / (e + 1.f);
}

}  // namespace
