// LSTM backward through time (reference il_modules/mrn.py:260-261 `loss.backward()` through modules/sequence_modeling.py): one kernel,
// a template over the hidden size and the arithmetic of its recurrent product, exact fp32 or split-fp16 x3.
//
// The geometry is the forward kernels' (lstm.hip; recurrent.hpp: LstmGeom, BT): 8 waves at 128, 16 at 256, and at 512 16 waves that each
// own the hidden units of two 16-unit tiles (w and w + 16, NP = 2 passes).  A step first writes the gate gradients of ALL of a wave's
// units to LDS, then -- behind the barrier -- forms dh_rec of all of them: no pass reads a half-written row.
#include "hl32.hpp"
#include "recurrent.hpp"

namespace {

template <int HS>
struct LstmBwdGeom {
  static constexpr int GLD = 4 * HS + 4;      // fp32 LDS row of gate gradients
  static constexpr int GLDH = 4 * HS + 8;     // fp16 LDS row (halves)
};

// The gradients d = (di, df, dg, do) with respect to the gate pre-activations of hidden unit j of sample b at time t (tp: the previous
// time in the direction's order, read while step > 0); dc_next carries the cell-state gradient to the step before.  Written to dgates
// as well; all zero for a row past the batch.
template <int HID>
__device__ __forceinline__ void lstm_gate_grads(const float* __restrict__ dout, const float* __restrict__ gates, const float* __restrict__ cseq,
                                                float* __restrict__ dgates, int b, int B, int T, int ndir, int dir, int t, int tp, int step,
                                                int j, float dh_rec, float& dc_next, float (&d)[4]) {
  float di = 0.f, df = 0.f, dg = 0.f, dob = 0.f;
  if (b < B) {
    const long base = ((long)b * T + t) * ndir + dir;
    const float* gp = gates + base * 4 * HID + j;
    const float ig = gp[0], fg = gp[HID], gg = gp[2 * HID], og = gp[3 * HID];
    const float ct = cseq[base * HID + j];
    const float cp = step > 0 ? cseq[(((long)b * T + tp) * ndir + dir) * HID + j] : 0.f;
    const float dh = dout[((long)b * T + t) * (ndir * HID) + dir * HID + j] + dh_rec;
    const float tc = tanhf(ct);
    dob = dh * tc * og * (1.f - og);
    const float dc = dc_next + dh * og * (1.f - tc * tc);
    di = dc * gg * ig * (1.f - ig);
    df = dc * cp * fg * (1.f - fg);
    dg = dc * ig * (1.f - gg * gg);
    dc_next = dc * fg;
    float* dp = dgates + base * 4 * HID + j;
    dp[0] = di; dp[HID] = df; dp[2 * HID] = dg; dp[3 * HID] = dob;
  }
  d[0] = di; d[1] = df; d[2] = dg; d[3] = dob;
}

// gates [B][T][ndir][4H] (post-activation i,f,g,o), cseq [B][T][ndir][H], dout [B][T][ndir*H]
// w_hhT: fragment-major W_hh^T (rows = hidden unit j, K = 4H gate index), one gate group
// dgates [B][T][ndir][4H]: gradient with respect to the gate pre-activations
// X3: the recurrent product dh_rec = dgates . W_hh as split-fp16 x3 on v_mfma_f32_16x16x32_f16: the gate gradients are written to LDS as
// two fp16 planes of gscale * dgate (gscale: a power of two from max|dout|, the gradients are 1e-3 .. 1e-8-sized), W_hh^T comes as the
// fragment-major hi / lo stream of ops.pack_fragment_major_h with its own prescale (w_inv).  96 MFMAs of 16 cycles per wave and step
// instead of 256 of 32 on the exact-fp32 pipe (at 256): the step was bound by them (4 waves per SIMD).  The fp32 form reads neither
// w_inv nor gscale.
template <int HS, bool X3>
__global__ __launch_bounds__(LstmGeom<HS>::NTH) void lstm_layer_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ gates,
                                                                           const float* __restrict__ cseq, const void* __restrict__ w_hhT,
                                                                           const float* __restrict__ w_inv, const float* __restrict__ gscale,
                                                                           float* __restrict__ dgates, int B, int T, int ndir) {
  constexpr int HID = HS, NW = LstmGeom<HS>::NW, NP = LstmGeom<HS>::NP, GLD = LstmBwdGeom<HS>::GLD, GLDH = LstmBwdGeom<HS>::GLDH;
  extern __shared__ __attribute__((aligned(16))) unsigned char dg_raw[];
  float* const dg_lds = reinterpret_cast<float*>(dg_raw);             // fp32: [BT][GLD]
  _Float16* const dg_hi = reinterpret_cast<_Float16*>(dg_raw);        // x3: [2 planes][BT][GLDH]
  _Float16* const dg_lo = dg_hi + BT * GLDH;
  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * BT;
  const int t_ = threadIdx.x, lane = t_ & 63, wave = t_ >> 6;
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  const int j0 = wave * 16 + col;               // this lane's hidden unit of pass 0 (pass p: + 16 * NW * p)
  // this direction's W_hh^T: HID x 4 HID weights of 4 bytes in either form (fp32, or fp16 hi + lo)
  const unsigned char* const W = static_cast<const unsigned char*>(w_hhT) + (long)dir * HID * 4 * HID * 4;
  float gs = 1.f, unscale = 1.f;
  if constexpr (X3) {
    gs = gscale[0];
    unscale = w_inv[dir] * gscale[1];
  }
  float dh_rec[NP][4], dc_next[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) dh_rec[p][r] = dc_next[p][r] = 0.f;

  for (int step = T - 1; step >= 0; --step) {
    const int t = dir == 0 ? step : T - 1 - step;           // time index processed at forward step `step`
    const int tp = dir == 0 ? t - 1 : t + 1;                // previous time in the direction's order
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int j = j0 + 16 * NW * p;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rbase + r;
        float d[4];
        lstm_gate_grads<HID>(dout, gates, cseq, dgates, b0 + row, B, T, ndir, dir, t, tp, step, j, dh_rec[p][r], dc_next[p][r], d);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if constexpr (X3) {
            _Float16 hh, ll;
            split_f16_sat(d[g] * gs, hh, ll);
            dg_hi[row * GLDH + g * HID + j] = hh;
            dg_lo[row * GLDH + g * HID + j] = ll;
          } else {
            dg_lds[row * GLD + g * HID + j] = d[g];
          }
        }
      }
    }
    __syncthreads();
    if (step > 0) {
      // dh_rec[b][j] = sum_n dgate[b][n] * W_hh[n][j]: unit tile wave + NW * p of pass p
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
        if constexpr (X3) mma_rows_h<1>(acc, dg_hi, dg_lo, W, 4 * HID, wave + NW * p, lane, GLDH);
        else mma_rows<1>(acc, dg_lds, GLD, reinterpret_cast<const float*>(W), 4 * HID, wave + NW * p, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh_rec[p][r] = X3 ? acc[0][r] * unscale : acc[0][r];
      }
    }
    __syncthreads();
  }
}

template <int HS, bool X3>
static void lstm_bwd_launch(const float* dout, const float* gates, const float* cseq, const void* w_hhT, const float* w_inv,
                            const float* gscale, float* dgates, int B, int T, int ndir, hipStream_t st) {
  constexpr size_t lds = X3 ? sizeof(_Float16) * 2 * BT * LstmBwdGeom<HS>::GLDH : sizeof(float) * BT * LstmBwdGeom<HS>::GLD;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)lstm_layer_bwd_kernel<HS, X3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = true;
  }
  hipLaunchKernelGGL((lstm_layer_bwd_kernel<HS, X3>), dim3(ceil_div(B, BT), ndir), dim3(LstmGeom<HS>::NTH), lds, st, dout, gates, cseq,
                     w_hhT, w_inv, gscale, dgates, B, T, ndir);
}

template <bool X3>
static int lstm_bwd(const char* who, const char* kernel, const float* dout, const float* gates, const float* cseq, const void* w_hhT,
                    const float* w_inv, const float* gscale, float* dgates, int B, int T, int hidden, int ndir, void* stream) {
  MRN_CHECK_ARG(dout && gates && cseq && w_hhT && (!X3 || (w_inv && gscale)) && dgates, "%s: null operand", who);
  MRN_CHECK_ARG(lstm_hidden_ok(hidden) && (ndir == 1 || ndir == 2),
                "%s: hidden=%d ndir=%d unsupported (the LSTM layer kernels are built for 128, 256 and 512)", who, hidden, ndir);
  if (B == 0 || T == 0) return MRN_OK;
  switch (hidden) {
    case 128: lstm_bwd_launch<128, X3>(dout, gates, cseq, w_hhT, w_inv, gscale, dgates, B, T, ndir, (hipStream_t)stream); break;
    case 256: lstm_bwd_launch<256, X3>(dout, gates, cseq, w_hhT, w_inv, gscale, dgates, B, T, ndir, (hipStream_t)stream); break;
    default: lstm_bwd_launch<512, X3>(dout, gates, cseq, w_hhT, w_inv, gscale, dgates, B, T, ndir, (hipStream_t)stream);
  }
  MRN_LAUNCH_CHECK(kernel);
  return MRN_OK;
}

}  // namespace

MRN_EXPORT int mrn_lstm_layer_bwd_f32(const float* dout, const float* gates, const float* cseq, const float* w_hhT,
                                      float* dgates, int B, int T, int hidden, int ndir, void* stream) {
  return lstm_bwd<false>("mrn_lstm_layer_bwd_f32", "lstm_layer_bwd", dout, gates, cseq, w_hhT, nullptr, nullptr, dgates, B, T, hidden, ndir,
                         stream);
}

// mrn_lstm_layer_bwd_f32 with the recurrent product as split-fp16 x3: w_hhT_h = per direction the fragment-major fp16 hi / lo stream of
// W_hh^T [H][4H] (ops.pack_fragment_major_h), w_inv device float[ndir] = 1 / its prescale, gscale device float[2] = {s, 1/s} with a power
// of two s that brings max|dout| to ~16 (mrn_pow2_scale_f32: the gate gradients are split as s * dgate; fp16 keeps a factor 4096 of headroom)
MRN_EXPORT int mrn_lstm_layer_bwd_x3(const float* dout, const float* gates, const float* cseq, const void* w_hhT_h, const float* w_inv,
                                     const float* gscale, float* dgates, int B, int T, int hidden, int ndir, void* stream) {
  return lstm_bwd<true>("mrn_lstm_layer_bwd_x3", "lstm_layer_bwd_x3", dout, gates, cseq, w_hhT_h, w_inv, gscale, dgates, B, T, hidden, ndir,
                        stream);
}
