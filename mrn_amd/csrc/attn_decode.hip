// Attention decoders: teacher-forced, greedy, beam, lexicon-constrained beam and beam with a character n-gram model, one persistent
// kernel each around one shared attention-cell step; their launch rules and entry points.
//
// Reference: modules/prediction.py:38-118 (Attention / AttentionCell, 26 decode steps).  The workgroup geometry and the MFMA
// helpers are recurrent.hpp's, shared with the BiLSTM layer (lstm.hip) and the backward (attn_bwd.hip).
#include "char_lm.hpp"
#include "hl32.hpp"
#include "recurrent.hpp"
#include <math.h>
#include <stdlib.h>

namespace {

// ---------------------------------------------------------------------------------------------
// Attention decoder, all S steps in one launch (reference recomputes i2h(H) every step and issues ~10
// small launches per step; here i2h(H) and the embedding half of the LSTMCell input projection are hoisted
// into GEMMs by the caller).
//   Hb     [B][T][D]      encoder states (D multiple of 16)
//   Hproj  [B][T][HID]    i2h(Hb)
//   eproj  [B][S][4*HID]  W_ih[:, D:] . emb(text) + b_ih       (teacher forced)
//   hid    [B][S][HID]    decoder hidden states (generator GEMM is applied afterwards)
// Greedy mode (tokens fed back through argmax of the generator) uses the same kernel one step at a time:
//   steps = 1, state carried in h_state / c_state.
// ---------------------------------------------------------------------------------------------
struct AttnDecParams {
  const float* Hb; const float* Hproj; const float* eproj;
  const float* w_h2h; const float* b_h2h; const float* w_score;
  const float* w_ih;                // context part of LSTMCell weight_ih ([4H][D]), fragment-major
  const float* w_hh;                // [4H][HID], fragment-major (w_h2h too)
  const float* b_hh;                // optional [4H] (eproj already carries b_ih)
  float* hid;
  const float* w_inv;               // x3 form only: device float[3] = 1 / prescale of w_h2h, w_ih, w_hh (then fragment-major fp16 hi / lo streams)
  float* h_state; float* c_state;   // optional [B][HID] carried state (nullptr: start from zero, do not store)
  float* alpha_out;                 // optional [B][S][T]
  float* gates_out; float* c_out;   // optional training saves: [B][S][4H] post-activation gates, [B][S][H] cell state
  float* ctx_out; float* hp_out;    //                          [B][S][D] context vectors, [B][S][H] h2h(h)+b
  int B, T, D, S;
  long eproj_stride_b, eproj_stride_s, hid_stride_b, hid_stride_s;
};

struct AttnDecGroup {
  AttnDecParams g[MAX_GROUPS];
  int tiles, groups, pinned, vb;
};

// X3: the three recurrent products (h2h, W_ih[:, :D] on the context, W_hh) as split-fp16 x3 on v_mfma_f32_16x16x32_f16 -- h and the
// context live in LDS as fp16 hi / lo planes, the weights come as fragment-major hi / lo streams with a power-of-two prescale
// (ops.pack_fragment_major_h).  On the exact-fp32 pipe those products are 30 us of a step (576 MFMAs of 32 cycles per wave, four
// waves per SIMD); as x3 216 MFMAs of 16 cycles.
// WIDE: the context tile holds CTX_CHUNK columns instead of D.  Phases (4) and the context half of (5) then run chunk by chunk: form
// one chunk of every row's context, multiply it into the gate accumulators, next chunk (attn_launch takes this form when the whole
// tile would not fit the LDS budget: D = 256 * G for G >= 8 at T = 65, DERNet's main head).
constexpr int CTX_CHUNK = 1024;

// ---- the attention cell's step, shared by attn_decoder_kernel, attn_greedy_kernel and attn_beam_kernel -------------------------------
// A workgroup owns the 16 rows of an MFMA tile; `nrows` of them are in use, row r belongs to sample b0 + r / per (per = 1: a row per
// sample; the beam kernel's W entries of a sample share its Hproj / Hb slices), the others are treated like rows beyond the batch.  One
// step, the same arithmetic in the same order for every caller -- which is what makes a beam row's logits bit-identical to the greedy
// kernel's, and beam width 1 greedy:
//   (1) hp = h2h(h) + bias                                                                  } attn_scores
//   (2) e[row][t] = score . tanh(Hproj[b][t] + hp[row])                                     }
//   (3) alpha = softmax over t, one wave per row                                            }
//       the caller loads the embedding half of the LSTMCell input for the step (eproj, or the token's row of etab): issued here, it
//       lands during phase (4) and becomes the INITIAL value of the gate accumulators (x the W_ih stream's power-of-two prescale:
//       exact) -- sixteen registers live over one phase, not the step
//   (4) context[row][:] = sum_t alpha[row][t] * Hb[b][t][:]   (context_chunk; WIDE: chunk by chunk in (5))       } attn_cell
//   (5) gates = that seed + ctx . W_ih[:, :D]^T + h . W_hh^T                                                    }
//   (6) LSTM cell; the new h replaces the old one in LDS, (h, gates, c) go back to the caller for its own stores  }
// The LDS map, in floats: h [BT][HLD] (x3: two fp16 planes [BT][LDH]), hp [BT][HLD], ctx [BT][CLD] (x3: two fp16 planes [BT][CLDH]),
// e [BT][T], the score vector [HID]; a kernel's own arrays follow at sw_lds + HID.
template <bool X3>
struct AttnTile {
  float *h_lds, *hp_lds, *ctx_lds, *e_lds, *sw_lds;
  _Float16 *h_hi, *h_lo, *c_hi, *c_lo;
  int CLD, CLDH;                             // context row: fp32, fp16 planes
  __amdgpu_buffer_rsrc_t r_h2h, r_ih, r_hh;  // x3: the three fp16 weight streams (4 bytes per weight) behind buffer resources
  float inv_h2h, inv_ih, inv_hh;
  int b0, Bend, nrows, per;
  int t_, lane, wave, col, rbase, j;         // lane (col, rbase ... rbase + 3) of the MFMA tile; j: this lane's hidden unit
  float bj, bh[4];                           // its h2h and gate biases
  __device__ __forceinline__ int sample(int row) const { return b0 + row / per; }
};

// the view of workgroup `tile` (ns samples of `per` rows each, dc context columns in LDS); fills the tile: h from the carried state
// where one is given, else zero, everything else zero (rows not in use stay zero), the score vector.  The caller's barrier follows
template <bool X3>
__device__ __forceinline__ AttnTile<X3> attn_tile(float* lds, const AttnDecParams& p, int dc, int tile, int ns, int per) {
  AttnTile<X3> v;
  const int T = p.T;
  v.CLD = dc + 4;
  v.CLDH = dc + 8;
  v.h_lds = lds;
  v.hp_lds = X3 ? lds + (2 * BT * LDH) / 2 : v.h_lds + BT * HLD;
  v.ctx_lds = v.hp_lds + BT * HLD;
  v.e_lds = X3 ? v.ctx_lds + (2 * BT * v.CLDH) / 2 : v.ctx_lds + BT * v.CLD;
  v.sw_lds = v.e_lds + BT * T;
  v.h_hi = reinterpret_cast<_Float16*>(v.h_lds);
  v.h_lo = v.h_hi + BT * LDH;
  v.c_hi = reinterpret_cast<_Float16*>(v.ctx_lds);
  v.c_lo = v.c_hi + BT * v.CLDH;
  v.inv_h2h = X3 ? p.w_inv[0] : 1.f, v.inv_ih = X3 ? p.w_inv[1] : 1.f, v.inv_hh = X3 ? p.w_inv[2] : 1.f;
  v.r_h2h = make_rsrc(p.w_h2h, X3 ? HID * HID * 4 : 0);
  v.r_ih = make_rsrc(p.w_ih, X3 ? 4 * HID * p.D * 4 : 0);
  v.r_hh = make_rsrc(p.w_hh, X3 ? 4 * HID * HID * 4 : 0);
  v.b0 = tile * ns;
  v.Bend = min(p.B, v.b0 + ns);
  v.nrows = ns * per;
  v.per = per;
  v.t_ = threadIdx.x, v.lane = v.t_ & 63, v.wave = v.t_ >> 6;
  v.col = v.lane & 15, v.rbase = (v.lane >> 4) * 4;
  v.j = v.wave * 16 + v.col;

  const int ld = X3 ? LDH : HLD;
  for (int i = v.t_; i < BT * ld; i += NTH) {
    const int row = i / ld, jj = i - row * ld;
    const int b = v.sample(row);
    const float h0 = (p.h_state && b < v.Bend && jj < HID) ? p.h_state[(long)b * HID + jj] : 0.f;
    if constexpr (X3) store_h_split(v.h_hi, v.h_lo, i, h0);
    else v.h_lds[i] = h0;
  }
  for (int i = v.t_; i < BT * HLD + BT * (X3 ? v.CLDH : v.CLD) + BT * T; i += NTH) v.hp_lds[i] = 0.f;   // hp, ctx (planes), e
  for (int i = v.t_; i < HID; i += NTH) v.sw_lds[i] = p.w_score[i];
#pragma unroll
  for (int g = 0; g < 4; ++g) v.bh[g] = p.b_hh ? p.b_hh[g * HID + v.j] : 0.f;
  v.bj = p.b_h2h[v.j];
  return v;
}

// (1)-(3); ends behind the barrier that publishes alpha.  SAVES (here, in context_chunk and in attn_cell): the teacher-forced kernel's
// optional training saves hp_out, alpha_out and ctx_out.  The decoding kernels, whose parameters leave them null, compile them out: the
// row addresses of the saves stay live over the step, registers that attn_greedy_kernel and attn_beam_kernel do not have to spare
template <bool X3, bool SAVES>
__device__ __forceinline__ void attn_scores(const AttnTile<X3>& v, const AttnDecParams& p, int step) {
  const int T = p.T, lane = v.lane, wave = v.wave;
  // (1) hp = h2h(h) + bias
  {
    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if constexpr (X3) mma_rows_hb<1>(acc, v.h_hi, v.h_lo, v.r_h2h, HID, wave, lane);
    else mma_rows<1>(acc, v.h_lds, HLD, p.w_h2h, HID, wave, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float hp = acc[0][r] * v.inv_h2h + v.bj;
      v.hp_lds[(v.rbase + r) * HLD + v.j] = hp;
      const int b = v.sample(v.rbase + r);
      if (SAVES && p.hp_out && b < v.Bend) p.hp_out[((long)b * p.S + step) * HID + v.j] = hp;
    }
  }
  __syncthreads();
  // (2) e[row][t] = score . tanh(Hproj[b][t] + hp[row]); one wave per (row, t) pair, 4 channels per lane, four pairs in
  //     flight per wave so the Hproj loads (L2) and the cross-lane reductions of different pairs overlap
  {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(v.sw_lds + lane * 4);
    const int npair = v.nrows * T;
    constexpr int U = 4;                 // pairs in flight per wave (8 measured the same, round 6)
    for (int pr0 = wave * U; pr0 < npair; pr0 += NW * U) {
      f32x4 hv[U];
      int rows[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pr = pr0 + u;
        const int row = pr < npair ? pr / T : 0, t = pr < npair ? pr - row * T : 0;
        rows[u] = row;
        const int b = v.sample(row);
        hv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (pr < npair && b < v.Bend) hv[u] = *reinterpret_cast<const f32x4*>(p.Hproj + ((long)b * T + t) * HID + lane * 4);
      }
      float sacc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(v.hp_lds + rows[u] * HLD + lane * 4);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) s = fmaf(wv[k], fast_tanh(hv[u][k] + pv[k]), s);
        sacc[u] = s;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) sacc[u] += __shfl_xor(sacc[u], o);
      }
      if (lane < U && pr0 + lane < npair) {
        float s = sacc[0];
#pragma unroll
        for (int u = 1; u < U; ++u) s = lane == u ? sacc[u] : s;
        v.e_lds[pr0 + lane] = (v.sample((pr0 + lane) / T) < v.Bend) ? s : 0.f;
      }
    }
  }
  __syncthreads();
  // (3) softmax over t, one wave per row
  if (wave < v.nrows) {
    float* e = v.e_lds + wave * T;
    float m = -INFINITY;
    for (int t = lane; t < T; t += 64) m = fmaxf(m, e[t]);
    m = wave_max(m);
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) {
      const float x = expf(e[t] - m);
      e[t] = x;
      sum += x;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    const int b = v.sample(wave);
    for (int t = lane; t < T; t += 64) {
      const float a = e[t] * inv;
      e[t] = a;
      if (SAVES && p.alpha_out && b < v.Bend) p.alpha_out[((long)b * p.S + step) * T + t] = a;
    }
  }
  __syncthreads();
}

// (4), the kn columns from k0: ctx[row][k0 + c] = sum_t alpha[row][t] * Hb[b][t][k0 + c] into column c of the LDS tile (fp32 rows, or
// the fp16 hi / lo planes) and ctx_out.  The sums do not depend on the cut, so the chunked context equals the whole one bit for bit
template <bool X3, bool SAVES>
__device__ __forceinline__ void context_chunk(const AttnTile<X3>& v, const AttnDecParams& p, int step, int k0, int kn) {
  const int T = p.T, D = p.D, n4 = kn / 4;
  for (int it = v.t_; it < v.nrows * n4; it += NTH) {
    const int row = it / n4, c4 = it - row * n4;
    const int b = v.sample(row);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (b < v.Bend) {
      const float* hb = p.Hb + (long)b * T * D + k0 + c4 * 4;
      int t = 0;
#pragma unroll 1
      for (; t + 4 <= T; t += 4) {                 // four independent loads in flight per lane, 16 waves per CU (eight: no faster)
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4*>(hb + (long)(t + u) * D);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float w = v.e_lds[row * T + t + u];
#pragma unroll
          for (int k = 0; k < 4; ++k) a[k] = fmaf(w, x[u][k], a[k]);
        }
      }
      for (; t < T; ++t) {
        const float w = v.e_lds[row * T + t];
        const f32x4 x = *reinterpret_cast<const f32x4*>(hb + (long)t * D);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = fmaf(w, x[k], a[k]);
      }
    }
    if constexpr (X3) {
#pragma unroll
      for (int k = 0; k < 4; ++k) store_h_split(v.c_hi, v.c_lo, row * v.CLDH + c4 * 4 + k, a[k]);
    } else {
      *reinterpret_cast<f32x4*>(v.ctx_lds + row * v.CLD + c4 * 4) = a;
    }
    if (SAVES && p.ctx_out && b < v.Bend) *reinterpret_cast<f32x4*>(p.ctx_out + ((long)b * p.S + step) * D + k0 + c4 * 4) = a;
  }
}

// (4)-(6): acc5 is the caller's gate seed, c the lane's cell state (updated); h and the post-activation gates come back, h is in LDS for
// the next step.  The caller's stores and the barrier that publishes h follow
template <bool X3, bool WIDE, bool SAVES>
__device__ __forceinline__ void attn_cell(const AttnTile<X3>& v, const AttnDecParams& p, int step, const f32x4 (&acc5)[4], float (&c)[4],
                                          float (&h)[4], float (&act)[4][4]) {
  const int D = p.D, lane = v.lane, wave = v.wave;
  if constexpr (!WIDE) {
    context_chunk<X3, SAVES>(v, p, step, 0, D);
    __syncthreads();
  }
  f32x4 acc[4];
  const float pre_ih = 1.f / v.inv_ih;               // (a power of two)
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = acc5[g] * pre_ih;
  if constexpr (WIDE) {
    for (int k0 = 0; k0 < D; k0 += CTX_CHUNK) {
      const int kn = min(CTX_CHUNK, D - k0);
      context_chunk<X3, SAVES>(v, p, step, k0, kn);
      __syncthreads();
      if constexpr (X3) mma_rows_hb_k<4>(acc, v.c_hi, v.c_lo, v.r_ih, D, k0, kn, wave, lane, v.CLDH);
      else mma_rows_k<4>(acc, v.ctx_lds, v.CLD, p.w_ih, D, k0, kn, wave, lane);
      if (k0 + CTX_CHUNK < D) __syncthreads();   // every wave is done with this chunk before the next one lands
    }
  } else {
    if constexpr (X3) mma_rows_hb<4>(acc, v.c_hi, v.c_lo, v.r_ih, D, wave, lane, v.CLDH);
    else mma_rows<4>(acc, v.ctx_lds, v.CLD, p.w_ih, D, wave, lane);
  }
  if constexpr (X3) {
    const float ratio = v.inv_ih / v.inv_hh;            // (powers of two: exact)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] *= ratio;
    mma_rows_hb<4>(acc, v.h_hi, v.h_lo, v.r_hh, HID, wave, lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] *= v.inv_hh;
  } else {
    mma_rows<4>(acc, v.h_lds, HLD, p.w_hh, HID, wave, lane);
  }
  __syncthreads();  // every wave has finished reading h_lds
  lstm_pointwise0(acc, v.bh, c, h, act);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = v.rbase + r;
    const float hn = v.sample(row) < v.Bend ? h[r] : 0.f;
    if constexpr (X3) store_h_split(v.h_hi, v.h_lo, row * LDH + v.j, hn);
    else v.h_lds[row * HLD + v.j] = hn;
  }
}

// Teacher forced: the gate seed of a step is eproj[b][step]; stores hid, the optional training saves and the carried state.
template <bool X3, bool WIDE>
__global__ __launch_bounds__(NTH) void attn_decoder_kernel(const AttnDecGroup grp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // pinned == 1: one expert's recurrent weights (2.3 MiB) stay in one XCD's L2, all tiles of a group run on XCD (group % 8); pinned == 2
  // (six experts: 24 workgroups on every XCD instead of 32 on six of them; two experts' weights per L2 at most)
  int gi, tile_;
  group_tile(grp.groups, grp.tiles, grp.pinned, gi, tile_);
  if (gi >= grp.groups) return;
  const AttnDecParams& p = grp.g[gi];       // (read in place, as the other two kernels do: a copy costs the kernel 90 bytes of scratch per lane)
  // vb = samples per workgroup (2 ... 16, the fewest that keep the launch within 256 workgroups -- attn_launch: every step
  // re-reads the workgroup's Hproj / Hb slices (66 KB per sample each), so more, smaller workgroups shorten the step);
  // rows >= vb of the 16-row MFMA tile are treated like rows beyond the batch
  const AttnTile<X3> v = attn_tile<X3>(lds, p, WIDE ? CTX_CHUNK : p.D, tile_, grp.vb, 1);
  const int j = v.j;
  float c[4];
  float h[4] = {0.f, 0.f, 0.f, 0.f};        // h of the last step (the carried state, exact also when LDS holds the fp16 planes)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = v.b0 + v.rbase + r;
    c[r] = (p.c_state && b < v.Bend) ? p.c_state[(long)b * HID + j] : 0.f;
  }
  __syncthreads();

  for (int step = 0; step < p.S; ++step) {
    attn_scores<X3, true>(v, p, step);
    f32x4 acc5[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = v.b0 + v.rbase + r;
      const float* ep = p.eproj + (long)(b < v.Bend ? b : 0) * p.eproj_stride_b + (long)step * p.eproj_stride_s + j;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc5[g][r] = ep[g * HID];
    }
    float act[4][4];
    attn_cell<X3, WIDE, true>(v, p, step, acc5, c, h, act);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = v.b0 + v.rbase + r;
      if (b < v.Bend) {
        p.hid[(long)b * p.hid_stride_b + (long)step * p.hid_stride_s + j] = h[r];
        if (p.gates_out) {
          const long base = (long)b * p.S + step;
#pragma unroll
          for (int g = 0; g < 4; ++g) p.gates_out[base * 4 * HID + g * HID + j] = act[g][r];
          p.c_out[base * HID + j] = c[r];
        }
      }
    }
    __syncthreads();
  }

  if (p.h_state) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = v.b0 + v.rbase + r;
      if (b < v.Bend) {
        p.h_state[(long)b * HID + j] = h[r];
        p.c_state[(long)b * HID + j] = c[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Greedy decoding (reference modules/prediction.py:70-86), all S steps of all experts in one launch: the shared step with the token fed
// back inside the workgroup.  A workgroup's samples never need another workgroup's result, so this is a plain persistent loop with
// workgroup barriers only.  What it adds to the step:
//   (0) token: the caller's start token at step 0, then the previous step's argmax (LDS); a token >= num_class counts as 0
//       (Attention.cut_unknown).  The gate seed is row `token` of etab [num_class][4*HID] = char_embeddings.weight . W_ih[:, D:]^T + b_ih
//   (7) logits[b][step][:] = h . W_gen^T + b_gen (generator_tiles)
//   (8) argmax: a running best per lane over its tiles, shuffles over the 16 class columns, then the 16 waves through LDS; the
//       comparison of rowops.hip argmax_kernel (first index of the maximum, a NaN beats a number, an all-NaN row gives 0)
// ---------------------------------------------------------------------------------------------
struct GreedyParams {
  AttnDecParams a;                  // Hb, Hproj, the recurrent streams, w_inv (x3: float[4], the generator's last), B / T / D / S
  const float* etab;                // [num_class][4*HID]
  const int64_t* start;             // device: the start token
  const float* w_gen;               // fragment-major [ceil(num_class / 16)][1][K-steps][64 lanes] (fp32, or fp16 hi / lo in the x3 form)
  const float* b_gen;               // [num_class]
  float* logits;                    // [B][S][num_class], free row strides
  int64_t* tokens_out;              // optional [B][S]
  long logits_stride_b, logits_stride_s;
  int num_class;
};
struct GreedyGroup {
  GreedyParams g[MAX_GROUPS];
  int tiles, groups, pinned, vb;
};
constexpr int GREEDY_LDS_EXTRA = 4 * (BT + 2 * NW * BT);     // 16 tokens + 16 x 16 (value, index) pairs

__device__ __forceinline__ bool argmax_take(float ov, int oi, float best, int bi) {
  return (ov > best) || (ov == best && oi < bi) || (ov != ov && best == best);
}

// the generator on the new h, of the greedy and beam kernels: logits[row][cls] = h . W_gen^T + b_gen, class tile n (16 classes) belongs
// to wave n % 16, K = 256 comes from the h planes in LDS, W_gen is a one-gate-group fragment-major stream whose rows are zero-padded
// to a multiple of 16 (padded columns never reach the sink).  sink(r, cls, logit): row rbase + r of the lane's class
// (r_gen, inv_gen: the stream's buffer resource and inverse prescale, formed by the kernel once before its step loop -- formed here, the
// beam kernel ran 0.4-1 % slower at W = 4 and 8)
template <bool X3, class Sink>
__device__ __forceinline__ void generator_tiles(const AttnTile<X3>& v, const GreedyParams& gp, __amdgpu_buffer_rsrc_t r_gen, float inv_gen,
                                                Sink sink) {
  const int C = gp.num_class, ntile = (C + 15) / 16;
#pragma unroll 1
  for (int n = v.wave; n < ntile; n += NW) {
    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if constexpr (X3) mma_rows_hb<1>(acc, v.h_hi, v.h_lo, r_gen, HID, n, v.lane);
    // (exact form: the stream pointer is advanced to tile n and the helper's wave argument stays 0 -- every other caller passes a wave
    // index below 16, a range the compiler carries into the shared helper and that attn_decoder_kernel's register allocation rests on)
    else mma_rows<1>(acc, v.h_lds, HLD, gp.w_gen + (long)n * (HID / 16) * 256, HID, 0, v.lane);
    const int cls = n * 16 + v.col;
    if (cls < C) {
      const float bg = gp.b_gen[cls];
#pragma unroll
      for (int r = 0; r < 4; ++r) sink(r, cls, acc[0][r] * inv_gen + bg);
    }
  }
}

template <bool X3, bool WIDE>
__global__ __launch_bounds__(NTH) void attn_greedy_kernel(const GreedyGroup grp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int gi, tile_;
  group_tile(grp.groups, grp.tiles, grp.pinned, gi, tile_);
  if (gi >= grp.groups) return;
  const GreedyParams& gp = grp.g[gi];
  const AttnDecParams& p = gp.a;
  const int C = gp.num_class;
  const float inv_gen = X3 ? p.w_inv[3] : 1.f;     // the generator stream (x3: fp16 hi / lo behind a buffer resource) and its inverse prescale
  const __amdgpu_buffer_rsrc_t r_gen = make_rsrc(gp.w_gen, X3 ? (C + 15) / 16 * 16 * HID * 4 : 0);
  const AttnTile<X3> v = attn_tile<X3>(lds, p, WIDE ? CTX_CHUNK : p.D, tile_, grp.vb, 1);
  int* tok_lds = reinterpret_cast<int*>(v.sw_lds + HID);     // behind the shared map: [BT] tokens, [NW][BT] best values, [NW][BT] best indices
  float* red_v = reinterpret_cast<float*>(tok_lds + BT);
  int* red_i = reinterpret_cast<int*>(red_v + NW * BT);
  const int t_ = v.t_, wave = v.wave, rbase = v.rbase, j = v.j;
  if (t_ < BT) {
    const long k = gp.start[0];
    tok_lds[t_] = (k >= C || k < 0) ? 0 : (int)k;
  }
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  for (int step = 0; step < p.S; ++step) {
    attn_scores<X3, false>(v, p, step);
    // (0) the token's row of etab
    f32x4 acc5[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* ep = gp.etab + (long)tok_lds[rbase + r] * (4 * HID) + j;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc5[g][r] = ep[g * HID];
    }
    float h[4], act[4][4];
    attn_cell<X3, WIDE, false>(v, p, step, acc5, c, h, act);
    __syncthreads();
    // (7) generator on the new h, (8) running argmax of the lane's classes
    float best[4];
    int bi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      best[r] = -INFINITY;
      bi[r] = 0x7fffffff;
    }
    generator_tiles<X3>(v, gp, r_gen, inv_gen, [&](int r, int cls, float x) {
      const int b = v.b0 + rbase + r;
      if (b < v.Bend) gp.logits[(long)b * gp.logits_stride_b + (long)step * gp.logits_stride_s + cls] = x;
      if (x > best[r] || (x != x && best[r] == best[r])) {
        best[r] = x;
        bi[r] = cls;
      }
    });
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ov = __shfl_xor(best[r], o);
        const int oi = __shfl_xor(bi[r], o);
        if (argmax_take(ov, oi, best[r], bi[r])) {
          best[r] = ov;
          bi[r] = oi;
        }
      }
    }
    if (v.col == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red_v[wave * BT + rbase + r] = best[r];
        red_i[wave * BT + rbase + r] = bi[r];
      }
    }
    __syncthreads();
    if (t_ < BT) {                 // the next step reads tok_lds behind the barrier of its phase (1)
      float bv = red_v[t_];
      int bx = red_i[t_];
      for (int w = 1; w < NW; ++w) {
        const float ov = red_v[w * BT + t_];
        const int oi = red_i[w * BT + t_];
        if (argmax_take(ov, oi, bv, bx)) {
          bv = ov;
          bx = oi;
        }
      }
      if (bx >= C) bx = 0;
      tok_lds[t_] = bx;
      const int b = v.b0 + t_;
      if (gp.tokens_out && b < v.Bend) gp.tokens_out[(long)b * p.S + step] = bx;
    }
  }
}

// rows[i][:] = table[min-cut(idx[i])][:]   (Attention.cut_unknown: indices >= num_class map to 0)
__global__ void embed_gather_kernel(const long* __restrict__ idx, const float* __restrict__ table,
                                    float* __restrict__ out, long n, int E, int num_class, long idx_stride, int S) {
  const long i = blockIdx.x;
  if (i >= n) return;
  const long b = i / S, s = i - b * S;
  long k = idx[b * idx_stride + s];
  if (k >= num_class || k < 0) k = 0;
  for (int e = threadIdx.x; e < E; e += blockDim.x) out[i * E + e] = table[k * E + e];
}

// ---------------------------------------------------------------------------------------------
// Beam-search decoding on the attention head (extends reference modules/prediction.py:70-86; the algorithm is stated in
// mrn_amd/modules/decoding.py), all S steps of all experts in one launch.  The 16 MFMA rows of a workgroup are 16 / W samples x W
// entries: row r is entry r % W of sample b0 + r / W, rows of one sample read the same Hproj / Hb slices.  Per step:
//   (0)-(7) the shared step in its whole-context form on every row, with the greedy kernel's token feed and generator: a row's logits
//       are bit-identical to the greedy kernel's for the same token history; the logits go to the workgroup's scratch rows in global
//       memory (16 x C floats do not fit beside the tile in LDS), the new c of every row is staged in hp_lds, free since phase (2)
//   (8) wave r, row r: log-sum-exp of the row, then its W best classes by W scans (larger logit first, a tie to the lower class, a
//       NaN logit counts as -inf) -> candidates (score_r + logit - lse, class, logit - lse) in LDS; a finished row gives (score_r,
//       eos, 0) alone, a dead row nothing
//   (9) one thread per candidate ranks it among its sample's W x W (larger score first, ties in (row, class) order); rank q < W with
//       a score above -inf becomes entry q of the next step: (parent, token, logp) go to the step's history record, score / token /
//       finished to LDS
//   (10) every row takes its parent's h (LDS planes, read to registers before a barrier, written behind it) and c (hp_lds)
// The loop ends early once no row of the workgroup is live and unfinished (every later step would copy the entries as they are).
// Tail: one thread per row walks the history back from the last step and writes the outputs.
// ---------------------------------------------------------------------------------------------
struct BeamParams {
  GreedyParams g;                   // the greedy operands (logits / tokens_out unused)
  float* scratch;                   // [tiles][16][Cpad + 3 * S]: per workgroup 16 logit rows, then history parent / token / logp [S][16]
  int32_t* tokens;                  // [B][W][S]
  int32_t* length;                  // [B][W]
  float* score;                     // [B][W]
  float* logp;                      // [B][W][S]
  int64_t* path;                    // [B][S]
  float* prob;                      // [B][S]
};
struct BeamGroup {
  BeamParams g[MAX_GROUPS];
  int tiles, groups, pinned, W, eos;
};
constexpr int BEAM_LDS_EXTRA = 4 * (8 * BT + 3 * BT * BT);   // token, score, finished, four next-step rows, a flag row + 16 x 16 candidates (score, class, logp)

__device__ __forceinline__ bool beam_before(float va, int ia, float vb_, int ib) { return va > vb_ || (va == vb_ && ia < ib); }

// Lexicon-constrained beam search (attn_lexicon_kernel, include/mrn_attn_lexicon.h): the beam search walked along a trie of the
// lexicon, one trie for all experts of a launch.  Node 0 is the root; the children of node n are the edges child_off[n] ...
// child_off[n + 1] - 1 with class child_tok[e] and node child_node[e]; word_of[n] >= 0 where a word ends.  What differs from the beam:
//   a node id per row in LDS (0 at the start, the chosen child's in (10); a finished or dead row keeps its node)
//   (8) the log-sum-exp is over all C classes as before; the W best are taken among the row's ADMISSIBLE candidates only: the
//       children of its node whose class is inside the expert's C classes (the guard is the bounds check of the scratch row), and eos
//       where a word ends at the node.  Same order, same exclusion of the pairs already taken, same NaN rule; the child node travels
//       with (value, class) through the wave reduction into a fourth candidate plane
//   (9) also writes the next node; the tail also writes word [B][W] = word_of of the entry's node, -1 for a dead slot
// The host checks the arrays once per lexicon (ops.upload_trie): every child_node and every node id a row can hold is inside the arrays
struct LexTrie {
  const int32_t* child_off;         // [nodes + 1]
  const int32_t* child_tok;         // [nodes - 1]
  const int32_t* child_node;        // [nodes - 1]
  const int32_t* word_of;           // [nodes]
  int32_t* word[MAX_GROUPS];        // per group [B][W]
  int nodes;
};
constexpr int LEX_LDS_MORE = 4 * (2 * BT + BT * BT);         // the node row, its next-step twin and the candidate-node plane

// Shallow fusion of a character n-gram model into the beam search (attn_beam_lm_kernel, include/mrn_attn_lm.h; the algorithm is stated in
// mrn_amd/modules/decoding.py): the model of char_lm.hpp, one for all experts of a launch.  What differs from the beam:
//   per row in LDS the last two LM symbols (a << 16 | b, 0 at the start = begin of text), the LM sum, the length in characters and the
//       fused key the row was kept by
//   (8) an unfinished row proposes its N = n_prop best classes (N scans instead of W; W <= N <= 16); lane q < N keeps proposal q in
//       registers and evaluates the LM term of its own class (one lm_logp: at most three probes of at most max_probe slots each): eos
//       reads as the end of text (symbol 0), class 0 scores unk_logp flat; key = acoustic + alpha * (lm + term) + beta * len' goes to a
//       fourth candidate plane and lm + term to a fifth.  A finished row proposes itself with its key unchanged
//   (9) ranks the W x N proposals by the key plane and carries the acoustic value, class and logp as before, and the next context
//       (b, symbol), LM sum, length and key
//   (10) moves them with the parent; the tail also writes fused [B][W] = the key, -inf for a dead slot
// score and logp stay acoustic.  With alpha = beta = 0 the key is the acoustic value and, N >= W, the survivors are the beam's (unless
// rounding gives a proposal behind a row's W-th the very float of one in front of it and a lower class: the tie rule then takes it).
// The host checks the arrays once per model (ops.upload_char_lm); contexts and classes are below 65535 (beam_grouped)
struct BeamLMParams {
  CharLMTable m;
  float alpha, beta;
  int n_prop;
  float* fused[MAX_GROUPS];         // per group [B][W]
};
constexpr int LM_LDS_MORE = 4 * (8 * BT + 2 * BT * BT);       // context, LM sum, length, key, their next-step twins + the key and LM-sum planes

// the body of attn_beam_kernel (LEX = LM = false: `lex` and `lm` are not read), attn_lexicon_kernel (LEX = true) and attn_beam_lm_kernel
// (LM = true)
template <bool X3, bool LEX, bool LM = false>
__device__ __forceinline__ void attn_beam_body(const BeamGroup& grp, const LexTrie* lex, const BeamLMParams* lm = nullptr) {
  static_assert(!(LEX && LM), "no fusion in the trie decoder");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int gi, tile_;
  group_tile(grp.groups, grp.tiles, grp.pinned, gi, tile_);
  if (gi >= grp.groups) return;
  const BeamParams& bp = grp.g[gi];
  const GreedyParams& gp = bp.g;
  const AttnDecParams& p = gp.a;
  const int C = gp.num_class, S = p.S;
  const int W = grp.W, eos = grp.eos;
  const int CP = (C + 15) / 16 * 16;         // scratch row stride
  const float inv_gen = X3 ? p.w_inv[3] : 1.f;     // the generator stream (x3: fp16 hi / lo behind a buffer resource) and its inverse prescale
  const __amdgpu_buffer_rsrc_t r_gen = make_rsrc(gp.w_gen, X3 ? (C + 15) / 16 * 16 * HID * 4 : 0);
  const AttnTile<X3> v = attn_tile<X3>(lds, p, p.D, tile_, BT / W, W);       // 16 / W samples x W entries
  int* tok_lds = reinterpret_cast<int*>(v.sw_lds + HID);     // behind the shared map: the beam state of BEAM_LDS_EXTRA
  float* score_lds = reinterpret_cast<float*>(tok_lds + BT);
  int* fin_lds = reinterpret_cast<int*>(score_lds + BT);
  float* nsc = reinterpret_cast<float*>(fin_lds + BT);
  int* npar = reinterpret_cast<int*>(nsc + BT);
  int* ntok = npar + BT;
  float* nlp = reinterpret_cast<float*>(ntok + BT);
  int* flag_lds = reinterpret_cast<int*>(nlp + BT);
  float* cand_v = reinterpret_cast<float*>(flag_lds + BT);
  int* cand_c = reinterpret_cast<int*>(cand_v + BT * BT);
  float* cand_lp = reinterpret_cast<float*>(cand_c + BT * BT);
  int* node_lds = reinterpret_cast<int*>(cand_lp + BT * BT);      // LEX only: LEX_LDS_MORE
  int* nnode = node_lds + BT;
  int* cand_n = nnode + BT;
  int* ctx_lds = node_lds;                                        // LM only (never with LEX): LM_LDS_MORE
  float* lms_lds = reinterpret_cast<float*>(ctx_lds + BT);
  int* len_lds = reinterpret_cast<int*>(lms_lds + BT);
  float* key_lds = reinterpret_cast<float*>(len_lds + BT);
  int* nctx = reinterpret_cast<int*>(key_lds + BT);
  float* nlms = reinterpret_cast<float*>(nctx + BT);
  int* nlen = reinterpret_cast<int*>(nlms + BT);
  float* nkey = reinterpret_cast<float*>(nlen + BT);
  float* cand_k = nkey + BT;
  float* cand_lm = cand_k + BT * BT;
  const int NP = LM ? lm->n_prop : W;         // proposals of an unfinished row
  const int b0 = v.b0, Bend = v.Bend, nrows = v.nrows, t_ = v.t_, lane = v.lane, wave = v.wave, rbase = v.rbase, j = v.j;
  float* const row_scr = bp.scratch + (long)tile_ * BT * (CP + 3 * S);      // [16][CP]
  int* const hist_par = reinterpret_cast<int*>(row_scr + (long)BT * CP);   // [S][16]
  int* const hist_tok = hist_par + (long)S * BT;
  float* const hist_lp = reinterpret_cast<float*>(hist_tok + (long)S * BT);

  if (t_ < BT) {
    const long k = gp.start[0];
    tok_lds[t_] = (k >= C || k < 0) ? 0 : (int)k;
    score_lds[t_] = (t_ < nrows && t_ % W == 0 && b0 + t_ / W < Bend) ? 0.f : -INFINITY;      // one live entry per sample
    fin_lds[t_] = 0;
    if constexpr (LEX) node_lds[t_] = 0;
    if constexpr (LM) {
      ctx_lds[t_] = 0;
      lms_lds[t_] = 0.f;
      len_lds[t_] = 0;
      key_lds[t_] = score_lds[t_];
    }
  }
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  int nst = 0;                               // steps run
  for (int step = 0; step < S; ++step) {
    attn_scores<X3, false>(v, p, step);
    // (0) the token's row of etab
    f32x4 acc5[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* ep = gp.etab + (long)tok_lds[rbase + r] * (4 * HID) + j;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc5[g][r] = ep[g * HID];
    }
    float h[4], act[4][4];
    attn_cell<X3, false, false>(v, p, step, acc5, c, h, act);
#pragma unroll
    for (int r = 0; r < 4; ++r) v.hp_lds[(rbase + r) * HLD + j] = c[r];      // staged for (10)
    __syncthreads();
    // (7) generator on the new h -> the workgroup's scratch rows
    generator_tiles<X3>(v, gp, r_gen, inv_gen, [&](int r, int cls, float x) { row_scr[(long)(rbase + r) * CP + cls] = x; });
    __syncthreads();
    // (8) row `wave`: log-sum-exp and the W best classes
    {
      const int row = wave;
      const float sc = score_lds[row];
      const bool live = row < nrows && b0 + row / W < Bend && sc > -INFINITY;
      if (lane < NP) {
        cand_v[row * BT + lane] = -INFINITY;
        cand_c[row * BT + lane] = 0x7fffffff;
        cand_lp[row * BT + lane] = 0.f;
        if constexpr (LEX) cand_n[row * BT + lane] = 0;
        if constexpr (LM) {
          cand_k[row * BT + lane] = -INFINITY;
          cand_lm[row * BT + lane] = 0.f;
        }
      }
      const int node = LEX ? node_lds[row] : 0;
      const int ctx = LM ? ctx_lds[row] : 0;  // LM: the row's context, LM sum and length
      const float lms = LM ? lms_lds[row] : 0.f;
      const int len = LM ? len_lds[row] : 0;
      if (lane == 0) {                       // the next step's row, dead until (9) fills it
        nsc[row] = -INFINITY;
        npar[row] = row;
        ntok[row] = eos;
        nlp[row] = 0.f;
        if constexpr (LEX) nnode[row] = node;
        if constexpr (LM) {
          nctx[row] = ctx;
          nlms[row] = lms;
          nlen[row] = len;
          nkey[row] = -INFINITY;
        }
      }
      if (live && fin_lds[row]) {
        if (lane == 0) {
          cand_v[row * BT] = sc;
          cand_c[row * BT] = eos;
          if constexpr (LEX) cand_n[row * BT] = node;
          if constexpr (LM) {                // its key already holds the end-of-text term
            cand_k[row * BT] = key_lds[row];
            cand_lm[row * BT] = lms;
          }
        }
      } else if (live) {
        const float* x = row_scr + (long)row * CP;
        float m = -INFINITY;
        for (int k = lane; k < C; k += 64) {
          const float v = x[k];
          m = fmaxf(m, v == v ? v : -INFINITY);
        }
        m = wave_max(m);
        float sum = 0.f;
        for (int k = lane; k < C; k += 64) {
          const float v = x[k];
          sum += v == v ? expf(v - m) : 0.f;
        }
        sum = wave_sum(sum);
        const float lse = m + logf(sum);
        float pv = INFINITY;
        int pc = -1;
        int e0 = 0, e1 = 0;                   // LEX: the node's edges, and whether a word ends here
        bool ends = false;
        if constexpr (LEX) {
          e0 = lex->child_off[node];
          e1 = lex->child_off[node + 1];
          ends = lex->word_of[node] >= 0;
        }
        float mv = -INFINITY;                 // LM: proposal `lane` of the row, kept by its lane
        int mc = 0x7fffffff;
        for (int q = 0; q < NP; ++q) {
          float bv = -INFINITY;
          int bc = 0x7fffffff;
          int bn = 0;
          if constexpr (LEX) {
            for (int e = e0 + lane; e < e1; e += 64) {
              const int k = lex->child_tok[e];
              if (k < 0 || k >= C) continue;          // a class this expert does not have: outside its scratch row
              float v = x[k];
              v = v == v ? v : -INFINITY;
              if ((v < pv || (v == pv && k > pc)) && beam_before(v, k, bv, bc)) {
                bv = v;
                bc = k;
                bn = lex->child_node[e];
              }
            }
            if (ends && lane == 0) {                  // the one virtual candidate: the word ends, the entry stays at its node
              float v = x[eos];
              v = v == v ? v : -INFINITY;
              if ((v < pv || (v == pv && eos > pc)) && beam_before(v, eos, bv, bc)) {
                bv = v;
                bc = eos;
                bn = node;
              }
            }
          } else {
            for (int k = lane; k < C; k += 64) {
              float v = x[k];
              v = v == v ? v : -INFINITY;
              if ((v < pv || (v == pv && k > pc)) && beam_before(v, k, bv, bc)) {
                bv = v;
                bc = k;
              }
            }
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oc = __shfl_xor(bc, o);
            const int on = LEX ? __shfl_xor(bn, o) : 0;
            if (beam_before(ov, oc, bv, bc)) {
              bv = ov;
              bc = oc;
              bn = on;
            }
          }
          if (bc >= C) break;                 // fewer than W classes
          if constexpr (LM) {
            if (lane == q) {
              mv = bv;
              mc = bc;
            }
          } else if (lane == 0) {
            const float lp = bv - lse;
            const float cv = sc + lp;
            cand_v[row * BT + q] = cv == cv ? cv : -INFINITY;
            cand_c[row * BT + q] = bc;
            cand_lp[row * BT + q] = lp;
            if constexpr (LEX) cand_n[row * BT + q] = bn;
          }
          pv = bv;
          pc = bc;
        }
        if constexpr (LM) {
          if (mc < C) {                       // (lanes < NP that found a class)
            const int a = (int)((unsigned)ctx >> 16), b = ctx & 0xffff;      // (classes up to 65534: the shift is unsigned)
            const float term = mc == eos ? lm_logp(lm->m, a, b, 0) : mc == 0 ? lm->m.unk_logp : lm_logp(lm->m, a, b, mc);
            const float lp = mv - lse;
            float cv = sc + lp;
            cv = cv == cv ? cv : -INFINITY;
            const float nl = lms + term;
            const float key = cv + lm->alpha * nl + lm->beta * (float)(len + (mc == eos ? 0 : 1));
            cand_v[row * BT + lane] = cv;
            cand_c[row * BT + lane] = mc;
            cand_lp[row * BT + lane] = lp;
            cand_k[row * BT + lane] = key == key ? key : -INFINITY;
            cand_lm[row * BT + lane] = nl;
          }
        }
      }
    }
    __syncthreads();
    // (9) rank every candidate among its sample's
    if (t_ < BT * BT) {
      const int row = t_ >> 4, q = t_ & 15;
      const float* cand_r = LM ? cand_k : cand_v;      // the plane the candidates are ranked by
      if (row < nrows && q < NP) {
        const float v = cand_r[t_];
        if (v > -INFINITY) {
          const int cc = cand_c[t_];
          const int r0 = (row / W) * W;
          int rank = 0;
          for (int i = r0; i < r0 + W; ++i)
            for (int k = 0; k < NP; ++k) {
              const float ov = cand_r[i * BT + k];
              const int oc = cand_c[i * BT + k];
              rank += (ov > v || (ov == v && (i < row || (i == row && oc < cc)))) ? 1 : 0;
            }
          if (rank < W) {
            nsc[r0 + rank] = LM ? cand_v[t_] : v;
            npar[r0 + rank] = row;
            ntok[r0 + rank] = cc;
            nlp[r0 + rank] = cand_lp[t_];
            if constexpr (LEX) nnode[r0 + rank] = cand_n[t_];
            if constexpr (LM) {
              nkey[r0 + rank] = v;
              nlms[r0 + rank] = cand_lm[t_];
              const bool fin = fin_lds[row] != 0;      // a finished parent keeps its context and length
              const int pctx = ctx_lds[row];
              nctx[r0 + rank] = fin ? pctx : (int)(((unsigned)pctx & 0xffffu) << 16 | (unsigned)(cc == eos ? 0 : cc));
              nlen[r0 + rank] = len_lds[row] + (!fin && cc != eos ? 1 : 0);
            }
          }
        }
      }
    }
    __syncthreads();
    // (10) every row takes its parent's state; the step's history record
    float hf[4];
    _Float16 hh[4], hl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int par = npar[rbase + r];
      c[r] = v.hp_lds[par * HLD + j];
      if constexpr (X3) {
        hh[r] = v.h_hi[par * LDH + j];
        hl[r] = v.h_lo[par * LDH + j];
      } else {
        hf[r] = v.h_lds[par * HLD + j];
      }
    }
    if (t_ < BT) {
      const float v = nsc[t_];
      const int tk = ntok[t_];
      hist_par[step * BT + t_] = npar[t_];
      hist_tok[step * BT + t_] = tk;
      hist_lp[step * BT + t_] = nlp[t_];
      score_lds[t_] = v;
      tok_lds[t_] = tk;
      fin_lds[t_] = tk == eos ? 1 : 0;
      if constexpr (LEX) node_lds[t_] = nnode[t_];
      if constexpr (LM) {
        ctx_lds[t_] = nctx[t_];
        lms_lds[t_] = nlms[t_];
        len_lds[t_] = nlen[t_];
        key_lds[t_] = nkey[t_];
      }
      const unsigned long long open = __ballot(v > -INFINITY && tk != eos);    // (threads 0 ... 15: one wave)
      if (t_ == 0) flag_lds[0] = (open & 0xffffull) != 0 ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + r;
      if constexpr (X3) {
        v.h_hi[row * LDH + j] = hh[r];
        v.h_lo[row * LDH + j] = hl[r];
      } else {
        v.h_lds[row * HLD + j] = hf[r];
      }
    }
    const int go_on = flag_lds[0];
    nst = step + 1;
    __syncthreads();
    if (!go_on) break;
  }

  // tail: walk the history back from the last step run; behind it (an early stop: every live entry is finished) the fill
  if (t_ < BT) {
    const int row = t_, b = b0 + row / W, q = row % W;
    if (row < nrows && b < Bend) {
      const float sc = score_lds[row];
      const bool live = sc > -INFINITY;
      int32_t* tk = bp.tokens + ((long)b * W + q) * S;
      float* lp = bp.logp + ((long)b * W + q) * S;
      int first = S;                          // step of the first eos
      int cur = row;
      for (int s = S - 1; s >= 0; --s) {
        int tok = eos;
        float l = 0.f;
        if (live && s < nst) {
          tok = hist_tok[s * BT + cur];
          l = hist_lp[s * BT + cur];
          cur = hist_par[s * BT + cur];
          if (tok == eos) first = s;
        }
        tk[s] = tok;
        lp[s] = l;
        if (q == 0) {
          bp.path[(long)b * S + s] = tok;
          bp.prob[(long)b * S + s] = expf(l);
        }
      }
      bp.length[(long)b * W + q] = live ? (first < S ? first + 1 : S) : -1;
      bp.score[(long)b * W + q] = live ? sc : -INFINITY;
      if constexpr (LEX) lex->word[gi][(long)b * W + q] = live ? lex->word_of[node_lds[row]] : -1;
      if constexpr (LM) lm->fused[gi][(long)b * W + q] = live ? key_lds[row] : -INFINITY;
    }
  }
}

template <bool X3>
__global__ __launch_bounds__(NTH) void attn_beam_kernel(const BeamGroup grp) {
  attn_beam_body<X3, false>(grp, nullptr);
}

template <bool X3>
__global__ __launch_bounds__(NTH) void attn_lexicon_kernel(const BeamGroup grp, const LexTrie lex) {
  attn_beam_body<X3, true>(grp, &lex);
}

template <bool X3>
__global__ __launch_bounds__(NTH) void attn_beam_lm_kernel(const BeamGroup grp, const BeamLMParams lm) {
  attn_beam_body<X3, false, true>(grp, nullptr, &lm);
}

// ---------------------------------------------------------------------------------------------
// Exact scoring of per-sample candidate words on the attention head (attn_score_kernel, include/mrn_attn_score.h; the algorithm is
// stated in mrn_amd/modules/decoding.py): score[b][k] = log p(word, eos | sample b) of word cand[b][k], every (sample, slot) pair a
// teacher-forced roll-out of its own, all steps of all experts in one launch.  The 16 MFMA rows of a workgroup are 16 / per samples x
// per slots (per = the smallest of 1, 2, 4, 8, 16 that is >= K; K > 16: one sample per workgroup, ceil(K / 16) workgroups per sample):
// row r is slot k0 + r % per of sample b0 + r / per, rows of one sample read the same Hproj / Hb slices.  Per step:
//   (0)-(7) the shared step in its whole-context form with the greedy kernel's token feed and generator: the row's input is the start
//       token, then the word's classes; a row's logits are bit-identical to the greedy kernel's for the same token history
//   (8) the generator's sink keeps, per lane and row, a running (max, sum of exp) over the lane's classes (a NaN logit counts as -inf)
//       and hands the logit of the row's target class (the word's next class, eos behind the last) to LDS; the pairs are merged over
//       the 16 class columns by shuffles, then over the 16 waves through LDS in wave order -- one order of operations for every row,
//       so the same (sample, word) gives the same bits in any slot.  No logits are written
//   (9) thread r, row r: lp = target logit - (max + log sum); added to the row's score (and stored to logp) while step <= the word's
//       length, then the next step's input and target
// The loop runs to the longest word of the workgroup's rows.  A slot is dead (score -inf, logp 0) when it is unused (-1), when a class
// of its word is not below the expert's num_class, or when its score is -inf or NaN.  Lengths are clamped to min(Lmax, S - 1) and a
// word index outside the table counts as unused, so no read or write leaves the arrays whatever the tables hold
// ---------------------------------------------------------------------------------------------
struct ScoreParams {
  GreedyParams g;                   // the greedy operands (logits / tokens_out unused)
  float* score_all;                 // [B][K]
  float* logp;                      // optional [B][K][S]
};
struct ScoreGroup {
  ScoreParams g[MAX_GROUPS];
  const int32_t* lex_tokens;        // [N][Lmax]
  const int32_t* lex_len;           // [N]
  const int32_t* cand;              // [B][K]
  int tiles, groups, pinned, per, nblk, K, N, Lmax, eos;
};
constexpr int SCORE_LDS_EXTRA = 4 * (5 * BT + 2 * NW * BT);  // word, length, input token, target, target logit + 16 x 16 (max, sum) pairs

// (m, s) <- the log-sum-exp pair of both: s = sum of exp(x - m) over the classes seen; an empty pair is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  s = M > -INFINITY ? s * expf(m - M) + os * expf(om - M) : 0.f;
  m = M;
}

template <bool X3>
__global__ __launch_bounds__(NTH) void attn_score_kernel(const ScoreGroup grp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int gi, tile_;
  group_tile(grp.groups, grp.tiles, grp.pinned, gi, tile_);
  if (gi >= grp.groups) return;
  const ScoreParams& sp = grp.g[gi];
  const GreedyParams& gp = sp.g;
  const AttnDecParams& p = gp.a;
  const int C = gp.num_class, S = p.S, K = grp.K, per = grp.per, eos = grp.eos, Lmax = grp.Lmax;
  const int k0 = (tile_ % grp.nblk) * BT;          // the first slot of this workgroup (K > 16: nblk workgroups per sample)
  const float inv_gen = X3 ? p.w_inv[3] : 1.f;     // the generator stream (x3: fp16 hi / lo behind a buffer resource) and its inverse prescale
  const __amdgpu_buffer_rsrc_t r_gen = make_rsrc(gp.w_gen, X3 ? (C + 15) / 16 * 16 * HID * 4 : 0);
  const AttnTile<X3> v = attn_tile<X3>(lds, p, p.D, tile_ / grp.nblk, BT / per, per);
  int* word_lds = reinterpret_cast<int*>(v.sw_lds + HID);    // behind the shared map: the row state of SCORE_LDS_EXTRA
  int* wlen_lds = word_lds + BT;
  int* tok_lds = wlen_lds + BT;
  int* tgt_lds = tok_lds + BT;
  float* tl_lds = reinterpret_cast<float*>(tgt_lds + BT);
  float* red_m = tl_lds + BT;
  float* red_s = red_m + NW * BT;
  const int t_ = v.t_, lane = v.lane, wave = v.wave, rbase = v.rbase, j = v.j;

  // wave r, row r: its word, and whether this expert can spell it
  {
    const int row = wave, b = v.sample(row), slot = k0 + row % per;
    const bool mine = row < v.nrows && b < v.Bend && slot < K;
    int w = mine ? grp.cand[(long)b * K + slot] : -1;
    if (w >= grp.N) w = -1;
    int L = -1;
    if (w >= 0) {
      L = min(max(grp.lex_len[w], 0), min(Lmax, S - 1));
      int bad = 0;
      for (int i = lane; i < L; i += 64) {
        const int cl = grp.lex_tokens[(long)w * Lmax + i];
        bad |= (cl < 0 || cl >= C) ? 1 : 0;
      }
      if (__any(bad)) L = -1;
    }
    if (lane == 0) {
      const long k = gp.start[0];
      word_lds[row] = w;
      wlen_lds[row] = L;
      tok_lds[row] = (k >= C || k < 0) ? 0 : (int)k;
      tgt_lds[row] = L > 0 ? grp.lex_tokens[(long)w * Lmax] : eos;
      tl_lds[row] = 0.f;
    }
    if (sp.logp && mine) {                       // 0 past the word's end (a dead slot: everywhere)
      float* lp = sp.logp + ((long)b * K + slot) * S;
      for (int s = L + 1 + lane; s < S; s += 64) lp[s] = 0.f;
    }
  }
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  int nsteps = 0;                                // the longest word of the workgroup's rows and its eos
  for (int r = 0; r < BT; ++r) nsteps = max(nsteps, wlen_lds[r] + 1);
  const int row_ = t_ < BT ? t_ : 0;             // thread r < 16 owns row r's score
  const int myL = wlen_lds[row_];
  const int32_t* const mytok = grp.lex_tokens + (long)max(word_lds[row_], 0) * Lmax;
  const int myb = v.sample(row_), myslot = k0 + row_ % per;
  const bool mine = t_ < BT && row_ < v.nrows && myb < v.Bend && myslot < K;
  float* const mylp = (sp.logp && mine) ? sp.logp + ((long)myb * K + myslot) * S : nullptr;
  float total = 0.f;

  for (int step = 0; step < nsteps; ++step) {
    attn_scores<X3, false>(v, p, step);
    // (0) the token's row of etab
    f32x4 acc5[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* ep = gp.etab + (long)tok_lds[rbase + r] * (4 * HID) + j;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc5[g][r] = ep[g * HID];
    }
    float h[4], act[4][4];
    attn_cell<X3, false, false>(v, p, step, acc5, c, h, act);
    __syncthreads();
    // (7) generator on the new h, (8) running (max, sum) of the lane's classes and the target's logit
    int tg[4];
    float m[4], s[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      tg[r] = tgt_lds[rbase + r];
      m[r] = -INFINITY;
      s[r] = 0.f;
    }
    generator_tiles<X3>(v, gp, r_gen, inv_gen, [&](int r, int cls, float x) {
      x = x == x ? x : -INFINITY;
      if (cls == tg[r]) tl_lds[rbase + r] = x;
      if (x > m[r]) {
        s[r] = s[r] * expf(m[r] - x) + 1.f;
        m[r] = x;
      } else if (x > -INFINITY) {
        s[r] += expf(x - m[r]);
      }
    });
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float om = __shfl_xor(m[r], o);
        const float os = __shfl_xor(s[r], o);
        lse_merge(m[r], s[r], om, os);
      }
    }
    if (v.col == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red_m[wave * BT + rbase + r] = m[r];
        red_s[wave * BT + rbase + r] = s[r];
      }
    }
    __syncthreads();
    if (t_ < BT) {                 // (9); the next step reads tok_lds and tgt_lds behind the barriers of its phases (1)-(3)
      float M = red_m[t_], sum = red_s[t_];
      for (int w = 1; w < NW; ++w) lse_merge(M, sum, red_m[w * BT + t_], red_s[w * BT + t_]);
      const float lp = tl_lds[t_] - (M + logf(sum));
      if (step <= myL) {
        total += lp;
        if (mylp) mylp[step] = lp;
      }
      tok_lds[t_] = step < myL ? mytok[step] : eos;
      tgt_lds[t_] = step + 1 < myL ? mytok[step + 1] : eos;
    }
  }

  if (mine) {
    const bool live = myL >= 0 && total == total && total > -INFINITY;
    sp.score_all[(long)myb * K + myslot] = live ? total : -INFINITY;
    if (!live && mylp)
      for (int s = 0; s <= myL; ++s) mylp[s] = 0.f;
  }
}

}  // namespace

// ---- launch rules of the three attention decoder kernels ------------------------------------------------------
// LDS bytes of AttnTile's map for dc context columns and T frames plus the launching kernel's own arrays.  ops._attn_tile_lds restates
// the sum for the four ops.attn_*_whole_context rules
static size_t attn_tile_lds(bool x3, int dc, int T, size_t extra) {
  return sizeof(float) * (2 * BT * HLD + BT * (dc + 4) + BT * T + HID) + (x3 ? 1024 : 0) + extra;
}

// the placement of groups x tiles workgroups (recurrent.hpp: group_grid): the three decoder kernels pin from two experts
static dim3 attn_grid(int groups, int tiles, bool balance, int& pinned) { return group_grid(groups, tiles, 2, balance, pinned); }

// samples per workgroup: the fewest (from two) that keep the launch within one workgroup per CU
static int attn_vb(int groups, int B) {
  for (int v = 2; v < BT; v *= 2)
    if ((long)groups * ceil_div(B, v) <= 256) return v;
  return BT;
}

template <class Kernel, class Group>
static void attn_kernel_launch(Kernel kernel, const Group& grp, dim3 grid, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, grid, dim3(NTH), lds, st, grp);
}
#define MRN_ATTN_FORM(kernel, x3, wide) \
  ((x3) ? ((wide) ? kernel<true, true> : kernel<true, false>) : ((wide) ? kernel<false, true> : kernel<false, false>))

static int attn_launch(AttnDecGroup& grp, int groups, int D, int T, hipStream_t st) {
  grp.groups = groups;
  const int B = grp.g[0].B;
  // attn_vb: the step is a chain of dependent phases whose length grows with the samples a workgroup walks through (B = 256, one expert,
  // us per launch: 1100 at 1, 1130 at 2, 1315 at 4, 1700 at 8, 2580 at 16 -- tools/bench_decoder.py with MRN_ATTN_VB), and a second round
  // of workgroups doubles it (three experts: 2330 at 2, 1380 at 4).  Not one: a trained network's launch then fills the chip, and the DER
  // step, which runs its two heads' decoders side by side, loses 3 % (loop A gains 1.5 %: tools/probe/vb_sweep.sh)
  grp.vb = attn_vb(groups, B);
  static const int forced_vb = getenv("MRN_ATTN_VB") ? atoi(getenv("MRN_ATTN_VB")) : 0;     // (A/B switch, read once)
  if (forced_vb == 1 || forced_vb == 2 || forced_vb == 4 || forced_vb == 8 || forced_vb == 16) grp.vb = forced_vb;
  grp.tiles = ceil_div(B, grp.vb);
  static const bool balance = !(getenv("MRN_ATTN_BALANCE") && atoi(getenv("MRN_ATTN_BALANCE")) == 0);     // (A/B switch, read once)
  const dim3 grid = attn_grid(groups, grp.tiles, balance, grp.pinned);
  const bool x3 = grp.g[0].w_inv != nullptr;
  // the single-launch form holds the tile's whole context (BT x (D + 4) floats) in LDS; where that breaks the 160 KB budget (D = 256 * G,
  // G >= 8 at T = 65) the WIDE form holds CTX_CHUNK columns of it at a time.  MRN_ATTN_CTX_CHUNK=1 takes the WIDE form at any D (test
  // switch, read per launch)
  const char* force = getenv("MRN_ATTN_CTX_CHUNK");
  const bool wide = attn_tile_lds(x3, D, T, 0) > 160 * 1024 || (force && atoi(force) == 1);
  const size_t lds = attn_tile_lds(x3, wide ? CTX_CHUNK : D, T, 0);
  MRN_CHECK_ARG(lds <= 160 * 1024, "mrn_attn_decoder_fwd: LDS budget exceeded (D=%d T=%d)", D, T);
  MRN_CHECK_ARG(!x3 || D % 32 == 0, "mrn_attn_decoder_fwd (x3): D=%d must be a multiple of 32", D);
  attn_kernel_launch(MRN_ATTN_FORM(attn_decoder_kernel, x3, wide), grp, grid, lds, st);
  MRN_LAUNCH_CHECK("attn_decoder");
  return MRN_OK;
}

// The four teacher-forced entry points: `groups` experts of identical geometry, one launch per MAX_GROUPS of them.  Every operand is a
// HOST array of `groups` device pointers (b_hh may be NULL); strides are shared.  x3 == false: w_inv is ignored.  The single-expert entry
// points (`single`) pass arrays of one and may give the carried state and the training saves
static int attn_decoder_fwd(const char* who, bool x3, bool single, const void* const* Hb, const void* const* Hproj,
                            const void* const* eproj, int64_t eproj_stride_b, int64_t eproj_stride_s, const void* const* w_h2h,
                            const void* const* b_h2h, const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                            const void* const* w_inv, const void* const* b_hh, const void* const* hid, int64_t hid_stride_b,
                            int64_t hid_stride_s, float* h_state, float* c_state, float* alpha_out, float* gates_out, float* c_out,
                            float* ctx_out, float* hp_out, int groups, int B, int T, int D, int S, int hidden, void* stream) {
  auto given = [&](int g) {
    return Hb[g] && Hproj[g] && eproj[g] && w_h2h[g] && b_h2h[g] && w_score[g] && w_ih_ctx[g] && w_hh[g] && (!x3 || w_inv[g]) && hid[g];
  };
  MRN_CHECK_ARG(Hb && Hproj && eproj && w_h2h && b_h2h && w_score && w_ih_ctx && w_hh && (!x3 || w_inv) && hid && groups >= 1 &&
                    (!single || given(0)), "%s: null operand", who);
  MRN_CHECK_ARG(hidden == HID, "%s: hidden=%d unsupported (library is built for %d)", who, hidden, HID);
  MRN_CHECK_ARG(D % (x3 ? 32 : 16) == 0 && D > 0, "%s: D=%d must be a multiple of %d", who, D, x3 ? 32 : 16);
  MRN_CHECK_ARG((h_state == nullptr) == (c_state == nullptr), "%s: h_state/c_state must come together", who);
  if (B == 0 || S == 0) return MRN_OK;
  MRN_CHECK_ARG(!gates_out || (c_out && ctx_out && hp_out && alpha_out), "%s: training saves must all be given", who);
  for (int g0 = 0; g0 < groups; g0 += MAX_GROUPS) {
    const int n = groups - g0 < MAX_GROUPS ? groups - g0 : MAX_GROUPS;
    AttnDecGroup grp;
    memset(&grp, 0, sizeof(grp));
    for (int i = 0; i < n; ++i) {
      const int g = g0 + i;
      MRN_CHECK_ARG(given(g), "%s: null operand in group %d", who, g);
      AttnDecParams& p = grp.g[i];
      p.Hb = (const float*)Hb[g]; p.Hproj = (const float*)Hproj[g]; p.eproj = (const float*)eproj[g];
      p.w_h2h = (const float*)w_h2h[g]; p.b_h2h = (const float*)b_h2h[g]; p.w_score = (const float*)w_score[g];
      p.w_ih = (const float*)w_ih_ctx[g]; p.w_hh = (const float*)w_hh[g]; p.b_hh = b_hh ? (const float*)b_hh[g] : nullptr;
      p.w_inv = x3 ? (const float*)w_inv[g] : nullptr;
      p.hid = (float*)hid[g];
      p.B = B; p.T = T; p.D = D; p.S = S;
      p.eproj_stride_b = eproj_stride_b; p.eproj_stride_s = eproj_stride_s;
      p.hid_stride_b = hid_stride_b; p.hid_stride_s = hid_stride_s;
      p.h_state = h_state; p.c_state = c_state;
      p.alpha_out = alpha_out; p.gates_out = gates_out; p.c_out = c_out; p.ctx_out = ctx_out; p.hp_out = hp_out;
    }
    const int rc = attn_launch(grp, n, D, T, (hipStream_t)stream);
    if (rc) return rc;
  }
  return MRN_OK;
}

MRN_EXPORT int mrn_attn_decoder_fwd_f32(const float* Hb, const float* Hproj, const float* eproj, int64_t eproj_stride_b,
                                        int64_t eproj_stride_s, const float* w_h2h, const float* b_h2h,
                                        const float* w_score, const float* w_ih_ctx, const float* w_hh,
                                        const float* b_hh, float* hid, int64_t hid_stride_b, int64_t hid_stride_s, float* h_state,
                                        float* c_state, float* alpha_out, float* gates_out, float* c_out, float* ctx_out,
                                        float* hp_out, int B, int T, int D, int S, int hidden, void* stream) {
  const void* const a[] = {Hb, Hproj, eproj, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, hid};
  return attn_decoder_fwd("mrn_attn_decoder_fwd_f32", false, true, a, a + 1, a + 2, eproj_stride_b, eproj_stride_s, a + 3, a + 4, a + 5,
                          a + 6, a + 7, nullptr, a + 8, a + 9, hid_stride_b, hid_stride_s, h_state, c_state, alpha_out, gates_out, c_out,
                          ctx_out, hp_out, 1, B, T, D, S, hidden, stream);
}

// Teacher-forced decoders of `groups` experts (identical geometry) in one launch.  Every pointer argument is a HOST
// array of `groups` device pointers; strides are shared.  No carried state / training saves.
MRN_EXPORT int mrn_attn_decoder_fwd_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* eproj,
                                                int64_t eproj_stride_b, int64_t eproj_stride_s, const void* const* w_h2h,
                                                const void* const* b_h2h, const void* const* w_score,
                                                const void* const* w_ih_ctx, const void* const* w_hh, const void* const* b_hh,
                                                const void* const* hid, int64_t hid_stride_b, int64_t hid_stride_s, int groups,
                                                int B, int T, int D, int S, int hidden, void* stream) {
  return attn_decoder_fwd("mrn_attn_decoder_fwd_grouped_f32", false, false, Hb, Hproj, eproj, eproj_stride_b, eproj_stride_s, w_h2h, b_h2h,
                          w_score, w_ih_ctx, w_hh, nullptr, b_hh, hid, hid_stride_b, hid_stride_s, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr, groups, B, T, D, S, hidden, stream);
}

// The same decoders with the three recurrent products as split-fp16 x3: w_h2h / w_ih_ctx / w_hh are the fragment-major fp16 hi / lo
// streams of ops.pack_fragment_major_h, w_inv a device float[3] = 1 / prescale of each (per group in the grouped form).  D % 32 == 0.
MRN_EXPORT int mrn_attn_decoder_fwd_x3(const float* Hb, const float* Hproj, const float* eproj, int64_t eproj_stride_b,
                                       int64_t eproj_stride_s, const void* w_h2h, const float* b_h2h, const float* w_score,
                                       const void* w_ih_ctx, const void* w_hh, const float* w_inv, const float* b_hh, float* hid,
                                       int64_t hid_stride_b, int64_t hid_stride_s, float* h_state, float* c_state, float* alpha_out,
                                       float* gates_out, float* c_out, float* ctx_out, float* hp_out, int B, int T, int D, int S,
                                       int hidden, void* stream) {
  const void* const a[] = {Hb, Hproj, eproj, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, hid};
  return attn_decoder_fwd("mrn_attn_decoder_fwd_x3", true, true, a, a + 1, a + 2, eproj_stride_b, eproj_stride_s, a + 3, a + 4, a + 5,
                          a + 6, a + 7, a + 8, a + 9, a + 10, hid_stride_b, hid_stride_s, h_state, c_state, alpha_out, gates_out, c_out,
                          ctx_out, hp_out, 1, B, T, D, S, hidden, stream);
}

MRN_EXPORT int mrn_attn_decoder_fwd_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* eproj,
                                               int64_t eproj_stride_b, int64_t eproj_stride_s, const void* const* w_h2h,
                                               const void* const* b_h2h, const void* const* w_score, const void* const* w_ih_ctx,
                                               const void* const* w_hh, const void* const* w_inv, const void* const* b_hh,
                                               const void* const* hid, int64_t hid_stride_b, int64_t hid_stride_s, int groups, int B,
                                               int T, int D, int S, int hidden, void* stream) {
  return attn_decoder_fwd("mrn_attn_decoder_fwd_x3_grouped", true, false, Hb, Hproj, eproj, eproj_stride_b, eproj_stride_s, w_h2h, b_h2h,
                          w_score, w_ih_ctx, w_hh, w_inv, b_hh, hid, hid_stride_b, hid_stride_s, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, groups, B, T, D, S, hidden, stream);
}

// ---- greedy decoding: attn_greedy_kernel ----------------------------------------------------------------
static int greedy_launch(GreedyGroup& grp, int groups, int D, int T, hipStream_t st) {
  grp.groups = groups;
  const int B = grp.g[0].a.B;
  // samples per workgroup: every workgroup streams its expert's whole generator every step (5.5 MB at 5374 classes) on top of its
  // samples' Hproj / Hb slices, so fewer, fuller workgroups cut that stream and lengthen the dependent chain.  Measured (B = 256, T = 65,
  // S = 26, ms per launch at 2 / 4 / 8 / 16 samples, tools/bench_greedy.py --vb-sweep): one expert of 2091 classes 1.93 / 2.14 / 2.53 /
  // 3.43, of 5374 classes 2.92 / 3.19 / 3.61 / 4.53, six experts 8.40 / 5.91 / 4.71 / 5.60 -- the chain wins until the launch no longer
  // fits one round of workgroups, so the rule is attn_launch's (attn_vb).  MRN_GREEDY_VB (2, 4, 8, 16; read per launch) overrides it for
  // tests and sweeps
  grp.vb = attn_vb(groups, B);
  const char* fvb = getenv("MRN_GREEDY_VB");
  if (fvb) {
    const int v = atoi(fvb);
    if (v == 2 || v == 4 || v == 8 || v == 16) grp.vb = v;
  }
  grp.tiles = ceil_div(B, grp.vb);
  const dim3 grid = attn_grid(groups, grp.tiles, true, grp.pinned);
  const bool x3 = grp.g[0].a.w_inv != nullptr;
  // the WIDE form wherever the whole-context tile with the tokens and the argmax pairs passes 160 KiB, or under MRN_ATTN_CTX_CHUNK=1
  // (read per launch).  ops.attn_greedy_whole_context restates the rule
  const char* force = getenv("MRN_ATTN_CTX_CHUNK");
  const bool wide = attn_tile_lds(x3, D, T, GREEDY_LDS_EXTRA) > 160 * 1024 || (force && atoi(force) == 1);
  const size_t lds = attn_tile_lds(x3, wide ? CTX_CHUNK : D, T, GREEDY_LDS_EXTRA);
  MRN_CHECK_ARG(lds <= 160 * 1024, "mrn_attn_greedy_decode: LDS budget exceeded (D=%d T=%d)", D, T);
  attn_kernel_launch(MRN_ATTN_FORM(attn_greedy_kernel, x3, wide), grp, grid, lds, st);
  MRN_LAUNCH_CHECK("attn_greedy");
  return MRN_OK;
}

// What the greedy, beam and lexicon entry points share, as it arrives: HOST arrays of `groups` device pointers (b_hh may be NULL or hold
// NULL entries; w_inv is read in the x3 form only), a class count per group, the shared start token and geometry
typedef const void* const* PtrArray;
struct DecodeOperands {
  PtrArray Hb, Hproj, etab;
  const int64_t* start_token;
  PtrArray w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, w_gen, b_gen;
  const int* num_class;
  int B, T, D, S;
};
static bool decode_arrays_given(const DecodeOperands& o, bool x3) {
  return o.Hb && o.Hproj && o.etab && o.start_token && o.w_h2h && o.b_h2h && o.w_score && o.w_ih_ctx && o.w_hh && (!x3 || o.w_inv) &&
         o.w_gen && o.b_gen && o.num_class;
}
static bool decode_group_given(const DecodeOperands& o, bool x3, int g) {
  return o.Hb[g] && o.Hproj[g] && o.etab[g] && o.w_h2h[g] && o.b_h2h[g] && o.w_score[g] && o.w_ih_ctx[g] && o.w_hh[g] &&
         (!x3 || o.w_inv[g]) && o.w_gen[g] && o.b_gen[g];
}

// group g's operands; the outputs (zero here) are the caller's
static void greedy_fill(GreedyParams& gp, const DecodeOperands& o, bool x3, int g) {
  memset(&gp, 0, sizeof(gp));
  AttnDecParams& p = gp.a;
  p.Hb = (const float*)o.Hb[g]; p.Hproj = (const float*)o.Hproj[g];
  p.w_h2h = (const float*)o.w_h2h[g]; p.b_h2h = (const float*)o.b_h2h[g]; p.w_score = (const float*)o.w_score[g];
  p.w_ih = (const float*)o.w_ih_ctx[g]; p.w_hh = (const float*)o.w_hh[g];
  p.w_inv = x3 ? (const float*)o.w_inv[g] : nullptr; p.b_hh = o.b_hh ? (const float*)o.b_hh[g] : nullptr;
  p.B = o.B; p.T = o.T; p.D = o.D; p.S = o.S;
  gp.etab = (const float*)o.etab[g]; gp.start = o.start_token;
  gp.w_gen = (const float*)o.w_gen[g]; gp.b_gen = (const float*)o.b_gen[g]; gp.num_class = o.num_class[g];
}

// The four greedy entry points: `groups` experts of identical geometry (B, T, D, S) and their own class counts in one launch (several
// beyond MAX_GROUPS).  logits and tokens_out are HOST arrays of `groups` device pointers, the two logits strides host arrays of `groups`
// values; tokens_out may be NULL.  The single-expert entry points (`single`) pass arrays of one
static int greedy_grouped(const char* who, bool x3, bool single, const DecodeOperands& o, PtrArray logits, const int64_t* logits_stride_b,
                          const int64_t* logits_stride_s, PtrArray tokens_out, int groups, int hidden, void* stream) {
  const int B = o.B, T = o.T, D = o.D, S = o.S;
  auto given = [&](int g) { return decode_group_given(o, x3, g) && logits[g]; };
  MRN_CHECK_ARG(decode_arrays_given(o, x3) && logits && logits_stride_b && logits_stride_s && groups >= 1 && (!single || given(0)),
                "%s: null operand", who);
  MRN_CHECK_ARG(hidden == HID, "%s: hidden=%d unsupported (library is built for %d)", who, hidden, HID);
  MRN_CHECK_ARG(D % (x3 ? 32 : 16) == 0 && D > 0, "%s: D=%d must be a multiple of %d", who, D, x3 ? 32 : 16);
  MRN_CHECK_ARG(B >= 0 && T > 0 && S >= 0, "%s: bad geometry (B=%d T=%d S=%d)", who, B, T, S);
  MRN_CHECK_ARG(!single || o.num_class[0] >= 1, "%s: num_class=%d", who, o.num_class[0]);
  if (B == 0 || S == 0) return MRN_OK;
  for (int g0 = 0; g0 < groups; g0 += MAX_GROUPS) {
    const int n = groups - g0 < MAX_GROUPS ? groups - g0 : MAX_GROUPS;
    GreedyGroup grp;
    memset(&grp, 0, sizeof(grp));
    for (int i = 0; i < n; ++i) {
      const int g = g0 + i;
      MRN_CHECK_ARG(given(g), "%s: null operand in group %d", who, g);
      MRN_CHECK_ARG(o.num_class[g] >= 1, "%s: num_class=%d in group %d", who, o.num_class[g], g);
      GreedyParams& gp = grp.g[i];
      greedy_fill(gp, o, x3, g);
      gp.logits = (float*)logits[g]; gp.logits_stride_b = logits_stride_b[g]; gp.logits_stride_s = logits_stride_s[g];
      gp.tokens_out = tokens_out ? (int64_t*)tokens_out[g] : nullptr;
    }
    const int rc = greedy_launch(grp, n, D, T, (hipStream_t)stream);
    if (rc) return rc;
  }
  return MRN_OK;
}

// Greedy decoding of one expert: S steps, argmax fed back inside the launch (reference modules/prediction.py:70-86).
MRN_EXPORT int mrn_attn_greedy_decode_f32(const float* Hb, const float* Hproj, const float* etab, const int64_t* start_token,
                                          const float* w_h2h, const float* b_h2h, const float* w_score, const float* w_ih_ctx,
                                          const float* w_hh, const float* b_hh, const float* w_gen, const float* b_gen, int num_class,
                                          float* logits, int64_t logits_stride_b, int64_t logits_stride_s, int64_t* tokens_out, int B,
                                          int T, int D, int S, int hidden, void* stream) {
  const void* const a[] = {Hb, Hproj, etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, b_hh, w_gen, b_gen, logits, tokens_out};
  const DecodeOperands o{a, a + 1, a + 2, start_token, a + 3, a + 4, a + 5, a + 6, a + 7, nullptr, a + 8, a + 9, a + 10, &num_class, B, T, D, S};
  return greedy_grouped("mrn_attn_greedy_decode_f32", false, true, o, a + 11, &logits_stride_b, &logits_stride_s, a + 12, 1, hidden, stream);
}

MRN_EXPORT int mrn_attn_greedy_decode_x3(const float* Hb, const float* Hproj, const float* etab, const int64_t* start_token,
                                         const void* w_h2h, const float* b_h2h, const float* w_score, const void* w_ih_ctx,
                                         const void* w_hh, const float* w_inv, const float* b_hh, const void* w_gen, const float* b_gen,
                                         int num_class, float* logits, int64_t logits_stride_b, int64_t logits_stride_s,
                                         int64_t* tokens_out, int B, int T, int D, int S, int hidden, void* stream) {
  const void* const a[] = {Hb, Hproj, etab, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, w_gen, b_gen, logits, tokens_out};
  const DecodeOperands o{a, a + 1, a + 2, start_token, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9, a + 10, a + 11, &num_class, B, T, D, S};
  return greedy_grouped("mrn_attn_greedy_decode_x3", true, true, o, a + 12, &logits_stride_b, &logits_stride_s, a + 13, 1, hidden, stream);
}

MRN_EXPORT int mrn_attn_greedy_decode_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                  const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                  const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                  const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                                  const int* num_class, const void* const* logits, const int64_t* logits_stride_b,
                                                  const int64_t* logits_stride_s, const void* const* tokens_out, int groups, int B, int T,
                                                  int D, int S, int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, nullptr, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  return greedy_grouped("mrn_attn_greedy_decode_grouped_f32", false, false, o, logits, logits_stride_b, logits_stride_s, tokens_out, groups,
                        hidden, stream);
}

MRN_EXPORT int mrn_attn_greedy_decode_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                 const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                 const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                 const void* const* w_inv, const void* const* b_hh, const void* const* w_gen,
                                                 const void* const* b_gen, const int* num_class, const void* const* logits,
                                                 const int64_t* logits_stride_b, const int64_t* logits_stride_s, const void* const* tokens_out,
                                                 int groups, int B, int T, int D, int S, int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  return greedy_grouped("mrn_attn_greedy_decode_x3_grouped", true, false, o, logits, logits_stride_b, logits_stride_s, tokens_out, groups,
                        hidden, stream);
}

MRN_EXPORT int mrn_embed_gather_f32(const int64_t* idx, int64_t idx_stride, const float* table, float* out, int B,
                                    int S, int E, int num_class, void* stream) {
  MRN_CHECK_ARG(idx && table && out, "mrn_embed_gather_f32: null operand");
  const long n = (long)B * S;
  if (n == 0) return MRN_OK;
  hipLaunchKernelGGL(embed_gather_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, (const long*)idx, table, out,
                     n, E, num_class, (long)idx_stride, S);
  MRN_LAUNCH_CHECK("embed_gather");
  return MRN_OK;
}

// ---- beam-search decoding on the attention head: attn_beam_kernel (include/mrn_attn_beam.h) ----------------
// the whole-context tile plus the beam state (BEAM_LDS_EXTRA); there is no chunked form.  lex: null, or the trie of attn_lexicon_kernel
// (include/mrn_attn_lexicon.h), whose node rows and candidate-node plane are LEX_LDS_MORE bytes on top; lm: null, or the model of
// attn_beam_lm_kernel (include/mrn_attn_lm.h), whose row state and two candidate planes are LM_LDS_MORE bytes on top (never both)
static int beam_launch(BeamGroup& grp, const LexTrie* lex, int groups, int D, int T, hipStream_t st, const BeamLMParams* lm = nullptr) {
  grp.groups = groups;
  const int B = grp.g[0].g.a.B;
  grp.tiles = ceil_div(B, BT / grp.W);       // 16 / W samples per workgroup
  const dim3 grid = attn_grid(groups, grp.tiles, true, grp.pinned);
  const bool x3 = grp.g[0].g.a.w_inv != nullptr;
  const size_t lds = attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA) + (lex ? LEX_LDS_MORE : 0) + (lm ? LM_LDS_MORE : 0);
  if (lm) {
    if (lds > 64 * 1024) {
      (void)hipFuncSetAttribute(x3 ? (const void*)attn_beam_lm_kernel<true> : (const void*)attn_beam_lm_kernel<false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    if (x3) hipLaunchKernelGGL(attn_beam_lm_kernel<true>, grid, dim3(NTH), lds, st, grp, *lm);
    else hipLaunchKernelGGL(attn_beam_lm_kernel<false>, grid, dim3(NTH), lds, st, grp, *lm);
    MRN_LAUNCH_CHECK("attn_beam_lm");
    return MRN_OK;
  }
  if (lex) {
    if (lds > 64 * 1024) {
      (void)hipFuncSetAttribute(x3 ? (const void*)attn_lexicon_kernel<true> : (const void*)attn_lexicon_kernel<false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    if (x3) hipLaunchKernelGGL(attn_lexicon_kernel<true>, grid, dim3(NTH), lds, st, grp, *lex);
    else hipLaunchKernelGGL(attn_lexicon_kernel<false>, grid, dim3(NTH), lds, st, grp, *lex);
    MRN_LAUNCH_CHECK("attn_lexicon");
    return MRN_OK;
  }
  if (x3) attn_kernel_launch(attn_beam_kernel<true>, grp, grid, lds, st);
  else attn_kernel_launch(attn_beam_kernel<false>, grp, grid, lds, st);
  MRN_LAUNCH_CHECK("attn_beam");
  return MRN_OK;
}

// the lexicon entry points' trie, as it arrives: four device arrays shared by the groups, a HOST array `word` of `groups` device pointers
struct LexOperands {
  const int32_t *child_off, *child_tok, *child_node, *word_of;
  int nodes, depth;
  PtrArray word;
};

// the fusion entry points' model, as it arrives: the operands of mrn_ctc_beam_lm_decode_f32 (device arrays shared by the groups), the
// proposals per row, a HOST array `fused` of `groups` device pointers
struct LMOperands {
  const void* keys;
  const float* vals;
  int64_t mask;
  int max_probe;
  const float *uni_logp, *uni_bow;
  int C_lm;
  float unk_logp;
  int order;
  float alpha, beta;
  int top_n;
  PtrArray fused;
};

// `groups` experts of identical geometry (B, T, D, S) and their own class counts in one launch per MAX_GROUPS experts.  Every limit is
// checked for every group before the first launch.  trie: null, or the lexicon of the two lexicon entry points; model: null, or the
// language model of the two fusion entry points
static int beam_grouped(const char* who, bool x3, const DecodeOperands& o, int eos, int W, PtrArray scratch, int64_t scratch_floats,
                        PtrArray tokens, PtrArray length, PtrArray score, PtrArray logp, PtrArray path, PtrArray prob, int groups,
                        int hidden, void* stream, const LexOperands* trie = nullptr, const LMOperands* model = nullptr) {
  const int B = o.B, T = o.T, D = o.D, S = o.S;
  MRN_CHECK_ARG(decode_arrays_given(o, x3) && scratch && tokens && length && score && logp && path && prob && groups >= 1,
                "%s: null operand", who);
  MRN_CHECK_ARG(hidden == HID, "%s: hidden=%d unsupported (library is built for %d)", who, hidden, HID);
  MRN_CHECK_ARG(W >= 1 && W <= BT, "%s: beam width W=%d outside 1 ... %d", who, W, BT);
  MRN_CHECK_ARG(S >= 1 && S <= 512, "%s: S=%d steps outside 1 ... 512", who, S);
  MRN_CHECK_ARG(D > 0 && D % (x3 ? 32 : 16) == 0, "%s: D=%d must be a multiple of %d", who, D, x3 ? 32 : 16);
  MRN_CHECK_ARG(B >= 0 && T > 0, "%s: bad geometry (B=%d T=%d)", who, B, T);
  MRN_CHECK_ARG(attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA) <= 160 * 1024, "%s: the whole context does not fit the LDS budget (D=%d T=%d)", who, D, T);
  if (trie) {
    const auto [child_off, child_tok, child_node, word_of, nodes, depth, word] = *trie;
    MRN_CHECK_ARG(attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA + LEX_LDS_MORE) <= 160 * 1024,
                  "%s: the whole context does not fit the LDS budget (D=%d T=%d)", who, D, T);
    MRN_CHECK_ARG(child_off && child_tok && child_node && word_of && word, "%s: null trie operand", who);
    MRN_CHECK_ARG(nodes >= 1, "%s: a trie of nodes=%d (at least the root)", who, nodes);
    MRN_CHECK_ARG(depth >= 0 && depth <= S - 1, "%s: trie depth=%d outside 0 ... S - 1 = %d (the longest word and its end token take S steps)", who, depth, S - 1);
    for (int g = 0; g < groups; ++g) MRN_CHECK_ARG(B == 0 || word[g], "%s: null operand in group %d", who, g);
  }
  if (model) {
    const LMOperands& m = *model;
    MRN_CHECK_ARG(attn_tile_lds(x3, D, T, BEAM_LDS_EXTRA + LM_LDS_MORE) <= 160 * 1024,
                  "%s: the whole context does not fit the LDS budget (D=%d T=%d)", who, D, T);
    MRN_CHECK_ARG(m.top_n >= 1 && m.top_n <= BT, "%s: top_n=%d outside 1 ... %d", who, m.top_n, BT);
    MRN_CHECK_ARG(m.order >= 1 && m.order <= 3, "%s: order %d outside 1 ... 3", who, m.order);
    MRN_CHECK_ARG(m.C_lm >= 1 && m.C_lm <= CHAR_LM_MAX_C, "%s: C_lm=%d outside 1 ... %d", who, m.C_lm, CHAR_LM_MAX_C);
    MRN_CHECK_ARG(m.mask >= 0 && m.mask < CHAR_LM_MAX_SLOTS && ((m.mask + 1) & m.mask) == 0,
                  "%s: table mask %ld is not a power of two up to 2^26 less one", who, (long)m.mask);
    MRN_CHECK_ARG(m.max_probe >= 0 && (int64_t)m.max_probe <= m.mask + 1, "%s: max_probe %d outside 0 ... %ld", who, m.max_probe,
                  (long)(m.mask + 1));
    MRN_CHECK_ARG(isfinite(m.unk_logp) && isfinite(m.alpha) && m.alpha >= 0.f && isfinite(m.beta),
                  "%s: unk_logp %g, alpha %g (>= 0) and beta %g must be finite", who, (double)m.unk_logp, (double)m.alpha, (double)m.beta);
    MRN_CHECK_ARG(m.keys && m.vals && m.uni_logp && m.uni_bow && m.fused, "%s: null model operand", who);
    for (int g = 0; g < groups; ++g) {
      MRN_CHECK_ARG(B == 0 || m.fused[g], "%s: null operand in group %d", who, g);
      MRN_CHECK_ARG(o.num_class[g] <= CHAR_LM_MAX_C, "%s: num_class=%d in group %d above %d (classes are 16-bit fields of a context)", who,
                    o.num_class[g], g, CHAR_LM_MAX_C);
    }
  }
  const long tiles = ceil_div(B, BT / W);
  for (int g = 0; g < groups; ++g) {
    MRN_CHECK_ARG(decode_group_given(o, x3, g) &&
                      (B == 0 || (scratch[g] && tokens[g] && length[g] && score[g] && logp[g] && path[g] && prob[g])),
                  "%s: null operand in group %d", who, g);
    MRN_CHECK_ARG(o.num_class[g] >= 2, "%s: num_class=%d in group %d (at least 2)", who, o.num_class[g], g);
    MRN_CHECK_ARG(eos >= 0 && eos < o.num_class[g], "%s: eos=%d outside the %d classes of group %d", who, eos, o.num_class[g], g);
    const long need = tiles * BT * ((long)ceil_div(o.num_class[g], 16) * 16 + 3L * S);
    MRN_CHECK_ARG(scratch_floats >= need, "%s: scratch of %ld floats, group %d needs %ld", who, (long)scratch_floats, g, need);
  }
  if (B == 0) return MRN_OK;
  for (int g0 = 0; g0 < groups; g0 += MAX_GROUPS) {
    const int n = groups - g0 < MAX_GROUPS ? groups - g0 : MAX_GROUPS;
    BeamGroup grp;
    memset(&grp, 0, sizeof(grp));
    grp.W = W;
    grp.eos = eos;
    for (int i = 0; i < n; ++i) {
      const int g = g0 + i;
      BeamParams& bp = grp.g[i];
      greedy_fill(bp.g, o, x3, g);
      bp.scratch = (float*)scratch[g];
      bp.tokens = (int32_t*)tokens[g];
      bp.length = (int32_t*)length[g];
      bp.score = (float*)score[g];
      bp.logp = (float*)logp[g];
      bp.path = (int64_t*)path[g];
      bp.prob = (float*)prob[g];
    }
    LexTrie lex;
    if (trie) {
      lex = LexTrie{trie->child_off, trie->child_tok, trie->child_node, trie->word_of, {}, trie->nodes};
      for (int i = 0; i < n; ++i) lex.word[i] = (int32_t*)trie->word[g0 + i];
    }
    BeamLMParams lm;
    if (model) {
      const LMOperands& m = *model;
      lm.m = CharLMTable{(const unsigned long long*)m.keys, (const float2*)m.vals, m.uni_logp, m.uni_bow, (unsigned)m.mask, m.max_probe,
                         m.C_lm, m.order, m.unk_logp};
      lm.alpha = m.alpha;
      lm.beta = m.beta;
      lm.n_prop = W > m.top_n ? W : m.top_n;          // N = min(16, max(W, top_n)): W and top_n are at most 16
      for (int i = 0; i < MAX_GROUPS; ++i) lm.fused[i] = i < n ? (float*)m.fused[g0 + i] : nullptr;
    }
    const int rc = beam_launch(grp, trie ? &lex : nullptr, n, D, T, (hipStream_t)stream, model ? &lm : nullptr);
    if (rc) return rc;
  }
  return MRN_OK;
}

MRN_EXPORT int mrn_attn_beam_decode_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                                const int* num_class, int eos, int W, const void* const* scratch, int64_t scratch_floats,
                                                const void* const* tokens, const void* const* length, const void* const* score,
                                                const void* const* logp, const void* const* path, const void* const* prob, int groups,
                                                int B, int T, int D, int S, int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, nullptr, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  return beam_grouped("mrn_attn_beam_decode_grouped_f32", false, o, eos, W, scratch, scratch_floats, tokens, length, score, logp, path, prob,
                      groups, hidden, stream);
}

MRN_EXPORT int mrn_attn_beam_decode_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                               const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                               const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                               const void* const* w_inv, const void* const* b_hh, const void* const* w_gen,
                                               const void* const* b_gen, const int* num_class, int eos, int W,
                                               const void* const* scratch, int64_t scratch_floats, const void* const* tokens,
                                               const void* const* length, const void* const* score, const void* const* logp,
                                               const void* const* path, const void* const* prob, int groups, int B, int T, int D, int S,
                                               int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  return beam_grouped("mrn_attn_beam_decode_x3_grouped", true, o, eos, W, scratch, scratch_floats, tokens, length, score, logp, path, prob,
                      groups, hidden, stream);
}

// ---- lexicon-constrained beam search on the attention head: attn_lexicon_kernel (include/mrn_attn_lexicon.h) ----
MRN_EXPORT int mrn_attn_lexicon_decode_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                   const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                   const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                   const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                                   const int* num_class, int eos, int W, const int32_t* child_off,
                                                   const int32_t* child_tok, const int32_t* child_node, const int32_t* word_of, int nodes,
                                                   int depth, const void* const* scratch, int64_t scratch_floats,
                                                   const void* const* tokens, const void* const* length, const void* const* score,
                                                   const void* const* logp, const void* const* path, const void* const* prob,
                                                   const void* const* word, int groups, int B, int T, int D, int S, int hidden,
                                                   void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, nullptr, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  const LexOperands trie{child_off, child_tok, child_node, word_of, nodes, depth, word};
  return beam_grouped("mrn_attn_lexicon_decode_grouped_f32", false, o, eos, W, scratch, scratch_floats, tokens, length, score, logp, path,
                      prob, groups, hidden, stream, &trie);
}

MRN_EXPORT int mrn_attn_lexicon_decode_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                  const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                  const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                  const void* const* w_inv, const void* const* b_hh, const void* const* w_gen,
                                                  const void* const* b_gen, const int* num_class, int eos, int W,
                                                  const int32_t* child_off, const int32_t* child_tok, const int32_t* child_node,
                                                  const int32_t* word_of, int nodes, int depth, const void* const* scratch,
                                                  int64_t scratch_floats, const void* const* tokens, const void* const* length,
                                                  const void* const* score, const void* const* logp, const void* const* path,
                                                  const void* const* prob, const void* const* word, int groups, int B, int T, int D, int S,
                                                  int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  const LexOperands trie{child_off, child_tok, child_node, word_of, nodes, depth, word};
  return beam_grouped("mrn_attn_lexicon_decode_x3_grouped", true, o, eos, W, scratch, scratch_floats, tokens, length, score, logp, path, prob,
                      groups, hidden, stream, &trie);
}

// ---- beam search with a character n-gram model on the attention head: attn_beam_lm_kernel (include/mrn_attn_lm.h) ----
MRN_EXPORT int mrn_attn_beam_lm_decode_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                   const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                   const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                   const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                                   const int* num_class, int eos, int W, int top_n, const void* lm_keys,
                                                   const float* lm_vals, int64_t lm_mask, int lm_max_probe, const float* uni_logp,
                                                   const float* uni_bow, int C_lm, float unk_logp, int order, float alpha, float beta,
                                                   const void* const* scratch, int64_t scratch_floats, const void* const* tokens,
                                                   const void* const* length, const void* const* score, const void* const* logp,
                                                   const void* const* path, const void* const* prob, const void* const* fused, int groups,
                                                   int B, int T, int D, int S, int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, nullptr, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  const LMOperands model{lm_keys, lm_vals, lm_mask, lm_max_probe, uni_logp, uni_bow, C_lm, unk_logp, order, alpha, beta, top_n, fused};
  return beam_grouped("mrn_attn_beam_lm_decode_grouped_f32", false, o, eos, W, scratch, scratch_floats, tokens, length, score, logp, path,
                      prob, groups, hidden, stream, nullptr, &model);
}

MRN_EXPORT int mrn_attn_beam_lm_decode_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                  const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                  const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                  const void* const* w_inv, const void* const* b_hh, const void* const* w_gen,
                                                  const void* const* b_gen, const int* num_class, int eos, int W, int top_n,
                                                  const void* lm_keys, const float* lm_vals, int64_t lm_mask, int lm_max_probe,
                                                  const float* uni_logp, const float* uni_bow, int C_lm, float unk_logp, int order,
                                                  float alpha, float beta, const void* const* scratch, int64_t scratch_floats,
                                                  const void* const* tokens, const void* const* length, const void* const* score,
                                                  const void* const* logp, const void* const* path, const void* const* prob,
                                                  const void* const* fused, int groups, int B, int T, int D, int S, int hidden,
                                                  void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  const LMOperands model{lm_keys, lm_vals, lm_mask, lm_max_probe, uni_logp, uni_bow, C_lm, unk_logp, order, alpha, beta, top_n, fused};
  return beam_grouped("mrn_attn_beam_lm_decode_x3_grouped", true, o, eos, W, scratch, scratch_floats, tokens, length, score, logp, path, prob,
                      groups, hidden, stream, nullptr, &model);
}

// ---- exact scoring of per-sample candidate words on the attention head: attn_score_kernel (include/mrn_attn_score.h) ----
// the whole-context tile plus the row state (SCORE_LDS_EXTRA); there is no chunked form.  ops.attn_score_whole_context restates the rule
static int score_launch(ScoreGroup& grp, int groups, int D, int T, hipStream_t st) {
  grp.groups = groups;
  const int B = grp.g[0].g.a.B, K = grp.K;
  int per = 1;                               // slots of a sample in a workgroup: the smallest of 1, 2, 4, 8, 16 that is >= K
  while (per < K && per < BT) per *= 2;
  grp.per = per;
  grp.nblk = ceil_div(K, BT);                // K > 16: one sample per workgroup, nblk workgroups per sample
  grp.tiles = K > BT ? B * grp.nblk : ceil_div(B, BT / per);
  const dim3 grid = attn_grid(groups, grp.tiles, true, grp.pinned);
  const bool x3 = grp.g[0].g.a.w_inv != nullptr;
  const size_t lds = attn_tile_lds(x3, D, T, SCORE_LDS_EXTRA);
  if (x3) attn_kernel_launch(attn_score_kernel<true>, grp, grid, lds, st);
  else attn_kernel_launch(attn_score_kernel<false>, grp, grid, lds, st);
  MRN_LAUNCH_CHECK("attn_score");
  return MRN_OK;
}

// `groups` experts of identical geometry (B, T, D, S) and their own class counts in one launch per MAX_GROUPS experts; the word table
// and the candidate table are shared.  Every limit is checked for every group before the first launch
static int score_grouped(const char* who, bool x3, const DecodeOperands& o, int eos, const int32_t* lex_tokens, int Lmax,
                         const int32_t* lex_len, int N, const int32_t* cand, int K, PtrArray score_all, PtrArray logp, int groups,
                         int hidden, void* stream) {
  const int B = o.B, T = o.T, D = o.D, S = o.S;
  MRN_CHECK_ARG(decode_arrays_given(o, x3) && score_all && groups >= 1, "%s: null operand", who);
  MRN_CHECK_ARG(hidden == HID, "%s: hidden=%d unsupported (library is built for %d)", who, hidden, HID);
  MRN_CHECK_ARG(S >= 1 && S <= 512, "%s: S=%d steps outside 1 ... 512", who, S);
  MRN_CHECK_ARG(D > 0 && D % (x3 ? 32 : 16) == 0, "%s: D=%d must be a multiple of %d", who, D, x3 ? 32 : 16);
  MRN_CHECK_ARG(B >= 0 && T > 0, "%s: bad geometry (B=%d T=%d)", who, B, T);
  MRN_CHECK_ARG(attn_tile_lds(x3, D, T, SCORE_LDS_EXTRA) <= 160 * 1024, "%s: the whole context does not fit the LDS budget (D=%d T=%d)", who, D, T);
  MRN_CHECK_ARG(N >= 1 && N <= (1 << 20), "%s: N=%d words outside 1 ... 2^20", who, N);
  MRN_CHECK_ARG(Lmax >= 0 && lex_len && (lex_tokens || Lmax == 0), "%s: null word table (Lmax=%d)", who, Lmax);
  MRN_CHECK_ARG(K >= 1 && cand, "%s: K=%d candidate slots, needs K >= 1 and a table", who, K);
  MRN_CHECK_ARG((long)B * ceil_div(K, BT) <= (1L << 24), "%s: B=%d samples x K=%d slots: too many workgroups", who, B, K);
  for (int g = 0; g < groups; ++g) {
    MRN_CHECK_ARG(decode_group_given(o, x3, g) && (B == 0 || score_all[g]), "%s: null operand in group %d", who, g);
    MRN_CHECK_ARG(o.num_class[g] >= 2 && o.num_class[g] <= 65535, "%s: num_class=%d in group %d outside 2 ... 65535", who, o.num_class[g], g);
    MRN_CHECK_ARG(eos >= 0 && eos < o.num_class[g], "%s: eos=%d outside the %d classes of group %d", who, eos, o.num_class[g], g);
  }
  if (B == 0) return MRN_OK;
  for (int g0 = 0; g0 < groups; g0 += MAX_GROUPS) {
    const int n = groups - g0 < MAX_GROUPS ? groups - g0 : MAX_GROUPS;
    ScoreGroup grp;
    memset(&grp, 0, sizeof(grp));
    grp.lex_tokens = lex_tokens; grp.lex_len = lex_len; grp.cand = cand;
    grp.K = K; grp.N = N; grp.Lmax = Lmax; grp.eos = eos;
    for (int i = 0; i < n; ++i) {
      const int g = g0 + i;
      ScoreParams& sp = grp.g[i];
      greedy_fill(sp.g, o, x3, g);
      sp.score_all = (float*)score_all[g];
      sp.logp = logp ? (float*)logp[g] : nullptr;
    }
    const int rc = score_launch(grp, n, D, T, (hipStream_t)stream);
    if (rc) return rc;
  }
  return MRN_OK;
}

MRN_EXPORT int mrn_attn_score_candidates_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                     const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                     const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                     const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                                     const int* num_class, int eos, const int32_t* lex_tokens, int Lmax,
                                                     const int32_t* lex_len, int N, const int32_t* cand, int K,
                                                     const void* const* score_all, const void* const* logp, int groups, int B, int T,
                                                     int D, int S, int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, nullptr, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  return score_grouped("mrn_attn_score_candidates_grouped_f32", false, o, eos, lex_tokens, Lmax, lex_len, N, cand, K, score_all, logp, groups,
                       hidden, stream);
}

MRN_EXPORT int mrn_attn_score_candidates_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                                    const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                                    const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                                    const void* const* w_inv, const void* const* b_hh, const void* const* w_gen,
                                                    const void* const* b_gen, const int* num_class, int eos, const int32_t* lex_tokens,
                                                    int Lmax, const int32_t* lex_len, int N, const int32_t* cand, int K,
                                                    const void* const* score_all, const void* const* logp, int groups, int B, int T, int D,
                                                    int S, int hidden, void* stream) {
  const DecodeOperands o{Hb, Hproj, etab, start_token, w_h2h, b_h2h, w_score, w_ih_ctx, w_hh, w_inv, b_hh, w_gen, b_gen, num_class, B, T, D, S};
  return score_grouped("mrn_attn_score_candidates_x3_grouped", true, o, eos, lex_tokens, Lmax, lex_len, N, cand, K, score_all, logp, groups,
                       hidden, stream);
}
