// CTC prefix beam search on the device: the n-best labels of one evaluation batch from the [B, T, C] logits of a CTC head, one wave per
// sample, one launch per batch.  Best path (mrn_argmax_prob_f32 + the collapse of score.hip) picks the most likely ALIGNMENT; this
// picks the most likely LABEL by summing over alignments, and its score is that label's (pruned) log-probability.
//
// Reference op site it extends: test.py:211-219 (the CTC branch of validation(): preds.max(2), softmax maxima).  Class 0 is the blank
// (tools/utils.py:10-40, CTCLabelConverter).  The algorithm is the one mrn_amd/modules/decoding.py::ctc_beam_host restates in float64:
// per frame log-softmax, cut-off to the k = min(K, C - 1) non-blank classes of largest raw logit (ties to the lower class), stay and
// extension candidates, exact merge of an extension into the live entry that already spells it, then the W largest totals in
// candidate order (entry, slot).
//
// Layout of the work.  An entry (prefix, pb, pnb) lives in lane i < W: its log-probabilities, length, last class and a 32-bit hash of
// the prefix in registers, its classes as 16-bit tokens in this wave's LDS ([2][W][T]: parents are read from one half, children
// written to the other, and the halves swap).  The rank-r class of the cut-off lives in lane r < k.  Candidate q = i * (k + 1) + slot
// (slot 0 = stay, 1 + r = extend by the rank-r class) belongs to lane q % 64, register q / 64: W * (K + 1) <= 256 is four per lane, and
// q is the tie order of the selection.  Every cross-lane read is a __shfl all 64 lanes execute; only the token arrays go through LDS,
// and only this wave touches its LDS region, so there is no block-wide barrier anywhere.
//
// Language-model fusion (mrn_ctc_beam_lm_decode_f32, include/mrn_ctc_lm.h) is the same body with LM = true: lane i < W also holds
// e_prev, the class before e_last, and e_lm, the sum of the model's log-probabilities over the prefix; every lane looks up the model
// for its own up-to-four candidates (at most three bounded probe sequences of 8-byte reads each into a read-only hash table,
// char_lm.hpp), the selection ranks by total + alpha * lm' + beta * len' instead of the total, and after the last frame
// W more rounds of wave_argmax order the entries by the key with the end-of-text term.  With LM = false nothing of that is compiled.
#include <math.h>

#include "char_lm.hpp"
#include "common.hpp"

namespace {

constexpr int BEAM_MAX_T = 512;
constexpr int BEAM_MAX_C = 65535;  // classes are stored as 16-bit tokens
constexpr int BEAM_MAX_W = 16;
constexpr int BEAM_MAX_K = 15;
constexpr int BEAM_CPL = 4;                 // candidates per lane: 16 * (15 + 1) / 64
constexpr int BEAM_ROWS = 4;                // samples (waves) per block at most
constexpr int BEAM_LDS_BUDGET = 64 * 1024;  // per block: two blocks fit the 160 KiB of a CU at any T
constexpr int BEAM_DROP_BYTES = BEAM_MAX_W * 16;

// this wave's LDS writes are visible to its other lanes: a wave's LDS accesses complete in order, the fence keeps the compiler's order
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float log_add_exp(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (!(hi > -INFINITY)) return -INFINITY;
  return hi + log1pf(expf(lo - hi));
}

__device__ __forceinline__ unsigned hash_push(unsigned h, int c) { return (h ^ (unsigned)c) * 0x9E3779B1u + 0x7F4A7C15u; }

// wave-wide arg-max over (value, lower order wins a tie); order < 0 = nothing to offer
__device__ __forceinline__ void wave_argmax(float& v, int& q) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oq = __shfl_xor(q, o);
    const bool take = oq >= 0 && (q < 0 || ov > v || (ov == v && oq < q));
    v = take ? ov : v;
    q = take ? oq : q;
  }
}

// the model (char_lm.hpp) with what the fused search adds: the weights and the key output
struct BeamLM : CharLMTable {
  float* fused;                    // [B][W] out: the key the entries are ordered by
  float alpha, beta;
};

template <bool LM>
__global__ __launch_bounds__(256) void ctc_beam_kernel(const float* __restrict__ logits, long sb, long st, int B, int T, int C, int W, int K,
                                                       int32_t* __restrict__ tokens, int32_t* __restrict__ length,
                                                       float* __restrict__ score, int64_t* __restrict__ path,
                                                       float* __restrict__ prob, const BeamLM lm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char beam_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int rows = blockDim.x >> 6;
  const int b = blockIdx.x * rows + wave;
  if (b >= B) return;  // (no block-wide barrier below: every wave works on its own LDS region)
  const int row_bytes = 2 * W * T * (int)sizeof(unsigned short) + BEAM_DROP_BYTES;
  unsigned char* mine = beam_lds + (size_t)wave * row_bytes;
  unsigned char* drop = mine;  // [W][16]: extension (entry, rank) already lives as an entry and was merged into it
  unsigned short* tokbuf = (unsigned short*)(mine + BEAM_DROP_BYTES);
  unsigned short* cur = tokbuf;  // [W][T] prefixes of the live entries
  unsigned short* nxt = tokbuf + W * T;

  const int k = min(K, C - 1);
  const int kp1 = k + 1;
  int cand_i[BEAM_CPL], cand_slot[BEAM_CPL];  // entry and slot of this lane's candidates: the same at every frame
#pragma unroll
  for (int j = 0; j < BEAM_CPL; ++j) {
    const int q = lane + 64 * j;
    cand_i[j] = q / kp1;
    cand_slot[j] = q - cand_i[j] * kp1;
  }

  // entry state of lane i < n_live
  float e_pb = lane == 0 ? 0.f : -INFINITY, e_pnb = -INFINITY, e_tot = e_pb;
  int e_len = lane == 0 ? 0 : -1, e_last = -1;
  unsigned e_hash = 0;
  int n_live = 1;
  int e_prev = 0;    // LM: the class before e_last, 0 = begin of text
  float e_lm = 0.f;  // LM: the model's log-probability of the prefix

  const float* xb = logits + (long)b * sb;
  for (int t = 0; t < T; ++t) {
    const float* x = xb + (long)t * st;
    // ---- log-softmax constants of the frame: accurate expf / logf ----
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(x[c] - m);
    const float logz = logf(wave_sum(s));
    const float lp0 = (x[0] - m) - logz;

    // ---- cut-off: k rounds, each the first class in (logit descending, class ascending) order behind the previous winner ----
    int sc = 0;              // lane r < k: the rank-r class
    float slp = -INFINITY;   // ... and its log-probability
    float pv = INFINITY;
    int pc = 0;
    int kk = k;              // classes found (fewer than k only when logits are NaN)
    for (int r = 0; r < k; ++r) {
      float bv = -INFINITY;
      int bc = -1;
      for (int c = 1 + lane; c < C; c += 64) {
        const float v = x[c];
        const bool behind = v < pv || (v == pv && c > pc);
        if (behind && (bc < 0 || v > bv)) {  // c ascends within a lane: the first of equal values stays
          bv = v;
          bc = c;
        }
      }
      wave_argmax(bv, bc);
      if (bc < 0) {
        kk = r;
        break;
      }
      if (lane == r) {
        sc = bc;
        slp = (bv - m) - logz;
      }
      pv = bv;
      pc = bc;
    }

    // ---- entry space: rank of the last class in the cut-off, stay candidate, the one extension that spells this entry ----
    int e_rank = -1;
    float e_lplast = -INFINITY;
    for (int r = 0; r < kk; ++r) {
      const int c = __shfl(sc, r);
      const float l = __shfl(slp, r);
      if (c == e_last) {
        e_rank = r;
        e_lplast = l;
      }
    }
    float stay_pb = e_tot + lp0;
    float stay_pnb = e_rank >= 0 ? e_pnb + e_lplast : -INFINITY;
    ((unsigned*)drop)[lane] = 0u;  // 64 lanes x 4 bytes = [16][16]
    wave_sync();
    int par = -1;  // the live entry whose prefix is this entry's without its last class
    for (int i = 0; i < n_live; ++i) {
      const int li = __shfl(e_len, i);
      const unsigned hi = __shfl(e_hash, i);
      if (lane < n_live && e_rank >= 0 && par < 0 && li == e_len - 1 && hash_push(hi, e_last) == e_hash) {
        const unsigned short* pa = cur + i * T;
        const unsigned short* pj = cur + lane * T;
        bool same = true;  // the hash and the length pre-filter, the token arrays decide
        for (int u = 0; u < li && same; ++u) same = pa[u] == pj[u];
        if (same) par = i;
      }
    }
    {
      const int pi = par >= 0 ? par : 0;
      const float p_pb = __shfl(e_pb, pi), p_tot = __shfl(e_tot, pi);
      const int p_last = __shfl(e_last, pi);
      if (par >= 0) {
        const float ext = (e_last == p_last ? p_pb : p_tot) + e_lplast;
        stay_pnb = log_add_exp(stay_pnb, ext);
        drop[par * 16 + e_rank] = 1;  // at most one entry has a given (parent, class): no two lanes write one byte
      }
    }
    wave_sync();

    // ---- candidate space ----
    float c_pb[BEAM_CPL], c_pnb[BEAM_CPL], c_tot[BEAM_CPL];
    float c_key[BEAM_CPL], c_lm[BEAM_CPL];  // LM: the ranking key (-inf where the total is not finite) and lm' of the candidate
    float(&c_rank)[BEAM_CPL] = LM ? c_key : c_tot;
    const int n_cand = n_live * kp1;
#pragma unroll
    for (int j = 0; j < BEAM_CPL; ++j) {
      c_pb[j] = c_pnb[j] = c_tot[j] = -INFINITY;
      if constexpr (LM) {
        c_key[j] = -INFINITY;
        c_lm[j] = 0.f;
      }
      if (64 * j < n_cand) {  // wave-uniform
        const bool valid = lane + 64 * j < n_cand;
        const int i = valid ? cand_i[j] : 0;
        const int r = valid && cand_slot[j] > 0 ? cand_slot[j] - 1 : 0;
        const float s_pb = __shfl(stay_pb, i), s_pnb = __shfl(stay_pnb, i);
        const float p_pb = __shfl(e_pb, i), p_tot = __shfl(e_tot, i);
        const int p_last = __shfl(e_last, i);
        const int c = __shfl(sc, r);
        const float lpc = __shfl(slp, r);
        if (valid) {
          if (cand_slot[j] == 0) {
            c_pb[j] = s_pb;
            c_pnb[j] = s_pnb;
          } else if (r < kk && !drop[i * 16 + r]) {
            c_pnb[j] = (c == p_last ? p_pb : p_tot) + lpc;
          }
          const float tot = log_add_exp(c_pb[j], c_pnb[j]);
          c_tot[j] = isfinite(tot) ? tot : -INFINITY;
        }
        if constexpr (LM) {
          const int p_prev = __shfl(e_prev, i), p_len = __shfl(e_len, i);
          const float p_lm = __shfl(e_lm, i);
          if (valid && c_tot[j] > -INFINITY) {
            const bool ext = cand_slot[j] > 0;
            c_lm[j] = ext ? p_lm + lm_logp(lm, p_prev, max(p_last, 0), c) : p_lm;
            c_key[j] = c_tot[j] + lm.alpha * c_lm[j] + lm.beta * (float)(p_len + (ext ? 1 : 0));
          }
        }
      }
    }

    // ---- select: W rounds of a wave-wide arg-max over (total, candidate order) ----
    float n_pb = -INFINITY, n_pnb = -INFINITY, n_tot = -INFINITY;
    int n_len = -1, n_last = -1;
    unsigned n_hash = 0;
    int live = 0;
    int n_prev = 0;
    float n_lm = 0.f;
    for (int n = 0; n < W; ++n) {
      float bt = -INFINITY, l_pb = -INFINITY, l_pnb = -INFINITY;  // this lane's best candidate
      float l_tot = -INFINITY, l_lm = 0.f;
      int bq = -1, lj = -1;
#pragma unroll
      for (int j = 0; j < BEAM_CPL; ++j)
        if (c_rank[j] > bt) {  // j ascends: the lower order keeps a tie
          bt = c_rank[j];
          l_pb = c_pb[j];
          l_pnb = c_pnb[j];
          if constexpr (LM) {
            l_tot = c_tot[j];
            l_lm = c_lm[j];
          }
          lj = j;
          bq = lane + 64 * j;
        }
      wave_argmax(bt, bq);
      if (bq < 0) break;
      bq = __builtin_amdgcn_readfirstlane(bq);
      const int owner = bq & 63;
      const float v_pb = __shfl(l_pb, owner), v_pnb = __shfl(l_pnb, owner);
      float v_tot = bt, v_lm = 0.f;  // LM: bt is the key, the total and lm' come from the owner
      if constexpr (LM) {
        v_tot = __shfl(l_tot, owner);
        v_lm = __shfl(l_lm, owner);
      }
#pragma unroll
      for (int j = 0; j < BEAM_CPL; ++j)
        if (lane == owner && j == lj) c_rank[j] = -INFINITY;  // (the winner is its owner's best: lj is its register)
      const int i = bq / kp1, slot = bq - i * kp1;
      const int p_len = __shfl(e_len, i), p_last = __shfl(e_last, i);
      const unsigned p_hash = __shfl(e_hash, i);
      const int c = __shfl(sc, slot > 0 ? slot - 1 : 0);
      if (lane == n) {
        n_pb = v_pb;
        n_pnb = v_pnb;
        n_tot = v_tot;
        n_len = p_len + (slot > 0 ? 1 : 0);
        n_last = slot > 0 ? c : p_last;
        n_hash = slot > 0 ? hash_push(p_hash, c) : p_hash;
      }
      if constexpr (LM) {
        const int p_prev = __shfl(e_prev, i);
        if (lane == n) {
          n_prev = slot > 0 ? max(p_last, 0) : p_prev;
          n_lm = v_lm;
        }
      }
      const unsigned short* src = cur + i * T;
      unsigned short* dst = nxt + n * T;
      for (int u = lane; u < p_len; u += 64) dst[u] = src[u];
      if (slot > 0 && lane == 0 && p_len < T) dst[p_len] = (unsigned short)c;  // (a prefix of t + 1 frames has at most t + 1 classes)
      live = n + 1;
    }
    e_pb = n_pb;
    e_pnb = n_pnb;
    e_tot = n_tot;
    e_len = n_len;
    e_last = n_last;
    e_hash = n_hash;
    if constexpr (LM) {
      e_prev = n_prev;
      e_lm = n_lm;
    }
    n_live = live;
    unsigned short* swap = cur;
    cur = nxt;
    nxt = swap;
    wave_sync();
  }

  // ---- LM: order the live entries by the key with the end-of-text term; lane n takes the state of its winner, the tokens stay ----
  int e_row = lane;  // the token row of this lane's entry
  if constexpr (LM) {
    const bool mine = lane < n_live;
    const float fkey = mine ? e_tot + lm.alpha * (e_lm + lm_logp(lm, e_prev, max(e_last, 0), 0)) + lm.beta * (float)e_len : -INFINITY;
    bool taken = !mine;
    float n_fused = -INFINITY;
    for (int n = 0; n < n_live; ++n) {
      float bv = taken ? -INFINITY : fkey;
      int bq = taken ? -1 : lane;
      wave_argmax(bv, bq);  // (a live entry's key is finite: one is found every round)
      if (bq < 0) break;
      bq = __builtin_amdgcn_readfirstlane(bq);
      if (lane == bq) taken = true;
      if (lane == n) {
        e_row = bq;
        n_fused = bv;
      }
    }
    e_tot = __shfl(e_tot, e_row);
    e_len = __shfl(e_len, e_row);
    if (lane < W) lm.fused[(long)b * W + lane] = n_fused;
  }

  // ---- outputs: the entries in their order (descending total; LM: descending key) ----
  if (lane < W) {
    length[(long)b * W + lane] = e_len;
    score[(long)b * W + lane] = e_tot;
  }
  for (int w = 0; w < W; ++w) {
    const int len = __shfl(e_len, w);
    int32_t* out = tokens + ((long)b * W + w) * T;
    const unsigned short* src = cur + (LM ? __shfl(e_row, w) : w) * T;
    for (int u = lane; u < T; u += 64) out[u] = u < len ? (int32_t)src[u] : 0;
  }
  if constexpr (LM) cur += __shfl(e_row, 0) * T;  // the best entry's row, for the path below
  // the best entry as a frame row: a blank between equal neighbours, blanks behind; greedy collapse gives the prefix back
  const int len0 = max(__shfl(e_len, 0), 0);
  const float tot0 = __shfl(e_tot, 0);
  int64_t* pth = path + (long)b * T;
  float* prb = prob + (long)b * T;
  int shift = 0;  // blanks inserted so far
  for (int t0 = 0; t0 < len0; t0 += 64) {
    const int u = t0 + lane;
    const int tok = u < len0 ? cur[u] : 0;
    const bool dup = u < len0 && u > 0 && tok == cur[u - 1];
    const unsigned long long mask = __ballot(dup);
    const int pos = u + shift + __popcll(mask & ((2ull << lane) - 1ull));
    if (u < len0 && pos < T) {
      pth[pos] = tok;
      if (dup) pth[pos - 1] = 0;
    }
    shift += __popcll(mask);
  }
  for (int u = min(len0 + shift, T) + lane; u < T; u += 64) pth[u] = 0;
  for (int u = lane; u < T; u += 64) prb[u] = u == 0 ? expf(tot0) : 1.f;
}

}  // namespace

MRN_EXPORT int mrn_ctc_beam_decode_f32(const float* logits, int64_t stride_b, int64_t stride_t, int B, int T, int C, int W, int K,
                                       int32_t* tokens, int32_t* length, float* score, int64_t* path, float* prob, void* stream) {
  MRN_CHECK_ARG(B >= 0 && stride_b >= 0 && stride_t >= 0, "mrn_ctc_beam_decode_f32: B = %d, strides %ld / %ld", B, (long)stride_b,
                (long)stride_t);
  MRN_CHECK_ARG(T >= 1 && T <= BEAM_MAX_T, "mrn_ctc_beam_decode_f32: T = %d outside 1..%d", T, BEAM_MAX_T);
  MRN_CHECK_ARG(C >= 2 && C <= BEAM_MAX_C, "mrn_ctc_beam_decode_f32: C = %d outside 2..%d", C, BEAM_MAX_C);
  MRN_CHECK_ARG(W >= 1 && W <= BEAM_MAX_W, "mrn_ctc_beam_decode_f32: beam width %d outside 1..%d", W, BEAM_MAX_W);
  MRN_CHECK_ARG(K >= 1 && K <= BEAM_MAX_K, "mrn_ctc_beam_decode_f32: cut-off %d outside 1..%d", K, BEAM_MAX_K);
  if (B == 0) return MRN_OK;
  MRN_CHECK_ARG(logits && tokens && length && score && path && prob, "mrn_ctc_beam_decode_f32: bad operands");
  const int row_bytes = 2 * W * T * (int)sizeof(unsigned short) + BEAM_DROP_BYTES;  // <= 33024
  int rows = BEAM_LDS_BUDGET / row_bytes;
  rows = rows > BEAM_ROWS ? BEAM_ROWS : rows;
  const dim3 grid((unsigned)((B + rows - 1) / rows)), block(64 * rows);
  hipLaunchKernelGGL(ctc_beam_kernel<false>, grid, block, (size_t)rows * row_bytes, (hipStream_t)stream, logits, (long)stride_b,
                     (long)stride_t, B, T, C, W, K, tokens, length, score, path, prob, BeamLM{});
  MRN_LAUNCH_CHECK("ctc_beam_decode");
  return MRN_OK;
}

MRN_EXPORT int mrn_ctc_beam_lm_decode_f32(const float* logits, int64_t stride_b, int64_t stride_t, int B, int T, int C, int W, int K,
                                          int32_t* tokens, int32_t* length, float* score, int64_t* path, float* prob,
                                          const void* lm_keys, const float* lm_vals, int64_t lm_mask, int lm_max_probe,
                                          const float* uni_logp, const float* uni_bow, int C_lm, float unk_logp, int order, float alpha,
                                          float beta, float* fused, void* stream) {
  MRN_CHECK_ARG(B >= 0 && stride_b >= 0 && stride_t >= 0, "mrn_ctc_beam_lm_decode_f32: B = %d, strides %ld / %ld", B, (long)stride_b,
                (long)stride_t);
  MRN_CHECK_ARG(T >= 1 && T <= BEAM_MAX_T, "mrn_ctc_beam_lm_decode_f32: T = %d outside 1..%d", T, BEAM_MAX_T);
  MRN_CHECK_ARG(C >= 2 && C <= BEAM_MAX_C, "mrn_ctc_beam_lm_decode_f32: C = %d outside 2..%d", C, BEAM_MAX_C);
  MRN_CHECK_ARG(W >= 1 && W <= BEAM_MAX_W, "mrn_ctc_beam_lm_decode_f32: beam width %d outside 1..%d", W, BEAM_MAX_W);
  MRN_CHECK_ARG(K >= 1 && K <= BEAM_MAX_K, "mrn_ctc_beam_lm_decode_f32: cut-off %d outside 1..%d", K, BEAM_MAX_K);
  MRN_CHECK_ARG(order >= 1 && order <= 3, "mrn_ctc_beam_lm_decode_f32: order %d outside 1..3", order);
  MRN_CHECK_ARG(C_lm >= 1 && C_lm <= CHAR_LM_MAX_C, "mrn_ctc_beam_lm_decode_f32: C_lm = %d outside 1..%d", C_lm, CHAR_LM_MAX_C);
  MRN_CHECK_ARG(lm_mask >= 0 && lm_mask < CHAR_LM_MAX_SLOTS && ((lm_mask + 1) & lm_mask) == 0,
                "mrn_ctc_beam_lm_decode_f32: table mask %ld is not a power of two up to 2^26 less one", (long)lm_mask);
  MRN_CHECK_ARG(lm_max_probe >= 0 && (int64_t)lm_max_probe <= lm_mask + 1, "mrn_ctc_beam_lm_decode_f32: max_probe %d outside 0..%ld",
                lm_max_probe, (long)(lm_mask + 1));
  MRN_CHECK_ARG(isfinite(unk_logp) && isfinite(alpha) && alpha >= 0.f && isfinite(beta),
                "mrn_ctc_beam_lm_decode_f32: unk_logp %g, alpha %g (>= 0) and beta %g must be finite", (double)unk_logp, (double)alpha,
                (double)beta);
  if (B == 0) return MRN_OK;
  MRN_CHECK_ARG(logits && tokens && length && score && path && prob && fused && lm_keys && lm_vals && uni_logp && uni_bow,
                "mrn_ctc_beam_lm_decode_f32: bad operands");
  BeamLM lm;
  lm.keys = (const unsigned long long*)lm_keys;
  lm.vals = (const float2*)lm_vals;
  lm.uni_logp = uni_logp;
  lm.uni_bow = uni_bow;
  lm.fused = fused;
  lm.mask = (unsigned)lm_mask;
  lm.max_probe = lm_max_probe;
  lm.C_lm = C_lm;
  lm.order = order;
  lm.unk_logp = unk_logp;
  lm.alpha = alpha;
  lm.beta = beta;
  const int row_bytes = 2 * W * T * (int)sizeof(unsigned short) + BEAM_DROP_BYTES;  // the layout and the rows-per-block rule above
  int rows = BEAM_LDS_BUDGET / row_bytes;
  rows = rows > BEAM_ROWS ? BEAM_ROWS : rows;
  const dim3 grid((unsigned)((B + rows - 1) / rows)), block(64 * rows);
  hipLaunchKernelGGL(ctc_beam_kernel<true>, grid, block, (size_t)rows * row_bytes, (hipStream_t)stream, logits, (long)stride_b,
                     (long)stride_t, B, T, C, W, K, tokens, length, score, path, prob, lm);
  MRN_LAUNCH_CHECK("ctc_beam_lm_decode");
  return MRN_OK;
}
