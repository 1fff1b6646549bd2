// Lexicon-constrained decoding of a CTC head on the device: the exact log-probability log p(word | image) of every (sample, word)
// pair of one evaluation batch by the CTC forward recursion, and per sample the n most likely words.  The lexicon-free decoders
// (mrn_argmax_prob_f32 + the collapse of score.hip, ctc_beam.hip) answer "which string"; this answers "which of these words", the
// protocol of the 50 / 1k / full lexicons of the scene-text benchmarks (CRNN).
//
// Reference op site it extends: test.py:211-219 (the CTC branch of validation()).  Class 0 is the blank (tools/utils.py:10-40).  The
// algorithm is the one mrn_amd/modules/decoding.py::ctc_lexicon_host restates in float64: per frame lp = x - logsumexp(x), states
// blank, c_1, blank, ..., c_L, blank, alpha_t(s) = lp[t][z_s] + logaddexp(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2)]),
// score = logaddexp of the last two states: -ctc_loss(log_softmax(x), word) without a [B*N, T, C] replica of anything.
//
// Layout of the work.  Three launches per batch:
//   lex_lse_kernel     one block per frame row: lse[B][T], the only intermediate besides score_all (it borrows the prob output);
//   lex_score_kernel   one wave per (sample, word): state s in lane s (63 states at L = 31), alpha(s-1) / alpha(s-2) by cross-lane
//                      shifts, per frame one gathered logit per lane (blank lanes read column 0), the next frame's gather issued
//                      before this frame's math.  The four waves of a block score four words of ONE sample, and a sample's blocks
//                      are neighbours on one XCD (xcd_remap), so its rows are re-read from L2;
//   lex_select_kernel  one block per sample: n rounds of a block-wide arg-max over score_all in (score descending, position
//                      ascending) order, then the best word as a frame row.
// The lexicon and the candidate lists are device data, so their range check is a pass of its own (lex_check_kernel) whose verdict
// the host reads before anything else is launched: the entry point synchronises the stream once and cannot be captured in a graph.
#include <math.h>

#include <mutex>

#include "common.hpp"

namespace {

constexpr int LEX_MAX_T = 512;
constexpr int LEX_MAX_C = 65535;
constexpr int LEX_MAX_L = 31;  // 2 L + 1 <= 64 states: the limit of the 64-state CTC loss kernel
constexpr int LEX_MAX_N = 1 << 20;
constexpr int LEX_MAX_TOP = 16;
constexpr int LEX_WAVES = 4;  // words per block

__device__ int g_lex_bad[4];  // verdict of lex_check_kernel: {length, token, candidate} out of range
std::mutex g_lex_mutex;       // one check at a time owns g_lex_bad

__global__ __launch_bounds__(256) void lex_check_kernel(const int32_t* __restrict__ tok, int Lmax, const int32_t* __restrict__ len, int N,
                                                        int C, const int32_t* __restrict__ cand, long n_cand, int* __restrict__ bad) {
  const long stride = (long)gridDim.x * 256;
  const long first = (long)blockIdx.x * 256 + threadIdx.x;
  const int lim = Lmax < LEX_MAX_L ? Lmax : LEX_MAX_L;
  for (long i = first; i < N; i += stride) {
    const int l = len[i];
    if (l < 0 || l > lim) bad[0] = 1;
  }
  for (long i = first; i < (long)N * Lmax; i += stride) {
    const int w = (int)(i / Lmax), u = (int)(i - (long)w * Lmax);
    const int l = len[w];
    if (l >= 0 && l <= lim && u < l) {
      const int c = tok[i];
      if (c < 1 || c >= C) bad[1] = 1;
    }
  }
  for (long i = first; i < n_cand; i += stride) {
    const int w = cand[i];
    if (w < -1 || w >= N) bad[2] = 1;
  }
}

// one block per row: lse = m + log sum exp(x - m).  A NaN or +inf logit, or a row of -inf, gives NaN: the sample is dead
__global__ __launch_bounds__(256) void lex_lse_kernel(const float* __restrict__ x, long sb, long st, int T, int C, float* __restrict__ lse) {
  __shared__ float scratch[4];
  const long row = blockIdx.x;
  const long b = row / T, t = row - b * T;
  const float* xr = x + b * sb + t * st;
  float m = -INFINITY;
  for (int c = threadIdx.x; c < C; c += 256) m = fmaxf(m, xr[c]);
  m = block_max<256>(m, scratch);
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) s += expf(xr[c] - m);
  s = block_sum<256>(s, scratch);
  if (threadIdx.x == 0) lse[row] = m + logf(s);
}

__global__ __launch_bounds__(256) void lex_score_kernel(const float* __restrict__ x, long sb, long st, const float* __restrict__ lse, int T,
                                                        const int32_t* __restrict__ tok, int Lmax, const int32_t* __restrict__ len,
                                                        const int32_t* __restrict__ cand, int K, int Nc, int chunks,
                                                        float* __restrict__ score_all) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int bid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int b = bid / chunks;
  const int j = (bid - b * chunks) * LEX_WAVES + wave;
  if (j >= Nc) return;  // (no block-wide barrier below)
  float* out = score_all + (long)b * Nc + j;
  const int w = cand ? cand[(long)b * K + j] : j;
  const float* lb = lse + (long)b * T;
  bool bad = false;  // a NaN lse in any frame: every word of the sample is dead
  for (int t = lane; t < T; t += 64) {
    const float v = lb[t];
    bad |= v != v;
  }
  if (w < 0 || __any(bad)) {
    if (lane == 0) *out = -INFINITY;
    return;
  }
  const int L = len[w];
  const int S = 2 * L + 1;
  const bool live = lane < S;
  const int cls = (live && (lane & 1)) ? tok[(long)w * Lmax + (lane >> 1)] : 0;
  const int cls_m2 = __shfl_up(cls, 2);
  const bool skip = live && (lane & 1) && lane >= 3 && cls != cls_m2;  // may come from s - 2
  const float* xp = x + (long)b * sb + cls;                            // this lane's column: in bounds for dead lanes too (column 0)

  float xt = xp[0];
  float a = (lane == 0 || (lane == 1 && L > 0)) ? xt - lb[0] : -INFINITY;
  if (T > 1) xt = xp[st];
  for (int t = 1; t < T; ++t) {
    const float xc = xt;
    if (t + 1 < T) xt = xp[(long)(t + 1) * st];  // the next frame's gather flies during this frame's math
    float a1 = __shfl_up(a, 1), a2 = __shfl_up(a, 2);
    if (lane < 1) a1 = -INFINITY;
    if (!skip) a2 = -INFINITY;
    const float m = fmaxf(fmaxf(a, a1), a2);
    float acc = -INFINITY;
    if (m > -INFINITY) acc = m + logf(expf(a - m) + expf(a1 - m) + expf(a2 - m));
    a = live ? acc + (xc - lb[t]) : -INFINITY;
  }
  const float e1 = __shfl(a, S - 1);
  const float e2 = __shfl(a, S >= 2 ? S - 2 : 0);
  float sc = e1;
  if (S >= 2) {
    const float m = fmaxf(e1, e2);
    sc = m > -INFINITY ? m + logf(expf(e1 - m) + expf(e2 - m)) : -INFINITY;
  }
  if (lane == 0) *out = sc == sc ? sc : -INFINITY;
}

// wave-wide arg-max over (value, lower position wins a tie); position < 0 = nothing to offer
__device__ __forceinline__ void lex_argmax(float& v, int& q) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oq = __shfl_xor(q, o);
    const bool take = oq >= 0 && (q < 0 || ov > v || (ov == v && oq < q));
    v = take ? ov : v;
    q = take ? oq : q;
  }
}

__global__ __launch_bounds__(256) void lex_select_kernel(const float* __restrict__ score_all, int Nc, const int32_t* __restrict__ cand, int K,
                                                         const int32_t* __restrict__ tok, int Lmax, const int32_t* __restrict__ len, int n,
                                                         int T, int32_t* __restrict__ index, float* __restrict__ score,
                                                         int64_t* __restrict__ path, float* __restrict__ prob) {
  __shared__ float sv[4];
  __shared__ int sq[4];
  __shared__ int s_pos;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = score_all + (long)b * Nc;
  float pv = INFINITY;  // the previous winner: round r takes the first position behind it in (score descending, position ascending)
  int pj = -1;
  float v0 = -INFINITY;
  int j0 = -1;
  int r = 0;
  for (; r < n; ++r) {
    float bv = -INFINITY;
    int bj = -1;
    for (int j = tid; j < Nc; j += 256) {
      const float v = row[j];
      const bool behind = v < pv || (v == pv && j > pj);
      if (behind && v > -INFINITY && (bj < 0 || v > bv)) {  // j ascends within a thread: the first of equal scores stays
        bv = v;
        bj = j;
      }
    }
    lex_argmax(bv, bj);
    __syncthreads();
    if (lane == 0) {
      sv[wave] = bv;
      sq[wave] = bj;
    }
    __syncthreads();
    bv = sv[0];
    bj = sq[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      const float ov = sv[i];
      const int oq = sq[i];
      if (oq >= 0 && (bj < 0 || ov > bv || (ov == bv && oq < bj))) {
        bv = ov;
        bj = oq;
      }
    }
    if (bj < 0) break;  // block-uniform: no live position is left
    if (tid == 0) {
      index[(long)b * n + r] = cand ? cand[(long)b * K + bj] : bj;
      score[(long)b * n + r] = bv;
    }
    if (r == 0) {
      v0 = bv;
      j0 = bj;
    }
    pv = bv;
    pj = bj;
  }
  for (int i = r + tid; i < n; i += 256) {  // dead slots come last
    index[(long)b * n + i] = -1;
    score[(long)b * n + i] = -INFINITY;
  }
  // the best word as a frame row: a blank between equal neighbours, blanks behind; greedy collapse gives the word back
  int64_t* pth = path + (long)b * T;
  float* prb = prob + (long)b * T;
  if (tid == 0) {
    int pos = 0;
    if (j0 >= 0) {
      const int w = cand ? cand[(long)b * K + j0] : j0;
      const int L = len[w];
      int prev = 0;
      for (int u = 0; u < L; ++u) {
        const int c = tok[(long)w * Lmax + u];
        if (c == prev && pos < T) pth[pos++] = 0;
        if (pos < T) pth[pos++] = c;  // (a live word has L + repeats <= T)
        prev = c;
      }
    }
    s_pos = pos;
  }
  __syncthreads();
  for (int u = s_pos + tid; u < T; u += 256) pth[u] = 0;
  for (int u = tid; u < T; u += 256) prb[u] = u == 0 ? (j0 >= 0 ? expf(v0) : 0.f) : 1.f;
}

}  // namespace

MRN_EXPORT int mrn_ctc_lexicon_decode_f32(const float* logits, int64_t stride_b, int64_t stride_t, int B, int T, int C,
                                          const int32_t* lex_tokens, int Lmax, const int32_t* lex_len, int N, const int32_t* cand, int K,
                                          int n, int32_t* index, float* score, float* score_all, int64_t* path, float* prob, void* stream) {
  const char* me = "mrn_ctc_lexicon_decode_f32";
  MRN_CHECK_ARG(B >= 0 && stride_b >= 0 && stride_t >= 0, "%s: B = %d, strides %ld / %ld", me, B, (long)stride_b, (long)stride_t);
  MRN_CHECK_ARG(T >= 1 && T <= LEX_MAX_T, "%s: T = %d outside 1..%d", me, T, LEX_MAX_T);
  MRN_CHECK_ARG(C >= 2 && C <= LEX_MAX_C, "%s: C = %d outside 2..%d", me, C, LEX_MAX_C);
  MRN_CHECK_ARG(N >= 1 && N <= LEX_MAX_N, "%s: N = %d words outside 1..%d", me, N, LEX_MAX_N);
  MRN_CHECK_ARG(Lmax >= 0, "%s: Lmax = %d", me, Lmax);
  MRN_CHECK_ARG(n >= 1 && n <= LEX_MAX_TOP, "%s: n = %d entries outside 1..%d", me, n, LEX_MAX_TOP);
  MRN_CHECK_ARG(!cand || K >= 1, "%s: K = %d candidate slots, needs K >= 1", me, K);
  if (B == 0) return MRN_OK;
  MRN_CHECK_ARG(logits && lex_len && (lex_tokens || Lmax == 0) && index && score && score_all && path && prob,
                "%s: bad operands", me);
  const int Nc = cand ? K : N;
  const int chunks = (Nc + LEX_WAVES - 1) / LEX_WAVES;
  MRN_CHECK_ARG((long)B * chunks <= 0x7fffffffL && (long)B * T <= 0x7fffffffL, "%s: B = %d samples x %d positions: too many blocks", me, B,
                Nc);
  hipStream_t st = (hipStream_t)stream;
  float* lse = prob;  // [B][T]: prob holds the frames' lse until lex_select_kernel, the last launch, writes the probabilities over it

  // ---- the device-resident operands: word lengths, tokens, candidate indices ----
  int bad[3] = {0, 0, 0};
  {
    std::lock_guard<std::mutex> hold(g_lex_mutex);
    int* flag = nullptr;
    hipError_t e = hipGetSymbolAddress((void**)&flag, HIP_SYMBOL(g_lex_bad));
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(bad), st);
    if (e == hipSuccess) {
      const long work = (long)N * (Lmax > 0 ? Lmax : 1) + (cand ? (long)B * K : 0);
      const long blocks = (work + 255) / 256;
      hipLaunchKernelGGL(lex_check_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, lex_tokens, Lmax, lex_len, N, C,
                         cand, cand ? (long)B * K : 0L, flag);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      mrn_set_error("%s: lexicon check failed: %s", me, hipGetErrorString(e));
      return (int)e;
    }
  }
  MRN_CHECK_ARG(!bad[0], "%s: a word length outside 0..%d (Lmax = %d)", me, Lmax < LEX_MAX_L ? Lmax : LEX_MAX_L, Lmax);
  MRN_CHECK_ARG(!bad[1], "%s: a word token outside 1..%d", me, C - 1);
  MRN_CHECK_ARG(!bad[2], "%s: a candidate index outside -1..%d", me, N - 1);

  hipLaunchKernelGGL(lex_lse_kernel, dim3((unsigned)((long)B * T)), dim3(256), 0, st, logits, (long)stride_b, (long)stride_t, T, C, lse);
  MRN_LAUNCH_CHECK("ctc_lexicon_lse");
  hipLaunchKernelGGL(lex_score_kernel, dim3((unsigned)((long)B * chunks)), dim3(64 * LEX_WAVES), 0, st, logits, (long)stride_b,
                     (long)stride_t, lse, T, lex_tokens, Lmax, lex_len, cand, K, Nc, chunks, score_all);
  MRN_LAUNCH_CHECK("ctc_lexicon_score");
  hipLaunchKernelGGL(lex_select_kernel, dim3((unsigned)B), dim3(256), 0, st, score_all, Nc, cand, K, lex_tokens, Lmax, lex_len, n, T, index,
                     score, path, prob);
  MRN_LAUNCH_CHECK("ctc_lexicon_select");
  return MRN_OK;
}
