// Validation scoring on the device: greedy-decode collapse, confidence and unit-cost edit distance of one evaluation batch, one
// wave per sample.  The host loop it replaces (mrn_amd/test.py) decoded every sample to a string, ran an O(len^2) Python Levenshtein
// and one np.cumprod per sample; here the same rules run on integer tokens, so every output is equal to the host's, not just close.
//
// Reference op sites: test.py:211-265 (greedy decode, [EOS] cut, ICDAR-2019 normalised edit distance, exact match, confidence as the
// cumulative product of the per-step maxima), tools/utils.py:62-76 (CTC collapse: drop blanks, merge repeats of the RAW index),
// tools/utils.py:133-143 (attention decode).
//
// Tokens are CANONICAL classes (mrn_amd/modules/scoring.py): canon[k] is the dictionary index of the character class k decodes to, so
// two classes that decode to the same character compare equal, as their strings do; -2 marks a class whose string is longer than
// one character ([UNK], [PAD], [SOS]) -- such a sample is flagged for the host, which scores it on strings.  A label character
// outside the dictionary is -1 and equals nothing.
//
// Levenshtein as an anti-diagonal wavefront: lanes run across the label (CPL consecutive columns per lane, 64 * CPL >= Lmax),
// diagonal k = i + j holds the cells that depend only on diagonals k - 1 and k - 2, which live in registers; one step costs one
// cross-lane shift (the left neighbour's last column), one LDS read (the next prediction token slides in) and CPL cells of integer
// min / compare.  n + m - 1 steps per sample.  A DP row with a prefix-min scan would take n steps of six shifts each.
#include "common.hpp"

namespace {

constexpr int SCORE_MAX_T = 512;
constexpr int SCORE_MAX_L = 256;
constexpr int SCORE_ROWS = 4;  // samples (waves) per 256-thread block

// exclusive count of set bits below this lane
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// D[n][m] of the unit-cost Levenshtein table between tok[0..n) (LDS, this wave's row) and this lane's label columns
// lab[c] = label[CPL * lane + c] (-1 beyond m); m >= 1.  Column j = 1 + CPL * lane + c; a column "above the table" (row i <= 0)
// holds D[0][j] = j, a column past row n keeps D[n][j].  Columns beyond m compute garbage nobody to their right consumes.
template <int CPL>
__device__ __forceinline__ int wavefront_levenshtein(const int* tok, int n, const int (&lab)[CPL], int m, int lane) {
  int d1[CPL], d2[CPL], pt[CPL];  // diagonal k-1, diagonal k-2, prediction token index of the cell (row i - 1 = k - 1 - j)
  const int j0 = 1 + CPL * lane;
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    d1[c] = j0 + c;
    d2[c] = j0 + c;
    pt[c] = 0;
  }
  int dg_left = j0 - 1;  // diagonal k-2 at column j0 - 1 (the previous step's shifted-in value)
  for (int k = 2; k <= n + m; ++k) {
    int left = __shfl_up(d1[CPL - 1], 1);  // diagonal k-1 at column j0 - 1 = D[i][j0 - 1]
    if (lane == 0) left = k - 1;           // column 0: D[i][0] = i
#pragma unroll
    for (int c = CPL - 1; c > 0; --c) pt[c] = pt[c - 1];
    const int r0 = k - 1 - j0;  // row index (i - 1) of this lane's first column on diagonal k
    pt[0] = (r0 >= 0 && r0 < n) ? tok[r0] : 0;
    int nd[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int lf = c ? d1[c - 1] : left;
      const int dg = c ? d2[c - 1] : dg_left;
      const int r = r0 - c;
      const int v = min(min(d1[c] + 1, lf + 1), dg + (pt[c] != lab[c] ? 1 : 0));
      nd[c] = (r >= 0 && r < n) ? v : d1[c];
    }
    dg_left = left;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      d2[c] = d1[c];
      d1[c] = nd[c];
    }
  }
  // column m lives in lane (m - 1) / CPL, slot (m - 1) % CPL
  int mine = d1[0];
#pragma unroll
  for (int c = 1; c < CPL; ++c)
    if ((m - 1) % CPL == c) mine = d1[c];
  return __shfl(mine, (m - 1) / CPL);
}

template <int CPL>
__global__ __launch_bounds__(256) void greedy_score_kernel(const int64_t* __restrict__ idx, const float* __restrict__ prob, int B, int T,
                                                           const int32_t* __restrict__ label, const int32_t* __restrict__ label_len,
                                                           int Lmax, const int32_t* __restrict__ canon, int C, int mode, int eos,
                                                           int32_t* __restrict__ tokens, int32_t* __restrict__ result,
                                                           float* __restrict__ confidence) {
  __shared__ int s_tok[SCORE_ROWS][SCORE_MAX_T];
  __shared__ float s_prob[SCORE_ROWS][SCORE_MAX_T];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * SCORE_ROWS + wave;
  if (b >= B) return;  // (no block-wide barrier below: every wave works on its own LDS rows)
  int* tok = s_tok[wave];
  float* pr = s_prob[wave];
  const int64_t* ib = idx + (long)b * T;
  const float* pb = prob + (long)b * T;
  int32_t* tb = tokens + (long)b * T;

  // ---- which positions are kept, front-packed into LDS and `tokens` ----
  int n = 0;           // kept tokens so far
  int flagged = 0;     // a scanned token decodes to more than one character
  int cut = T;         // attention: position of the first [EOS]
  if (mode == 1) {
    for (int t0 = 0; t0 < T && cut == T; t0 += 64) {
      const int t = t0 + lane;
      const bool is_eos = t < T && ib[t] == (int64_t)eos;
      const unsigned long long mask = __ballot(is_eos);
      if (mask) cut = t0 + __ffsll((long long)mask) - 1;
    }
  }
  const int keep_end = mode == 1 ? (cut < T ? cut : T - 1) : T;   // no [EOS]: the last position is dropped (find() == -1)
  const int scan_end = mode == 1 ? (cut < T ? cut : T) : T;       // ... but still scanned for multi-character tokens
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    bool keep = false;
    int ct = -2;
    if (t < T) {
      pr[t] = pb[t];
      if (t < scan_end) {
        const int64_t k = ib[t];
        if (mode == 0) keep = k != 0 && (t == 0 || k != ib[t - 1]);
        else keep = true;
        if (keep) ct = (k >= 0 && k < C) ? canon[k] : -2;
      }
    }
    if (__ballot(keep && ct == -2)) flagged = 1;
    keep = keep && t < keep_end;
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int pos = n + lanes_below(mask, lane);
      tok[pos] = ct;
      tb[pos] = ct;
    }
    n += __popcll(mask);
  }
  for (int t = n + lane; t < T; t += 64) tb[t] = -1;
  // other lanes of this wave read tok[] / pr[] below: a wave's LDS accesses complete in order, the fence keeps the compiler's order too
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // ---- edit distance against label[:m] ----
  const int m = min(max(label_len[b], 0), Lmax);
  int lab[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int j = CPL * lane + c;
    lab[c] = j < m ? label[(long)b * Lmax + j] : -1;
  }
  const int dist = m == 0 ? n : wavefront_levenshtein<CPL>(tok, n, lab, m, lane);

  // ---- confidence: one lane, left to right, as np.cumprod(float32) does ----
  if (lane == 0) {
    const int np_ = mode == 1 ? keep_end : T;
    float conf = 0.f;
    if (np_ > 0) {
      conf = pr[0];
      for (int t = 1; t < np_; ++t) conf = conf * pr[t];
    }
    confidence[b] = conf;
    result[b * 4 + 0] = n;
    result[b * 4 + 1] = dist;
    result[b * 4 + 2] = dist == 0 ? 1 : 0;   // distance 0 <=> equal length and every token equal (-1 equals nothing)
    result[b * 4 + 3] = flagged;
  }
}

}  // namespace

MRN_EXPORT int mrn_greedy_score_f32(const int64_t* idx, const float* prob, int B, int T, const int32_t* label, const int32_t* label_len,
                                    int Lmax, const int32_t* canon, int C, int mode, int eos, int32_t* tokens, int32_t* result,
                                    float* confidence, void* stream) {
  MRN_CHECK_ARG(idx && prob && label_len && canon && tokens && result && confidence, "mrn_greedy_score_f32: bad operands");
  MRN_CHECK_ARG(B >= 0 && T >= 1 && T <= SCORE_MAX_T, "mrn_greedy_score_f32: T = %d outside 1..%d", T, SCORE_MAX_T);
  MRN_CHECK_ARG(Lmax >= 0 && Lmax <= SCORE_MAX_L && (label || Lmax == 0), "mrn_greedy_score_f32: Lmax = %d outside 0..%d", Lmax,
                SCORE_MAX_L);
  MRN_CHECK_ARG(C > 0 && (mode == 0 || mode == 1), "mrn_greedy_score_f32: C = %d, mode = %d", C, mode);
  if (B == 0) return MRN_OK;
  const dim3 grid((unsigned)((B + SCORE_ROWS - 1) / SCORE_ROWS)), block(256);
  if (Lmax <= 64)
    hipLaunchKernelGGL(greedy_score_kernel<1>, grid, block, 0, (hipStream_t)stream, idx, prob, B, T, label, label_len, Lmax, canon, C,
                       mode, eos, tokens, result, confidence);
  else
    hipLaunchKernelGGL(greedy_score_kernel<4>, grid, block, 0, (hipStream_t)stream, idx, prob, B, T, label, label_len, Lmax, canon, C,
                       mode, eos, tokens, result, confidence);
  MRN_LAUNCH_CHECK("greedy_score");
  return MRN_OK;
}
