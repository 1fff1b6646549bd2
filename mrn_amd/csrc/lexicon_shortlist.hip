// Lexicon shortlist: the K lexicon words nearest (unit-cost Levenshtein distance over class tokens) to one hypothesis per sample, the
// middle step of the CRNN lexicon protocol (Shi et al., section 3.3: transcribe lexicon-free, keep the words within a small edit
// distance, choose among them by the model's probability).  The definition is stated in mrn_amd/modules/decoding.py and restated in
// numpy by lexicon_shortlist_host there; everything is integer arithmetic, so the result is equal to the host's, not just close.
//
// Reference op sites: test.py:243-250 (edit_distance between a prediction and a word, unit costs), tools/utils.py:62-76 and 133-143
// (the class tokens both sides are spelled in).
//
// Two launches.
//
// 1. shortlist_distance_kernel, one thread per (sample, word), SL_SAMPLES samples per workgroup and tile of 256 words, so a tile of
//    the word table is read once per SL_SAMPLES samples.  Myers' bit-vector algorithm (Hyyro's edit-distance form) with the
//    hypothesis as the pattern: a hypothesis of at most 64 tokens is one machine word of state per (sample, word), 32 bits when every
//    sample of the group has at most 32 tokens (64-bit integer VALU is two 32-bit instructions per operation, the carry chain of the
//    add included).  A sample's match masks are a 128-slot open-addressing table (class, mask) in LDS, built once per workgroup by
//    one wave with LDS compare-and-swap: which slot a class lands in depends on the order the lanes' atomics land, the mask a
//    look-up returns does not.  A look-up is one 4-byte key read per probe and one 8-byte mask read; lanes with the same token read
//    the same address (a broadcast), lanes with different tokens hit the 32 banks at random, which costs a few LDS cycles beside the
//    ~40 VALU instructions of the step and needs no VALU at all -- a conflict-free scan of the table (every lane reads entry e, a
//    broadcast) costs four VALU instructions per distinct class of the hypothesis instead.  The tile's tokens are staged through
//    LDS 32 positions at a time, transposed ([position][word], rows padded by one dword so the transposing store is conflict-free)
//    and narrowed to 16 bits (classes go to 65 534).  The distances (at most max(64, 255) = 255) are stored as bytes, B x N of
//    them, and counted into a per-sample histogram: LDS integer atomics per workgroup, then one global integer atomic per non-empty
//    bin.  Integer sums do not depend on the order of their terms.
//
// 2. shortlist_select_kernel, one workgroup per sample.  The histogram's prefix sums give the cut distance dc (the smallest d with
//    at least K words at distance <= d, after the max_dist cut-off) and how many words of bin dc are taken.  One sweep over the
//    sample's bytes in index order, 4096 per step (16 per thread, one 16-byte load), with a workgroup scan of the two counts
//    (d < dc, d == dc): the words below the cut go to an LDS list in index order, the first `take` words of bin dc behind them.  The
//    at most 256 keys (d << 20 | w, all different) are then ranked by counting and written in (d, w) order.  No atomics here.
//
// Recomputing the distances in the second launch instead of storing the bytes would double the dominant cost (the Myers steps) to
// save N bytes of traffic per sample; the bytes are kept ("Lexicon shortlist", has the arithmetic and the times).
#include "common.hpp"

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_SAMPLES = 8;            // samples per workgroup of the distance kernel
constexpr int SL_SLOTS = 128;            // hash slots per sample: at most 64 keys, so a probe always ends at a free slot
constexpr int SL_CHUNK = 32;             // token positions staged per step
constexpr int SL_ROW = SL_THREADS + 2;   // 16-bit elements per staged row: 129 dwords
constexpr int SL_MAX_HYP = 64;
constexpr int SL_MAX_K = 256;
constexpr int SL_MAX_L = 255;
constexpr int SL_MAX_N = 1 << 20;
constexpr int SL_SWEEP = SL_THREADS * 16;

__device__ __forceinline__ int sl_hash(int c) { return (int)(((unsigned)c * 0x9E3779B1u) >> 25); }   // 7 bits

// the Myers steps of SL_CHUNK staged positions for this thread's word against the group's samples
template <typename W>
__device__ __forceinline__ void sl_steps(const unsigned short (*s_tok)[SL_ROW], const int (*s_key)[SL_SLOTS],
                                         const unsigned long long (*s_mask)[SL_SLOTS], const int (&n)[SL_SAMPLES], int count, W (&Pv)[SL_SAMPLES],
                                         W (&Mv)[SL_SAMPLES], int (&sc)[SL_SAMPLES]) {
  for (int c = 0; c < count; ++c) {
    const int t = s_tok[c][threadIdx.x];
    const int h = sl_hash(t);
#pragma unroll
    for (int s = 0; s < SL_SAMPLES; ++s) {
      if (n[s] <= 0) continue;          // (uniform: n lives in scalar registers)
      W eq = 0;
      int slot = h;
      for (int probe = 0; probe < SL_SLOTS; ++probe) {
        const int k = s_key[s][slot];
        if (k == t) {
          eq = (W)s_mask[s][slot];
          break;
        }
        if (k < 0) break;
        slot = (slot + 1) & (SL_SLOTS - 1);
      }
      const W top = (W)1 << (n[s] - 1);
      const W pv = Pv[s], mv = Mv[s];
      const W xv = eq | mv;
      const W xh = (((eq & pv) + pv) ^ pv) | eq;
      W ph = mv | ~(xh | pv);
      W mh = pv & xh;
      sc[s] += (ph & top) ? 1 : ((mh & top) ? -1 : 0);
      ph = (ph << 1) | (W)1;
      mh = mh << 1;
      Pv[s] = mh | ~(xv | ph);
      Mv[s] = ph & xv;
    }
  }
}

template <typename W>
__device__ __forceinline__ void sl_distances(const int32_t* __restrict__ lex_tokens, int Lmax, int N, int L, int tile_L,
                                             unsigned short (*s_tok)[SL_ROW], const int (*s_key)[SL_SLOTS],
                                             const unsigned long long (*s_mask)[SL_SLOTS], const int (&n)[SL_SAMPLES], int (&sc)[SL_SAMPLES]) {
  W Pv[SL_SAMPLES], Mv[SL_SAMPLES];
#pragma unroll
  for (int s = 0; s < SL_SAMPLES; ++s) {
    Pv[s] = ~(W)0;
    Mv[s] = 0;
    sc[s] = n[s] > 0 ? n[s] : 0;
  }
  const int w0 = blockIdx.x * SL_THREADS;
  for (int j0 = 0; j0 < tile_L; j0 += SL_CHUNK) {
    __syncthreads();                    // the previous chunk has been consumed
    for (int e = threadIdx.x; e < SL_THREADS * SL_CHUNK; e += SL_THREADS) {
      const int r = e >> 5, c = e & (SL_CHUNK - 1);      // 32 consecutive lanes read 32 consecutive positions of one word
      const int gw = w0 + r, p = j0 + c;
      const int v = (gw < N && p < Lmax) ? lex_tokens[(long)gw * Lmax + p] : 0;
      s_tok[c][r] = (unsigned short)v;
    }
    __syncthreads();
    sl_steps<W>(s_tok, s_key, s_mask, n, min(SL_CHUNK, L - j0), Pv, Mv, sc);
  }
}

__global__ __launch_bounds__(SL_THREADS) void shortlist_distance_kernel(const int32_t* __restrict__ hyp, int Hmax,
                                                                        const int32_t* __restrict__ hyp_len, int B,
                                                                        const int32_t* __restrict__ lex_tokens, int Lmax,
                                                                        const int32_t* __restrict__ lex_len, int N, int* __restrict__ hist,
                                                                        unsigned char* __restrict__ dist8, long row_bytes) {
  __shared__ int s_key[SL_SAMPLES][SL_SLOTS];
  __shared__ unsigned long long s_mask[SL_SAMPLES][SL_SLOTS];
  __shared__ unsigned short s_tok[SL_CHUNK][SL_ROW];
  __shared__ int s_hist[SL_SAMPLES][256];
  __shared__ int s_n[SL_SAMPLES];
  __shared__ int s_tile_L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.y * SL_SAMPLES;
  const int w = blockIdx.x * SL_THREADS + tid;

  for (int i = tid; i < SL_SAMPLES * SL_SLOTS; i += SL_THREADS) {
    (&s_key[0][0])[i] = -1;
    (&s_mask[0][0])[i] = 0ull;
  }
  for (int i = tid; i < SL_SAMPLES * 256; i += SL_THREADS) (&s_hist[0][0])[i] = 0;
  if (tid == 0) s_tile_L = 0;
  __syncthreads();

  // ---- the match masks of every sample of the group: wave v builds samples v, v + 4 ----
  for (int s = wave; s < SL_SAMPLES; s += SL_THREADS / 64) {
    const int b = b0 + s;
    int n = -1;                         // -1: not computed (past B, or left to the host)
    if (b < B) {
      const int len = hyp_len[b];
      if (len >= 0 && len <= SL_MAX_HYP) n = min(len, Hmax);
    }
    if (lane == 0) s_n[s] = n;
    if (lane < n) {
      const int t = hyp[(long)b * Hmax + lane];
      if (t >= 0) {                     // a negative token equals no class of any word
        int slot = sl_hash(t);
        for (int probe = 0; probe < SL_SLOTS; ++probe) {
          const int old = atomicCAS(&s_key[s][slot], -1, t);
          if (old == -1 || old == t) break;
          slot = (slot + 1) & (SL_SLOTS - 1);
        }
        atomicOr(&s_mask[s][slot], 1ull << lane);
      }
    }
  }
  const int L = w < N ? min(max(lex_len[w], 0), Lmax) : 0;
  atomicMax(&s_tile_L, L);
  __syncthreads();

  int n[SL_SAMPLES], sc[SL_SAMPLES];
  int longest = 0;
#pragma unroll
  for (int s = 0; s < SL_SAMPLES; ++s) {
    n[s] = __builtin_amdgcn_readfirstlane(s_n[s]);
    longest = max(longest, n[s]);
  }
  const int tile_L = longest > 0 ? s_tile_L : 0;      // hypotheses all empty: the distance is the word's length, no step runs
  if (longest <= 32)
    sl_distances<unsigned>(lex_tokens, Lmax, N, L, tile_L, s_tok, s_key, s_mask, n, sc);
  else
    sl_distances<unsigned long long>(lex_tokens, Lmax, N, L, tile_L, s_tok, s_key, s_mask, n, sc);

#pragma unroll
  for (int s = 0; s < SL_SAMPLES; ++s) {
    if (n[s] < 0 || w >= N) continue;
    const int d = min(max(n[s] == 0 ? L : sc[s], 0), 255);
    dist8[(long)(b0 + s) * row_bytes + w] = (unsigned char)d;
    atomicAdd(&s_hist[s][d], 1);
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SL_SAMPLES; ++s) {
    if (n[s] < 0) continue;
    const int c = s_hist[s][tid];
    if (c) atomicAdd(&hist[(long)(b0 + s) * 256 + tid], c);
  }
}

// inclusive prefix of v over the workgroup's 256 threads in thread order, and the total; s_part holds 4 ints
__device__ __forceinline__ int sl_block_scan(int v, int* s_part, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off);
    if (lane >= off) v += u;
  }
  __syncthreads();                      // the previous call's reads of s_part are done
  if (lane == 63) s_part[wave] = v;
  __syncthreads();
  int add = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < SL_THREADS / 64; ++i) {
    const int p = s_part[i];
    if (i < wave) add += p;
    total += p;
  }
  return v + add;
}

__global__ __launch_bounds__(SL_THREADS) void shortlist_select_kernel(const int32_t* __restrict__ hyp_len, int N, int K, int max_dist,
                                                                      const int* __restrict__ hist, const unsigned char* __restrict__ dist8,
                                                                      long row_bytes, int32_t* __restrict__ cand, int32_t* __restrict__ dist,
                                                                      int32_t* __restrict__ flag) {
  __shared__ int s_cum[256];
  __shared__ int s_part[SL_THREADS / 64];
  __shared__ unsigned s_sel[SL_MAX_K];
  __shared__ int s_cut, s_below;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  int32_t* cb = cand + (long)b * K;
  int32_t* db = dist + (long)b * K;
  const int len = hyp_len[b];
  if (len < 0 || len > SL_MAX_HYP) {    // (uniform) left to the host
    for (int k = tid; k < K; k += SL_THREADS) {
      cb[k] = -1;
      db[k] = -1;
    }
    if (tid == 0) flag[b] = 1;
    return;
  }
  // ---- the cut distance ----
  int total;
  const int mine = (max_dist >= 0 && tid > max_dist) ? 0 : hist[(long)b * 256 + tid];
  const int cum = sl_block_scan(mine, s_part, total);
  const int want = min(K, total);
  s_cum[tid] = cum;
  if (tid == 0) {
    s_cut = 0;
    s_below = 0;
  }
  __syncthreads();
  if (want > 0 && cum >= want && cum - mine < want) {   // exactly one thread: the prefix sums do not decrease
    s_cut = tid;
    s_below = cum - mine;
  }
  __syncthreads();
  const int cut = s_cut, below = s_below;               // below < want <= K
  const int take = want - below;                        // words of bin `cut` that are kept, lowest indices first
  // ---- one sweep in index order ----
  const unsigned char* row = dist8 + (long)b * row_bytes;
  int run_a = 0, run_b = 0;
  for (int base = 0; base < N && want > 0; base += SL_SWEEP) {
    const int i0 = base + tid * 16;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i0 < N) v = *reinterpret_cast<const uint4*>(row + i0);      // row_bytes is a multiple of 16 that covers N
    const unsigned q4[4] = {v.x, v.y, v.z, v.w};
    int cnt_a = 0, cnt_b = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int d = (int)((q4[q >> 2] >> (8 * (q & 3))) & 0xffu);
      const bool in = i0 + q < N;
      cnt_a += (in && d < cut) ? 1 : 0;
      cnt_b += (in && d == cut) ? 1 : 0;
    }
    int tot;
    const int inc = sl_block_scan(cnt_a | (cnt_b << 16), s_part, tot);      // at most 4096 of either: the halves do not meet
    int pos_a = run_a + ((inc & 0xffff) - cnt_a), pos_b = run_b + ((inc >> 16) - cnt_b);
    if (cnt_a | cnt_b) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int d = (int)((q4[q >> 2] >> (8 * (q & 3))) & 0xffu);
        const bool in = i0 + q < N;
        const unsigned key = ((unsigned)d << 20) | (unsigned)(i0 + q);
        if (in && d < cut) {
          if (pos_a < below) s_sel[pos_a] = key;
          ++pos_a;
        } else if (in && d == cut) {
          if (pos_b < take) s_sel[below + pos_b] = key;
          ++pos_b;
        }
      }
    }
    run_a += tot & 0xffff;
    run_b += tot >> 16;
    if (run_a >= below && run_b >= take) break;         // (uniform) every kept word has been seen
  }
  __syncthreads();
  // ---- rank the kept keys (all different) by counting, write in (d, w) order ----
  if (tid < want) {
    const unsigned key = s_sel[tid];
    int rank = 0;
    for (int j = 0; j < want; ++j) rank += s_sel[j] < key ? 1 : 0;
    cb[rank] = (int32_t)(key & 0xfffffu);
    db[rank] = (int32_t)(key >> 20);
  }
  for (int k = want + tid; k < K; k += SL_THREADS) {
    cb[k] = -1;
    db[k] = -1;
  }
  if (tid == 0) flag[b] = 0;
}

long sl_row_bytes(int N) { return ((long)N + 15) & ~15L; }

}  // namespace

MRN_EXPORT int64_t mrn_lexicon_shortlist_work_bytes(int B, int N) {
  if (B < 0 || N < 1 || N > SL_MAX_N) return -1;
  return (int64_t)B * 256 * 4 + (int64_t)B * sl_row_bytes(N);
}

MRN_EXPORT int mrn_lexicon_shortlist_i32(const int32_t* hyp, int Hmax, const int32_t* hyp_len, int B, const int32_t* lex_tokens, int Lmax,
                                         const int32_t* lex_len, int N, int K, int max_dist, int32_t* cand, int32_t* dist, int32_t* flag,
                                         void* work, int64_t work_bytes, void* stream) {
  MRN_CHECK_ARG(hyp_len && lex_tokens && lex_len && cand && dist && flag && work, "mrn_lexicon_shortlist_i32: bad operands");
  MRN_CHECK_ARG(Hmax >= 0 && (hyp || Hmax == 0), "mrn_lexicon_shortlist_i32: Hmax = %d without hypotheses", Hmax);
  MRN_CHECK_ARG(K >= 1 && K <= SL_MAX_K, "mrn_lexicon_shortlist_i32: K = %d outside 1..%d", K, SL_MAX_K);
  MRN_CHECK_ARG(N >= 1 && N <= SL_MAX_N, "mrn_lexicon_shortlist_i32: N = %d outside 1..2^20", N);
  MRN_CHECK_ARG(Lmax >= 1 && Lmax <= SL_MAX_L, "mrn_lexicon_shortlist_i32: Lmax = %d outside 1..%d", Lmax, SL_MAX_L);
  MRN_CHECK_ARG(B >= 0 && max_dist >= -1, "mrn_lexicon_shortlist_i32: B = %d, max_dist = %d", B, max_dist);
  if (work_bytes < mrn_lexicon_shortlist_work_bytes(B, N)) {
    mrn_set_error("mrn_lexicon_shortlist_i32: %lld bytes of workspace, %lld needed", (long long)work_bytes,
                  (long long)mrn_lexicon_shortlist_work_bytes(B, N));
    return MRN_ERR_WORKSPACE;
  }
  if (B == 0) return MRN_OK;
  int* hist = (int*)work;
  unsigned char* dist8 = (unsigned char*)work + (size_t)B * 256 * 4;
  const long row_bytes = sl_row_bytes(N);
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * 256 * 4, (hipStream_t)stream);
  if (e != hipSuccess) {
    mrn_set_error("mrn_lexicon_shortlist_i32: clearing the histogram failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  const dim3 grid((unsigned)ceil_div(N, SL_THREADS), (unsigned)ceil_div(B, SL_SAMPLES));
  hipLaunchKernelGGL(shortlist_distance_kernel, grid, dim3(SL_THREADS), 0, (hipStream_t)stream, hyp, Hmax, hyp_len, B, lex_tokens, Lmax,
                     lex_len, N, hist, dist8, row_bytes);
  MRN_LAUNCH_CHECK("shortlist_distance");
  hipLaunchKernelGGL(shortlist_select_kernel, dim3((unsigned)B), dim3(SL_THREADS), 0, (hipStream_t)stream, hyp_len, N, K, max_dist,
                     (const int*)hist, (const unsigned char*)dist8, row_bytes, cand, dist, flag);
  MRN_LAUNCH_CHECK("shortlist_select");
  return MRN_OK;
}
