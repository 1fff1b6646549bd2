// Herding exemplar selection for the rehearsal memory (iCaRL, Rebuffi et al. 2017, algorithm 4), per task.  The algorithm is stated in
// mrn_amd/modules/herding.py and restated in float64 numpy by features_host / herding_host there.
//
// Reference op sites: il_modules/base.py:278-302 (build_rehearsal_memory: the memory of a finished task is drawn with np.random.choice;
// its comment "Calculate the means of old classes with newly trained network" is the herding routine's) and data/data_manage.py
// (rehearsal_prev_model: the ordered loader over the previous task's data the features are computed from).
//
// herding_features_kernel, one workgroup per sample: thread j sums column j of the sample's [T][D] feature over time (coalesced, fp32),
// keeps the mean in LDS, the workgroup sums the squares, and every mean is divided by (norm + 1e-8) on its way to the table.
//
// The selection takes m sequential picks, each a matrix-vector product over the whole table; the table stays where it is and only the
// D values of the residual r change between picks.  mu and r live in float64 on the device (D values, updated once per step) and r is
// rounded to fp32 once per step for the products: the error of a step is that of one fp32 dot product however many steps ran.
//
//   herd_mu_partial_kernel + herd_mu_finish_kernel: the column sums over HERD_MU_PARTS fixed row ranges, then over the ranges in index
//     order, in float64.  No atomics: the same table gives the same mu, bit for bit.
//   herd_norms_kernel: ||f_i||^2 in fp32 and the cleared exclusion marks.
//   herd_step_kernel, ONE launch per step, and one closing launch of a single workgroup.  Launch k (0-based) scores step k + 1.  It
//     begins, in EVERY workgroup, by reducing the at most HERD_MAX_GROUPS partial (d, row) pairs launch k - 1 left in the workspace, so
//     every workgroup knows pick k; it forms r_{k+1} = r_k + mu - f_pick in float64 from r_k (the half of a double buffer launch k - 1
//     wrote), rounds it into LDS, and workgroup 0 alone writes picks / dist of step k, r_{k+1} into the other half and the row's
//     exclusion mark.  The other workgroups exclude that row by comparison: the mark is only guaranteed visible from the next launch
//     on.  Then the workgroups split the rows; a row is shared by the smallest power of two of lanes that covers its 16-byte chunks
//     (at most a wave, which then loops), each lane multiplies its chunks with r in LDS, the lanes of the row add up by shuffles, and
//     the workgroup reduces its rows to one (d, row) pair under the tie rule (smaller d, then lower row) and writes it to the half
//     of the partial buffer this launch owns.
//
// No launch waits on another workgroup: the kernel boundary is the only synchronisation (no cooperative launch, no grid barrier, no
// flag or ticket).  The choice against a fence-and-ticket finish inside one launch: the last-arriver form costs every workgroup a
// device-scope fence per step (microseconds each, m of them in sequence) where a dependent launch on the same stream costs about one
// and a half, and wgrad_operands.hip records what the same pattern did to a pass of this library.
#include "common.hpp"

namespace {

constexpr int HERD_THREADS = 256;
constexpr int HERD_WAVES = HERD_THREADS / 64;
constexpr int HERD_MAX_N = 1 << 24;
constexpr int HERD_MIN_D = 4;
constexpr int HERD_MAX_D = 8192;
constexpr int HERD_MAX_GROUPS = 1024;     // workgroups of a step launch = partial pairs the next launch reduces
constexpr int HERD_GROUP_ROWS = 32;       // a workgroup scores at least this many rows (but for the last one)
constexpr int HERD_MU_PARTS = 128;        // fixed row ranges of the column sums
constexpr int HERD_UNROLL = 8;            // rows in flight per lane group
constexpr float HERD_EPS = 1e-8f;
constexpr float HERD_INF = __builtin_inff();

struct HerdPair {
  float d;
  int row;
};

__device__ __forceinline__ bool herd_less(float d2, int i2, float d, int i) { return d2 < d || (d2 == d && i2 < i); }

__device__ __forceinline__ void herd_wave_min(float& d, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float d2 = __shfl_xor(d, o);
    const int i2 = __shfl_xor(i, o);
    if (herd_less(d2, i2, d, i)) {
      d = d2;
      i = i2;
    }
  }
}

// the minimum pair of the workgroup under the tie rule, known to every thread afterwards; s_d / s_i hold HERD_WAVES entries
__device__ __forceinline__ void herd_block_min(float& d, int& i, float* s_d, int* s_i) {
  herd_wave_min(d, i);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    s_d[w] = d;
    s_i[w] = i;
  }
  __syncthreads();
  d = s_d[0];
  i = s_i[0];
#pragma unroll
  for (int k = 1; k < HERD_WAVES; ++k)
    if (herd_less(s_d[k], s_i[k], d, i)) {
      d = s_d[k];
      i = s_i[k];
    }
}

// sum over the lpr lanes (a power of two, a lane group aligned to it) that share a row
__device__ __forceinline__ float herd_group_sum(float v, int lpr) {
  for (int o = lpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void __launch_bounds__(HERD_THREADS) herding_features_kernel(const float* __restrict__ feat, int T, int D, long batch_stride,
                                                                        long time_stride, float* __restrict__ F, int row0) {
  extern __shared__ __attribute__((aligned(16))) char herd_smem[];
  float* s_mean = (float*)herd_smem;                 // [D]
  float* s_red = s_mean + D;                         // [HERD_WAVES]
  const float* src = feat + (size_t)blockIdx.x * batch_stride;
  const float inv_t = 1.f / (float)T;
  float sq = 0.f;
  for (int j = threadIdx.x; j < D; j += HERD_THREADS) {
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += src[(size_t)t * time_stride + j];
    const float mean = s * inv_t;
    s_mean[j] = mean;
    sq = fmaf(mean, mean, sq);
  }
  const float total = block_sum<HERD_THREADS>(sq, s_red);
  const float denom = sqrtf(total) + HERD_EPS;
  float* dst = F + ((size_t)row0 + blockIdx.x) * D;
  for (int j = threadIdx.x; j < D; j += HERD_THREADS) dst[j] = s_mean[j] / denom;      // (each thread reads back its own means)
}

// part[p][j] = sum of column j over the rows of range p, in row order
__global__ void __launch_bounds__(HERD_THREADS) herd_mu_partial_kernel(const float* __restrict__ F, int N, int D, int rows_per_part,
                                                                       double* __restrict__ part) {
  const int j = blockIdx.y * HERD_THREADS + threadIdx.x;
  if (j >= D) return;
  const long i0 = (long)blockIdx.x * rows_per_part;
  const long i1 = i0 + rows_per_part < (long)N ? i0 + rows_per_part : (long)N;
  double s = 0.0;
  for (long i = i0; i < i1; ++i) s += (double)F[(size_t)i * D + j];
  part[(size_t)blockIdx.x * D + j] = s;
}

__global__ void __launch_bounds__(HERD_THREADS) herd_mu_finish_kernel(const double* __restrict__ part, int parts, int N, int D,
                                                                      double* __restrict__ mu, double* __restrict__ r0) {
  const int j = blockIdx.x * HERD_THREADS + threadIdx.x;
  if (j >= D) return;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += part[(size_t)p * D + j];
  s /= (double)N;
  mu[j] = s;
  r0[j] = s;                                           // r_1 = mu
}

__global__ void __launch_bounds__(HERD_THREADS) herd_norms_kernel(const float* __restrict__ F, int N, int D, int lpr, float* __restrict__ norms,
                                                                  unsigned char* __restrict__ taken) {
  const int chunks = D >> 2;
  const int lane = threadIdx.x & 63, sub = lane & (lpr - 1);
  const int rows_per_wave = 64 / lpr;
  const long row = ((long)blockIdx.x * HERD_WAVES + (threadIdx.x >> 6)) * rows_per_wave + lane / lpr;
  float acc = 0.f;
  if (row < N) {
    const f32x4* f = (const f32x4*)(F + (size_t)row * D);
    for (int c = sub; c < chunks; c += lpr) {
      const f32x4 v = f[c];
      acc = fmaf(v.x, v.x, acc);
      acc = fmaf(v.y, v.y, acc);
      acc = fmaf(v.z, v.z, acc);
      acc = fmaf(v.w, v.w, acc);
    }
  }
  acc = herd_group_sum(acc, lpr);
  if (row < N && sub == 0) {
    norms[row] = acc;
    taken[row] = 0;
  }
}

// launch k of the selection (see the head of the file).  prev_groups: the pairs launch k - 1 wrote (0 in launch 0); score = 0 in the
// closing launch, which only records the last pick
__global__ void __launch_bounds__(HERD_THREADS) herd_step_kernel(const float* __restrict__ F, int N, int D, int lpr, int rows_per_group,
                                                                 const float* __restrict__ norms, unsigned char* taken,
                                                                 const double* __restrict__ mu, const double* __restrict__ r_in,
                                                                 double* __restrict__ r_out, const HerdPair* __restrict__ prev, int prev_groups,
                                                                 HerdPair* __restrict__ next, int k, int score, int32_t* __restrict__ picks,
                                                                 float* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) char herd_smem[];
  float* s_r = (float*)herd_smem;                     // [D], 16-byte aligned
  float* s_d = s_r + D;                               // [HERD_WAVES]
  int* s_i = (int*)(s_d + HERD_WAVES);                // [HERD_WAVES]
  const int tid = threadIdx.x;
  int pick = -1;
  if (prev_groups > 0) {
    // ---- pick k of the previous launch: the minimum of its partial pairs, in every workgroup ----
    float d = HERD_INF;
    int i = 0x7fffffff;
    for (int g = tid; g < prev_groups; g += HERD_THREADS) {
      const HerdPair p = prev[g];
      if (herd_less(p.d, p.row, d, i)) {
        d = p.d;
        i = p.row;
      }
    }
    herd_block_min(d, i, s_d, s_i);
    pick = i < N ? i : N - 1;                          // (m <= N: some group always had an unpicked row; the clamp only guards the reads)
    const float* f = F + (size_t)pick * D;
    for (int j = tid; j < D; j += HERD_THREADS) {
      const double rn = r_in[j] + mu[j] - (double)f[j];
      s_r[j] = (float)rn;
      if (blockIdx.x == 0) r_out[j] = rn;
    }
    if (blockIdx.x == 0 && tid == 0) {
      picks[k - 1] = pick;
      dist[k - 1] = d;
      taken[pick] = 1;
    }
  } else {
    for (int j = tid; j < D; j += HERD_THREADS) s_r[j] = (float)r_in[j];
  }
  if (!score) return;
  __syncthreads();
  // ---- d_i = ||f_i||^2 - 2 f_i . r of this workgroup's rows ----
  const int chunks = D >> 2;
  const int lane = tid & 63, sub = lane & (lpr - 1);
  const int rows_per_wave = 64 / lpr;
  const int rows_per_pass = HERD_WAVES * rows_per_wave;
  const long b0 = (long)blockIdx.x * rows_per_group;
  const long b1 = b0 + rows_per_group < (long)N ? b0 + rows_per_group : (long)N;
  const long mine = b0 + (long)(tid >> 6) * rows_per_wave + lane / lpr;
  const f32x4* r4 = (const f32x4*)s_r;
  float best = HERD_INF;
  int best_row = 0x7fffffff;
  for (long base = 0; b0 + base < b1; base += (long)rows_per_pass * HERD_UNROLL) {     // (uniform over the workgroup)
    float acc[HERD_UNROLL];
    long row[HERD_UNROLL];
#pragma unroll
    for (int u = 0; u < HERD_UNROLL; ++u) {
      row[u] = mine + base + (long)u * rows_per_pass;
      acc[u] = 0.f;
    }
    for (int c = sub; c < chunks; c += lpr) {
      const f32x4 rv = r4[c];
#pragma unroll
      for (int u = 0; u < HERD_UNROLL; ++u) {
        if (row[u] < b1) {
          const f32x4 v = ((const f32x4*)(F + (size_t)row[u] * D))[c];
          acc[u] = fmaf(v.x, rv.x, acc[u]);
          acc[u] = fmaf(v.y, rv.y, acc[u]);
          acc[u] = fmaf(v.z, rv.z, acc[u]);
          acc[u] = fmaf(v.w, rv.w, acc[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < HERD_UNROLL; ++u) {
      const float dot = herd_group_sum(acc[u], lpr);
      if (row[u] < b1) {
        const int i = (int)row[u];
        float d = fmaf(-2.f, dot, norms[i]);
        if (!(d < HERD_INF)) d = HERD_INF;             // (an overflow or a NaN still loses to every finite d and keeps its row)
        if (i != pick && !taken[i] && herd_less(d, i, best, best_row)) {
          best = d;
          best_row = i;
        }
      }
    }
  }
  herd_block_min(best, best_row, s_d, s_i);
  if (tid == 0) {
    HerdPair p;
    p.d = best;
    p.row = best_row;
    next[blockIdx.x] = p;
  }
}

int herd_lanes_per_row(int D) {
  int lpr = 1;
  while (lpr < D / 4 && lpr < 64) lpr <<= 1;
  return lpr;
}
int herd_groups(int N) {
  const int g = ceil_div(N, HERD_GROUP_ROWS);
  return g < HERD_MAX_GROUPS ? g : HERD_MAX_GROUPS;
}
int herd_mu_parts(int N) {
  const int p = ceil_div(N, 128);
  return p < HERD_MU_PARTS ? p : HERD_MU_PARTS;
}
int64_t herd_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
bool herd_dims_ok(int N, int D) { return N >= 1 && N <= HERD_MAX_N && D >= HERD_MIN_D && D <= HERD_MAX_D && D % 4 == 0; }

struct HerdWork {
  int64_t mu, r, part, pairs, norms, taken, total;
};
HerdWork herd_layout(int N, int D) {
  HerdWork w;
  int64_t at = 0;
  w.mu = at;
  at = herd_align(at + (int64_t)D * 8);
  w.r = at;
  at = herd_align(at + (int64_t)D * 16);
  w.part = at;
  at = herd_align(at + (int64_t)herd_mu_parts(N) * D * 8);
  w.pairs = at;
  at = herd_align(at + (int64_t)2 * HERD_MAX_GROUPS * sizeof(HerdPair));
  w.norms = at;
  at = herd_align(at + (int64_t)N * 4);
  w.taken = at;
  at = herd_align(at + (int64_t)N);
  w.total = at;
  return w;
}

}  // namespace

MRN_EXPORT int mrn_herding_features_f32(const float* feat, int B, int T, int D, int64_t batch_stride, int64_t time_stride, float* F, int N,
                                        int row0, void* stream) {
  MRN_CHECK_ARG(feat && F, "mrn_herding_features_f32: bad operands");
  MRN_CHECK_ARG(B >= 0 && T >= 1, "mrn_herding_features_f32: B = %d, T = %d", B, T);
  MRN_CHECK_ARG(herd_dims_ok(N, D), "mrn_herding_features_f32: a table of N = %d rows (1..2^24) and D = %d columns (4..%d, D %% 4 = 0)", N, D,
                HERD_MAX_D);
  MRN_CHECK_ARG(row0 >= 0 && (int64_t)row0 + B <= N, "mrn_herding_features_f32: rows %d..%d outside a table of %d", row0, row0 + B, N);
  MRN_CHECK_ARG(batch_stride >= 0 && time_stride >= 0, "mrn_herding_features_f32: negative strides");
  if (B == 0) return MRN_OK;
  const size_t lds = (size_t)D * 4 + HERD_WAVES * 4;
  hipLaunchKernelGGL(herding_features_kernel, dim3((unsigned)B), dim3(HERD_THREADS), lds, (hipStream_t)stream, feat, T, D, (long)batch_stride,
                     (long)time_stride, F, row0);
  MRN_LAUNCH_CHECK("herding_features");
  return MRN_OK;
}

MRN_EXPORT int64_t mrn_herding_select_work_bytes(int N, int D) {
  if (!herd_dims_ok(N, D)) return -1;
  return herd_layout(N, D).total;
}

MRN_EXPORT int mrn_herding_select_f32(const float* F, int N, int D, int m, int32_t* picks, float* dist, void* work, int64_t work_bytes,
                                      void* stream) {
  MRN_CHECK_ARG(F && picks && dist && work, "mrn_herding_select_f32: bad operands");
  MRN_CHECK_ARG(herd_dims_ok(N, D), "mrn_herding_select_f32: a table of N = %d rows (1..2^24) and D = %d columns (4..%d, D %% 4 = 0)", N, D,
                HERD_MAX_D);
  MRN_CHECK_ARG(m >= 1 && m <= N, "mrn_herding_select_f32: m = %d outside 1..N = %d", m, N);
  const HerdWork w = herd_layout(N, D);
  if (work_bytes < w.total) {
    mrn_set_error("mrn_herding_select_f32: %lld bytes of workspace, %lld needed", (long long)work_bytes, (long long)w.total);
    return MRN_ERR_WORKSPACE;
  }
  char* base = (char*)work;
  double* mu = (double*)(base + w.mu);
  double* r = (double*)(base + w.r);
  double* part = (double*)(base + w.part);
  HerdPair* pairs = (HerdPair*)(base + w.pairs);
  float* norms = (float*)(base + w.norms);
  unsigned char* taken = (unsigned char*)(base + w.taken);
  hipStream_t s = (hipStream_t)stream;
  const int parts = herd_mu_parts(N), lpr = herd_lanes_per_row(D), groups = herd_groups(N);
  const int rows_per_part = ceil_div(N, parts), rows_per_group = ceil_div(N, groups);
  const int rows_per_block = HERD_WAVES * (64 / lpr);
  hipLaunchKernelGGL(herd_mu_partial_kernel, dim3((unsigned)parts, (unsigned)ceil_div(D, HERD_THREADS)), dim3(HERD_THREADS), 0, s, F, N, D,
                     rows_per_part, part);
  MRN_LAUNCH_CHECK("herd_mu_partial");
  hipLaunchKernelGGL(herd_mu_finish_kernel, dim3((unsigned)ceil_div(D, HERD_THREADS)), dim3(HERD_THREADS), 0, s, (const double*)part, parts, N, D,
                     mu, r);
  MRN_LAUNCH_CHECK("herd_mu_finish");
  hipLaunchKernelGGL(herd_norms_kernel, dim3((unsigned)ceil_div(N, rows_per_block)), dim3(HERD_THREADS), 0, s, F, N, D, lpr, norms, taken);
  MRN_LAUNCH_CHECK("herd_norms");
  const size_t lds = (size_t)D * 4 + HERD_WAVES * 8;
  for (int k = 0; k <= m; ++k) {
    // launch k reads r_k from half (k - 1) & 1 (launch 0: r_1 = mu in half 0) and the pairs of half (k - 1) & 1, writes halves k & 1
    const int in = k == 0 ? 0 : (k - 1) & 1, out = k & 1;
    const int score = k < m ? 1 : 0;
    hipLaunchKernelGGL(herd_step_kernel, dim3((unsigned)(score ? groups : 1)), dim3(HERD_THREADS), lds, s, F, N, D, lpr, rows_per_group,
                       (const float*)norms, taken, (const double*)mu, (const double*)(r + (size_t)in * D), r + (size_t)out * D,
                       (const HerdPair*)(pairs + (size_t)in * HERD_MAX_GROUPS), k == 0 ? 0 : groups, pairs + (size_t)out * HERD_MAX_GROUPS, k, score,
                       picks, dist);
    MRN_LAUNCH_CHECK("herd_step");
  }
  return MRN_OK;
}
