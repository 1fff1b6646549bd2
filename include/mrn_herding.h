/* C ABI of libmrn_hip.so, herding exemplar selection for the rehearsal memory.  Bound by mrn_amd/_lib.py the same way as include/mrn_hip.h,
 * include/mrn_decode.h, include/mrn_attn_beam.h, include/mrn_lexicon.h, include/mrn_attn_lexicon.h, include/mrn_attn_score.h and
 * include/mrn_shortlist.h (prototypes parsed from this file, return code 0 = ok, mrn_last_error() for the message); a header of its own
 * because the tests pin the prototypes of the other seven. */
#ifndef MRN_HERDING_H
#define MRN_HERDING_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Herding features (mrn_amd/modules/herding.py states the algorithm, features_host restates this in float64): for each of the B samples
 * of feat [B][T][D] (DEVICE, fp32; element strides batch_stride and time_stride, the D values of a frame contiguous) the time mean,
 * divided by (its Euclidean norm + 1e-8), written to row row0 + b of the table F [N][D] (DEVICE, fp32, contiguous).  The mean and the
 * norm accumulate in fp32; an all-zero sample comes out all zeros.  The other rows of F are not touched.  One launch, one workgroup
 * per sample.
 * Limits (an error code, nothing is launched): 0 <= B, 1 <= T, 4 <= D <= 8192 with D % 4 = 0, 0 <= row0, row0 + B <= N <= 2^24,
 * strides >= 0, no null operand. */
int mrn_herding_features_f32(const float* feat, int B, int T, int D, int64_t batch_stride, int64_t time_stride, float* F, int N, int row0,
                             void* stream);

/* Bytes of device workspace mrn_herding_select_f32 needs for a table of N rows and D columns (mu and the two halves of the residual in
 * float64, the partial column sums of mu, the two halves of the partial minima, the squared norms and the exclusion marks); -1 outside
 * 1 <= N <= 2^24, 4 <= D <= 8192 with D % 4 = 0. */
int64_t mrn_herding_select_work_bytes(int N, int D);

/* Herding selection (iCaRL) of m of the N rows of F [N][D] (DEVICE, fp32, contiguous): mu = the column mean, r_1 = mu; at step
 * k = 1 ... m the pick is the unpicked row i that minimises d_i = ||f_i||^2 - 2 f_i . r_k, a tie to the lower row index, and
 * r_{k+1} = r_k + mu - f_i.  picks [m] (DEVICE, int32) holds the rows IN PICK ORDER, dist [m] (DEVICE, fp32) the minimised d of every
 * step.  csrc/herding.hip: mu and r are kept in float64 on the device and r is rounded to fp32 once per step, so a step's error is that
 * of one fp32 dot product however many steps ran; mu is reduced over a fixed partition in a fixed order and nothing uses float atomics,
 * so two calls on the same table return the same bits.  One launch per step and m + 4 launches in all, all enqueued on `stream` with no
 * host synchronisation between them; no launch waits on another workgroup.  The host form is mrn_amd/modules/herding.py::herding_host.
 * The features must be finite (the caller's to check).  work: work_bytes >= mrn_herding_select_work_bytes(N, D) bytes, 16-byte aligned,
 * contents undefined before and after.
 * Limits (an error code, nothing is launched): 1 <= m <= N <= 2^24, 4 <= D <= 8192 with D % 4 = 0 (a row is read in 16-byte loads; row
 * offsets are 64-bit), no null operand. */
int mrn_herding_select_f32(const float* F, int N, int D, int m, int32_t* picks, float* dist, void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
