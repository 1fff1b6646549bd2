/* C ABI of libmrn_hip.so, decoding part: the entry points that decode a head's logits into labels.  Bound by mrn_amd/_lib.py the
 * same way as include/mrn_hip.h (prototypes parsed from this file, return code 0 = ok, mrn_last_error() for the message); kept
 * beside it because tests/test_greedy_decode_cpu.py pins the number of prototypes in that header. */
#ifndef MRN_DECODE_H
#define MRN_DECODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* CTC prefix beam search on a CTC head's logits (extends test.py:211-219, the CTC branch of validation(): best path picks the most
 * likely alignment, this the most likely label), one wave per sample, one launch per batch.  logits: fp32 [B][T][C] with strides in
 * elements and a contiguous last dimension; class 0 is the blank.  W = beam width, K = cut-off: per frame only the min(K, C - 1)
 * non-blank classes of largest raw logit (ties to the lower class) extend a prefix.  The algorithm is restated in float64 by
 * mrn_amd/modules/decoding.py::ctc_beam_host.  Outputs, entries in descending total: tokens [B][W][T] (classes, 0 behind the
 * prefix), length [B][W] (-1 = dead slot), score [B][W] = log-probability of the label (-inf for a dead slot); for the best entry
 * path [B][T] = its classes with one blank between equal neighbours, blanks behind (greedy collapse gives the prefix back) and
 * prob [B][T] = {exp(score), 1, 1, ...}: the pair mrn_greedy_score_f32 takes in place of mrn_argmax_prob_f32's.
 * Limits (an error code, never a fault): 1 <= T <= 512, 2 <= C <= 65535, 1 <= W <= 16, 1 <= K <= 15. */
int mrn_ctc_beam_decode_f32(const float* logits, int64_t stride_b, int64_t stride_t, int B, int T, int C, int W, int K,
                            int32_t* tokens, int32_t* length, float* score, int64_t* path, float* prob, void* stream);

#ifdef __cplusplus
}
#endif
#endif
