/* C ABI of libmrn_hip.so, beam-search decoding on the attention head.  Bound by mrn_amd/_lib.py the same way as include/mrn_hip.h and
 * include/mrn_decode.h (prototypes parsed from this file, return code 0 = ok, mrn_last_error() for the message); a header of its own
 * because the tests pin the number of prototypes in the other two. */
#ifndef MRN_ATTN_BEAM_H
#define MRN_ATTN_BEAM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Beam search on the attention head (extends the greedy loop of modules/prediction.py:70-86: W entries per sample instead of the one
 * arg-max), all S steps of `groups` experts of one geometry (B, T, D, S) in one launch per eight experts (csrc/attn_decode.hip attn_beam_kernel,
 * exact-fp32 form).  The algorithm is stated in mrn_amd/modules/decoding.py and restated in float64 by attn_beam_host there.  The
 * operands are those of mrn_attn_greedy_decode_grouped_f32: every pointer argument but start_token is a HOST array of `groups` device
 * pointers, num_class a host array of `groups` class counts.  eos = the end token, W = the beam width.  scratch[g]: scratch_floats
 * floats, at least ceil(B / (16 / W)) * 16 * (16 * ceil(num_class[g] / 16) + 3 * S) (a step's logits and the history records).
 * Outputs per group, entries in descending score: tokens int32 [B][W][S] (eos behind the first eos), length int32 [B][W] (tokens up
 * to and including eos, S for an entry that never finished, -1 = dead slot), score fp32 [B][W] (-inf for a dead slot), logp fp32
 * [B][W][S] (0 behind the first eos); for the best entry path int64 [B][S] and prob fp32 [B][S] = exp(logp): the pair
 * mrn_greedy_score_f32 takes in place of mrn_argmax_prob_f32's.
 * Limits (an error code, nothing is launched): 1 <= W <= 16, 1 <= S <= 512, num_class >= 2, 0 <= eos < num_class, hidden = 256, D a
 * multiple of 16 whose whole-context tile fits the LDS budget: 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + 3584 <= 160 KiB. */
int mrn_attn_beam_decode_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                     const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                     const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                     const void* const* b_hh, const void* const* w_gen, const void* const* b_gen, const int* num_class,
                                     int eos, int W, const void* const* scratch, int64_t scratch_floats, const void* const* tokens,
                                     const void* const* length, const void* const* score, const void* const* logp,
                                     const void* const* path, const void* const* prob, int groups, int B, int T, int D, int S, int hidden,
                                     void* stream);

/* The same (modules/prediction.py:70-86) with the recurrent products and the generator as split-fp16 x3: the fp16 hi / lo streams and
 * w_inv (device float[4] per group: h2h, ih, hh, generator) of mrn_attn_greedy_decode_x3_grouped.
 * Limits (an error code, nothing is launched): 1 <= W <= 16, 1 <= S <= 512, num_class >= 2, 0 <= eos < num_class, hidden = 256, D a
 * multiple of 32 whose whole-context tile fits the LDS budget: the sum above + 1024 <= 160 KiB. */
int mrn_attn_beam_decode_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                    const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                    const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                    const void* const* w_inv, const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                    const int* num_class, int eos, int W, const void* const* scratch, int64_t scratch_floats,
                                    const void* const* tokens, const void* const* length, const void* const* score,
                                    const void* const* logp, const void* const* path, const void* const* prob, int groups, int B, int T,
                                    int D, int S, int hidden, void* stream);

#ifdef __cplusplus
}
#endif
#endif
