/* C ABI of libmrn_hip.so, exact scoring of per-sample candidate words on the attention head.  Bound by mrn_amd/_lib.py the same way as
 * include/mrn_hip.h, include/mrn_decode.h, include/mrn_attn_beam.h, include/mrn_lexicon.h and include/mrn_attn_lexicon.h (prototypes
 * parsed from this file, return code 0 = ok, mrn_last_error() for the message); a header of its own because the tests pin the
 * prototypes of the other five. */
#ifndef MRN_ATTN_SCORE_H
#define MRN_ATTN_SCORE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* log p(word, eos | sample) of every candidate word of every sample, each (sample, slot) pair a teacher-forced roll-out of the
 * attention decoder (extends the greedy loop of modules/prediction.py:70-86: the fed-back token is the word's next class instead of
 * the arg-max), all steps of `groups` experts of one geometry (B, T, D, S) in one launch per eight experts (csrc/attn_decode.hip
 * attn_score_kernel, exact-fp32 form).  The algorithm is stated in mrn_amd/modules/decoding.py and restated in float64 by
 * attn_candidates_host there.  The operands up to num_class are those of mrn_attn_greedy_decode_grouped_f32.  The word table and the
 * candidate table, shared by the groups, are DEVICE arrays of int32: lex_tokens [N][Lmax] (classes of word w in its first lex_len[w]
 * places), lex_len [N], cand [B][K] = the word of slot k of sample b, -1 for an unused slot.  Outputs per group: score_all fp32
 * [B][K], and logp fp32 [B][K][S] where the HOST array logp is not NULL: the log-probability of every class of the word and of its
 * eos, 0 behind.  A slot is dead (score -inf, logp 0) when it is unused, when a class of its word is not below the group's num_class,
 * or when its score is -inf or NaN.  The kernel clamps a length to min(Lmax, S - 1) and treats a word index outside 0 ... N - 1 as
 * unused; the caller checks the tables (mrn_amd/ops.py attn_score_candidates_grouped).
 * Limits (an error code, nothing is launched): 1 <= S <= 512, 2 <= num_class <= 65535, 0 <= eos < num_class, hidden = 256,
 * 1 <= N <= 2^20, K >= 1, Lmax >= 0, D a multiple of 16 whose whole-context tile fits the LDS budget:
 * 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + 2368 <= 160 KiB. */
int mrn_attn_score_candidates_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                          const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                          const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                          const void* const* b_hh, const void* const* w_gen, const void* const* b_gen, const int* num_class,
                                          int eos, const int32_t* lex_tokens, int Lmax, const int32_t* lex_len, int N, const int32_t* cand,
                                          int K, const void* const* score_all, const void* const* logp, int groups, int B, int T, int D,
                                          int S, int hidden, void* stream);

/* The same (modules/prediction.py:70-86) with the recurrent products and the generator as split-fp16 x3: the fp16 hi / lo streams and
 * w_inv (device float[4] per group: h2h, ih, hh, generator) of mrn_attn_greedy_decode_x3_grouped.
 * Limits (an error code, nothing is launched): 1 <= S <= 512, 2 <= num_class <= 65535, 0 <= eos < num_class, hidden = 256,
 * 1 <= N <= 2^20, K >= 1, Lmax >= 0, D a multiple of 32 whose whole-context tile fits the LDS budget: the sum above + 1024 <= 160 KiB. */
int mrn_attn_score_candidates_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                         const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                         const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                         const void* const* w_inv, const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                         const int* num_class, int eos, const int32_t* lex_tokens, int Lmax, const int32_t* lex_len, int N,
                                         const int32_t* cand, int K, const void* const* score_all, const void* const* logp, int groups,
                                         int B, int T, int D, int S, int hidden, void* stream);

#ifdef __cplusplus
}
#endif
#endif
