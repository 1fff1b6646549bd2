/* C ABI of libmrn_hip.so, beam search on the attention head with a character n-gram language model.  Bound by mrn_amd/_lib.py the same
 * way as include/mrn_hip.h and include/mrn_decode.h (prototypes parsed from this file, return code 0 = ok, mrn_last_error() for the
 * message); kept in a header of its own because the tests of the other headers pin their prototype counts. */
#ifndef MRN_ATTN_LM_H
#define MRN_ATTN_LM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mrn_attn_beam_decode_grouped_f32 (include/mrn_attn_beam.h; extends the greedy loop of modules/prediction.py:70-86) with shallow fusion
 * of a character n-gram model, all S steps of `groups` experts of one geometry in one launch per eight experts (csrc/attn_decode.hip
 * attn_beam_lm_kernel, exact-fp32 form).  The algorithm is stated in mrn_amd/modules/decoding.py and restated in float64 by
 * attn_beam_host(lm=) there.  The operands, scratch and the six outputs are those of mrn_attn_beam_decode_grouped_f32.  An entry also
 * carries its last two LM symbols (0, 0 at the start = begin of text), its LM sum and its length in characters.  An unfinished entry
 * proposes its N = min(16, max(W, top_n)) classes of largest logit (a tie to the lower class, a NaN logit counts as -inf); a proposal of
 * class k has key = acoustic + alpha * (lm + term) + beta * len', term = logp(a, b, 0) for k = eos (the end of text), unk_logp for
 * k = 0 (the converter's [UNK], which no text contains) and logp(a, b, k) otherwise, len' = len + 1 (len for eos); the context becomes
 * (b, k), (b, 0) for eos -- a predicted class 0 reads as begin of text to its successors.  A finished entry proposes itself with its
 * key unchanged.  The W x N proposals of a sample are ranked by key, ties in (entry, class) order; rank < W with a key above -inf (a
 * NaN key counts as -inf) survives.
 * The model is that of mrn_ctc_beam_lm_decode_f32 (include/mrn_ctc_lm.h; mrn_amd/modules/char_lm.py CharLM.table()), one for all
 * groups: lm_keys uint64 [lm_mask + 1], lm_vals fp32 [lm_mask + 1][2], lm_max_probe the longest probe sequence of a stored key (a lookup
 * reads at most that many slots, so no table can make the kernel loop), uni_logp, uni_bow fp32 [C_lm]; a class >= C_lm scores
 * unk_logp; order 1..3.  The table is only read.
 * Outputs per group: those of mrn_attn_beam_decode_grouped_f32 with the entries in descending key -- score [B][W] and logp [B][W][S]
 * stay acoustic, so prob [B][S] stays a probability -- and fused fp32 [B][W], the key (-inf for a dead slot).  With alpha = beta = 0 the
 * first six outputs are mrn_attn_beam_decode_grouped_f32's, bit for bit.
 * Limits (an error code and a message, nothing is launched): 1 <= W <= 16, 1 <= top_n <= 16, 1 <= S <= 512, 2 <= num_class <= 65535,
 * 0 <= eos < num_class, hidden = 256, D a multiple of 16 whose whole-context tile fits the LDS budget:
 * 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + 3584 + 2560 <= 160 KiB; 1 <= C_lm <= 65535, lm_mask + 1 a power of two <= 2^26,
 * 0 <= lm_max_probe <= lm_mask + 1, 1 <= order <= 3, alpha >= 0, alpha, beta and unk_logp finite.  The arrays are trusted:
 * ops.upload_char_lm checks them on the host first. */
int mrn_attn_beam_lm_decode_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                        const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                        const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                        const void* const* b_hh, const void* const* w_gen, const void* const* b_gen, const int* num_class,
                                        int eos, int W, int top_n, const void* lm_keys, const float* lm_vals, int64_t lm_mask,
                                        int lm_max_probe, const float* uni_logp, const float* uni_bow, int C_lm, float unk_logp, int order,
                                        float alpha, float beta, const void* const* scratch, int64_t scratch_floats,
                                        const void* const* tokens, const void* const* length, const void* const* score,
                                        const void* const* logp, const void* const* path, const void* const* prob,
                                        const void* const* fused, int groups, int B, int T, int D, int S, int hidden, void* stream);

/* The same (modules/prediction.py:70-86) with the recurrent products and the generator as split-fp16 x3: the fp16 hi / lo streams and
 * w_inv (device float[4] per group: h2h, ih, hh, generator) of mrn_attn_beam_decode_x3_grouped.
 * Limits (an error code and a message, nothing is launched): 1 <= W <= 16, 1 <= top_n <= 16, 1 <= S <= 512, 2 <= num_class <= 65535,
 * 0 <= eos < num_class, hidden = 256, D a multiple of 32 whose whole-context tile fits the LDS budget: the sum above + 1024 <= 160 KiB;
 * the model's limits as above. */
int mrn_attn_beam_lm_decode_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                       const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                       const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                       const void* const* w_inv, const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                       const int* num_class, int eos, int W, int top_n, const void* lm_keys, const float* lm_vals,
                                       int64_t lm_mask, int lm_max_probe, const float* uni_logp, const float* uni_bow, int C_lm,
                                       float unk_logp, int order, float alpha, float beta, const void* const* scratch,
                                       int64_t scratch_floats, const void* const* tokens, const void* const* length,
                                       const void* const* score, const void* const* logp, const void* const* path,
                                       const void* const* prob, const void* const* fused, int groups, int B, int T, int D, int S,
                                       int hidden, void* stream);

#ifdef __cplusplus
}
#endif
#endif
