/* C ABI of libmrn_hip.so, CTC prefix beam search with a character n-gram language model.  Bound by mrn_amd/_lib.py the same way as
 * include/mrn_hip.h and include/mrn_decode.h (prototypes parsed from this file, return code 0 = ok, mrn_last_error() for the
 * message); kept in a header of its own because the tests of the other headers pin their prototype counts. */
#ifndef MRN_CTC_LM_H
#define MRN_CTC_LM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mrn_ctc_beam_decode_f32 (include/mrn_decode.h; extends test.py:211-219, the CTC branch of validation()) with shallow fusion of a
 * character n-gram model: the operands, the layout of the work (one wave per sample, one launch per batch) and the outputs of that
 * entry point, and the candidates of a frame ranked by total + alpha * lm' + beta * len' instead of the total, lm' = the model's
 * log-probability of the candidate's prefix, len' its length.  After the last frame the live entries are ordered by
 * fused = total + alpha * (lm + logp(end of text)) + beta * len, descending, a tie to the earlier slot.  The algorithm and the model
 * are restated in float64 by mrn_amd/modules/decoding.py::ctc_beam_host(lm=) and mrn_amd/modules/char_lm.py.
 * The model (char_lm.py CharLM.table(); tokens are the head's classes, 0 = begin of text in a context and end of text when
 * predicted): lm_keys uint64 [lm_mask + 1], an open-addressing hash table with linear probing, key = n << 60 | a << 32 | b << 16 | c
 * for n = 2 (a = 0) and n = 3, 0 = empty slot, slot = mix(key) & lm_mask with the splitmix64 finaliser; lm_vals fp32 [lm_mask + 1][2]
 * = (logp, bow); lm_max_probe = the longest probe sequence of a stored key: a lookup reads at most that many slots, so no table can
 * make the kernel loop; uni_logp, uni_bow fp32 [C_lm]; a class >= C_lm scores unk_logp; order 1..3.  The table is only read.
 * Outputs: those of mrn_ctc_beam_decode_f32 with the entries in descending fused key -- score [B][W] stays the acoustic
 * log-probability of the label, so prob [B][T] = {exp(score), 1, 1, ...} stays a probability -- and fused fp32 [B][W], the key
 * (-inf for a dead slot).  With alpha = beta = 0 the first five outputs are mrn_ctc_beam_decode_f32's, bit for bit.
 * Limits (an error code and a message before any launch, never a fault): 1 <= T <= 512, 2 <= C <= 65535, 1 <= W <= 16,
 * 1 <= K <= 15, 1 <= C_lm <= 65535, lm_mask + 1 a power of two <= 2^26, 0 <= lm_max_probe <= lm_mask + 1, 1 <= order <= 3,
 * alpha >= 0, alpha, beta and unk_logp finite.  The arrays are trusted: ops.upload_char_lm checks them on the host first. */
int mrn_ctc_beam_lm_decode_f32(const float* logits, int64_t stride_b, int64_t stride_t, int B, int T, int C, int W, int K,
                               int32_t* tokens, int32_t* length, float* score, int64_t* path, float* prob,
                               const void* lm_keys, const float* lm_vals, int64_t lm_mask, int lm_max_probe,
                               const float* uni_logp, const float* uni_bow, int C_lm, float unk_logp, int order, float alpha,
                               float beta, float* fused, void* stream);

#ifdef __cplusplus
}
#endif
#endif
