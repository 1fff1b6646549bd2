/* C ABI of libmrn_hip.so, lexicon-constrained decoding.  Bound by mrn_amd/_lib.py the same way as include/mrn_hip.h and
 * include/mrn_decode.h (prototypes parsed from this file, return code 0 = ok, mrn_last_error() for the message); kept in a header
 * of its own because the tests of the other headers pin their prototype counts. */
#ifndef MRN_LEXICON_H
#define MRN_LEXICON_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Lexicon-constrained decoding of a CTC head's logits (extends test.py:211-219, the CTC branch of validation(): the lexicon-free
 * decoders pick a string, this picks the word of a list with the largest log p(word | image)), one wave per (sample, word) pair, one
 * scoring launch per batch behind a row pass for the frames' logsumexp and in front of the top-n selection.  logits: fp32 [B][T][C]
 * with strides in elements and a contiguous last dimension; class 0 is the blank.  The lexicon: lex_tokens int32 [N][Lmax] (classes
 * 1..C-1, anything behind a word's length), lex_len int32 [N] (0..min(Lmax, 31)).  cand: NULL = every sample is scored against all N
 * words, else int32 [B][K] word indices per sample, -1 = unused slot, repeats allowed.  Nc = cand ? K : N positions per sample.
 * score(b, w) = -ctc_loss(log_softmax(x[b]), w, blank = 0): the CTC forward recursion in float32, restated in float64 by
 * mrn_amd/modules/decoding.py::ctc_lexicon_host; a word that does not fit the T frames (length + repeats > T) scores -inf, and a
 * sample with a NaN logsumexp in any frame (a NaN or +inf logit, a frame of -inf) has no live word.
 * Outputs: score_all [B][Nc] (-inf for a dead position: an infeasible word, an unused slot, a dead sample); index int32 [B][n] and
 * score [B][n]: the n best live positions in descending score, a tie to the lower position, as WORD indices (cand[b][slot] when
 * candidate lists are given), dead slots last as (-1, -inf); for the best entry path int64 [B][T] = the word's classes with one blank
 * between equal neighbours, blanks behind (greedy collapse gives the word back) and prob [B][T] = {exp(score), 1, 1, ...}: the pair
 * mrn_greedy_score_f32 takes in place of mrn_argmax_prob_f32's.  A sample without a live word has an all-blank path and prob[0] = 0.
 * prob doubles as the [B][T] logsumexp buffer while the call runs.
 * Limits (an error code and a message, never a fault; the outputs stay untouched): 1 <= T <= 512, 2 <= C <= 65535, 1 <= N <= 2^20,
 * 1 <= n <= 16, K >= 1 with cand, every length in 0..min(Lmax, 31), every token of a word in 1..C-1, every cand entry in -1..N-1.
 * The last three are device data: a checking pass reads them and the host waits for its verdict before launching anything else, so
 * the call synchronises the stream once and cannot be captured in a graph. */
int mrn_ctc_lexicon_decode_f32(const float* logits, int64_t stride_b, int64_t stride_t, int B, int T, int C,
                               const int32_t* lex_tokens, int Lmax, const int32_t* lex_len, int N,
                               const int32_t* cand, int K, int n, int32_t* index, float* score, float* score_all,
                               int64_t* path, float* prob, void* stream);

#ifdef __cplusplus
}
#endif
#endif
