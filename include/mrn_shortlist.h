/* C ABI of libmrn_hip.so, lexicon shortlists by edit distance.  Bound by mrn_amd/_lib.py the same way as include/mrn_hip.h,
 * include/mrn_decode.h, include/mrn_attn_beam.h, include/mrn_lexicon.h, include/mrn_attn_lexicon.h and include/mrn_attn_score.h
 * (prototypes parsed from this file, return code 0 = ok, mrn_last_error() for the message); a header of its own because the tests pin
 * the prototypes of the other six. */
#ifndef MRN_SHORTLIST_H
#define MRN_SHORTLIST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace mrn_lexicon_shortlist_i32 needs for B samples and N words (a histogram of 256 counts per sample and one
 * distance byte per (sample, word), rows padded to 16 bytes); -1 outside 0 <= B, 1 <= N <= 2^20. */
int64_t mrn_lexicon_shortlist_work_bytes(int B, int N);

/* The K lexicon words nearest to one hypothesis per sample (extends the scoring loop of test.py:243-250: its edit_distance between a
 * prediction and ONE label becomes the distance between a prediction and every word of a lexicon, with a top-K selection; the middle
 * step of the lexicon protocol of Shi et al., section 3.3).  csrc/lexicon_shortlist.hip: Myers' bit-vector algorithm, one thread per
 * (sample, word), then a histogram cut and an index-ordered compaction.  The algorithm is stated in mrn_amd/modules/decoding.py and
 * restated in numpy by lexicon_shortlist_host there.  DEVICE arrays of int32: hyp [B][Hmax] (class tokens of the hypothesis of sample
 * b in its first hyp_len[b] places), hyp_len [B], the word table lex_tokens [N][Lmax] / lex_len [N] of ops.upload_words.  d(b, w) is
 * the unit-cost Levenshtein distance between hyp[b][:hyp_len[b]] and lex_tokens[w][:lex_len[w]].  Per sample the words with
 * max_dist = -1 or d <= max_dist are ranked by (d, w) ascending, a tie to the lower word index; the first K go to cand [B][K] (word
 * indices) and dist [B][K] (their distances), -1 in both behind them.  flag [B] = 1 for a sample with hyp_len > 64 or hyp_len < 0:
 * it is not computed, its rows are all -1, the caller finishes it on the host.  Integer arithmetic throughout: the result is defined
 * to the last bit and does not depend on the order in which atomics land.  The kernel clamps hyp_len to Hmax and lex_len to
 * 0 ... Lmax; the caller checks the tables (decoding.check_word_table).  work: work_bytes >= mrn_lexicon_shortlist_work_bytes(B, N)
 * bytes, 16-byte aligned, contents undefined before and after.
 * Limits (an error code, nothing is launched): 1 <= K <= 256, 1 <= N <= 2^20, 1 <= Lmax <= 255, 0 <= Hmax, max_dist >= -1, classes
 * 0 ... 65534 (the caller's to keep), no null operand (hyp may be null where Hmax = 0). */
int mrn_lexicon_shortlist_i32(const int32_t* hyp, int Hmax, const int32_t* hyp_len, int B, const int32_t* lex_tokens, int Lmax,
                              const int32_t* lex_len, int N, int K, int max_dist, int32_t* cand, int32_t* dist, int32_t* flag,
                              void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
