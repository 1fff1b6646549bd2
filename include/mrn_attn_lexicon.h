/* C ABI of libmrn_hip.so, lexicon-constrained beam search on the attention head.  Bound by mrn_amd/_lib.py the same way as
 * include/mrn_hip.h, include/mrn_decode.h, include/mrn_attn_beam.h and include/mrn_lexicon.h (prototypes parsed from this file, return
 * code 0 = ok, mrn_last_error() for the message); a header of its own because the tests pin the prototypes of the other four. */
#ifndef MRN_ATTN_LEXICON_H
#define MRN_ATTN_LEXICON_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Beam search on the attention head walked along a trie of a lexicon (extends the greedy loop of modules/prediction.py:70-86: W
 * entries per sample, each one a prefix of a lexicon word, instead of the one arg-max), all S steps of `groups` experts of one geometry
 * (B, T, D, S) in one launch per eight experts (csrc/attn_decode.hip attn_lexicon_kernel, exact-fp32 form).  The algorithm is stated in
 * mrn_amd/modules/decoding.py and restated in float64 by attn_lexicon_host there.  The operands, eos, W, scratch and the six outputs
 * are those of mrn_attn_beam_decode_grouped_f32 (include/mrn_attn_beam.h).  The trie, one for all groups, is four DEVICE arrays of
 * int32: node 0 is the root, the children of node n are the edges child_off[n] ... child_off[n + 1] - 1 (child_off [nodes + 1]) with
 * class child_tok[e] and node child_node[e] (both [nodes - 1]); word_of [nodes] is the lexicon index of a word that ends at the node,
 * else -1.  A child whose class is not below a group's num_class is skipped for that group.  depth = the longest word.  The kernel
 * trusts the arrays: the caller checks them (mrn_amd/ops.py upload_trie: offsets monotone from 0 to nodes - 1, parent < child_node <
 * nodes).  One more output per group: word int32 [B][W] = word_of of the entry's node, -1 for a dead slot; a sample none of whose
 * words can be spelled has only dead slots (length -1, score -inf, path all eos, prob all 1).
 * Limits (an error code, nothing is launched): 1 <= W <= 16, 1 <= S <= 512, num_class >= 2, 0 <= eos < num_class, hidden = 256,
 * nodes >= 1, 0 <= depth <= S - 1, no null trie array, D a multiple of 16 whose whole-context tile fits the LDS budget:
 * 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + 3584 + 1152 <= 160 KiB. */
int mrn_attn_lexicon_decode_grouped_f32(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                        const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                        const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                        const void* const* b_hh, const void* const* w_gen, const void* const* b_gen, const int* num_class,
                                        int eos, int W, const int32_t* child_off, const int32_t* child_tok, const int32_t* child_node,
                                        const int32_t* word_of, int nodes, int depth, const void* const* scratch, int64_t scratch_floats,
                                        const void* const* tokens, const void* const* length, const void* const* score,
                                        const void* const* logp, const void* const* path, const void* const* prob,
                                        const void* const* word, int groups, int B, int T, int D, int S, int hidden, void* stream);

/* The same (modules/prediction.py:70-86) with the recurrent products and the generator as split-fp16 x3: the fp16 hi / lo streams and
 * w_inv (device float[4] per group: h2h, ih, hh, generator) of mrn_attn_beam_decode_x3_grouped.
 * Limits (an error code, nothing is launched): 1 <= W <= 16, 1 <= S <= 512, num_class >= 2, 0 <= eos < num_class, hidden = 256,
 * nodes >= 1, 0 <= depth <= S - 1, no null trie array, D a multiple of 32 whose whole-context tile fits the LDS budget: the sum above
 * + 1024 <= 160 KiB. */
int mrn_attn_lexicon_decode_x3_grouped(const void* const* Hb, const void* const* Hproj, const void* const* etab,
                                       const int64_t* start_token, const void* const* w_h2h, const void* const* b_h2h,
                                       const void* const* w_score, const void* const* w_ih_ctx, const void* const* w_hh,
                                       const void* const* w_inv, const void* const* b_hh, const void* const* w_gen, const void* const* b_gen,
                                       const int* num_class, int eos, int W, const int32_t* child_off, const int32_t* child_tok,
                                       const int32_t* child_node, const int32_t* word_of, int nodes, int depth, const void* const* scratch,
                                       int64_t scratch_floats, const void* const* tokens, const void* const* length,
                                       const void* const* score, const void* const* logp, const void* const* path, const void* const* prob,
                                       const void* const* word, int groups, int B, int T, int D, int S, int hidden, void* stream);

#ifdef __cplusplus
}
#endif
#endif
