// The character n-gram model of modules/char_lm.py in its device form: the table a kernel reads and the back-off evaluation, shared by
// the CTC prefix beam search (ctc_beam.hip) and the attention head's fused beam search (attn_decode.hip).  The hash (lm_mix) is stated
// here and in char_lm.py mix(), nowhere else.  The table is only read, and every loop over it is bounded by max_probe.
#pragma once
#include "common.hpp"

struct CharLMTable {
  const unsigned long long* keys;  // [mask + 1]: n << 60 | a << 32 | b << 16 | c, 0 = empty slot
  const float2* vals;              // [mask + 1]: (logp, bow)
  const float* uni_logp;           // [C_lm], entry 0 = end of text
  const float* uni_bow;            // [C_lm]
  unsigned mask;
  int max_probe, C_lm, order;
  float unk_logp;
};

// the 64-bit mix of char_lm.py mix(): the splitmix64 finaliser
__device__ __forceinline__ unsigned long long lm_mix(unsigned long long h) {
  h ^= h >> 30;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 31;
  return h;
}

// bounded linear probe: at most max_probe slots, whatever the table holds
__device__ __forceinline__ bool lm_find(const CharLMTable& lm, unsigned long long key, float2& v) {
  unsigned s = (unsigned)lm_mix(key) & lm.mask;
  for (int p = 0; p < lm.max_probe; ++p) {
    const unsigned long long k = lm.keys[s];
    if (k == key) {
      v = lm.vals[s];
      return true;
    }
    if (k == 0ull) return false;
    s = (s + 1u) & lm.mask;
  }
  return false;
}

// log p(c | a, b) by the back-off evaluation of char_lm.py CharLM.logp, float32 sums in its order; a, b, c in 0 .. 65534
__device__ __forceinline__ float lm_logp(const CharLMTable& lm, int a, int b, int c) {
  const float uni = c < lm.C_lm ? lm.uni_logp[c] : lm.unk_logp;
  if (lm.order == 1) return uni;
  const unsigned long long kb = (unsigned long long)b << 16, kc = (unsigned long long)c;
  float2 v;
  float bo = 0.f;
  if (lm.order == 3) {
    if (lm_find(lm, 3ull << 60 | (unsigned long long)a << 32 | kb | kc, v)) return v.x;
    if (lm_find(lm, 2ull << 60 | (unsigned long long)a << 16 | (unsigned long long)b, v)) bo = v.y;
  }
  if (lm_find(lm, 2ull << 60 | kb | kc, v)) return bo + v.x;
  return bo + ((b < lm.C_lm ? lm.uni_bow[b] : 0.f) + uni);
}

// the limits every entry point that takes a model checks before its launch (include/mrn_ctc_lm.h, include/mrn_attn_lm.h)
constexpr int CHAR_LM_MAX_C = 65535;                        // classes are 16-bit fields of a key
constexpr int64_t CHAR_LM_MAX_SLOTS = (int64_t)1 << 26;     // slots of the hash table
