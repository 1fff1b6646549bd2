// The HL32 operand format of the split-fp16 x3 products, in one place: how a value is split, how a line is laid out, how lines
// reach LDS and how they are multiplied.
//
// Every fp32 operand is x = hi + lo (two fp16, 22 significand bits); one 128-byte line holds 32 consecutive values of one row
// (pixel, token, output channel ...) as [ hi fp16 x 32 | lo fp16 x 32 ]: value c of the line has its hi half at byte 2c and its lo
// half at byte 64 + 2c.  A product of two operands is lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation.
#pragma once
#include "common.hpp"

typedef _Float16 f16v8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16v4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// buffer descriptor over `bytes` bytes at `base`: an offset beyond the range reads zeros (how padded taps / rows are produced)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}

// 16 bytes per lane, global (buffer descriptor + per-lane byte offset + wave-uniform offset) -> LDS (wave-uniform base + 16*lane)
__device__ __forceinline__ void dma16(const __amdgpu_buffer_rsrc_t r, unsigned char* l, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)l, 16, voff, soff, 0, 0);
}

// one f16 32x32x16 product on eight halves per lane and operand (16 bytes of a line's hi or lo half)
__device__ __forceinline__ f32x16 mma(const u32x4 a, const u32x4 b, const f32x16 c) {
#if defined(MRN_PROBE_NO_MFMA) || defined(MRN_WPROBE_NO_MFMA) || defined(MRN_PPROBE_NO_MFMA)
  f32x16 r = c;                 // (what-if probe of tools/build_probe.sh, never in the product build: the staging floor without matrix work)
  r[0] += __builtin_bit_cast(float, a[0] ^ b[0]);
  return r;
#endif
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16v8*>(&a), *reinterpret_cast<const f16v8*>(&b), c, 0, 0, 0);
}

// x = hi + lo as two fp16 (22 significand bits).  The operand is pinned in a register first: under -ffp-contract=fast the
// compiler may otherwise fold the multiply / fma that PRODUCED x into the conversion (v_fma_mixlo_f16: one rounding from the
// exact product) for one use of hi and convert the fp32-rounded value (two roundings) for another -- the two differ by one
// fp16 ulp when the fp32 value sits on an fp16 tie, and the pair then misses x by 2^-11 (seen on 2 of 65536 elements).
__device__ __forceinline__ void split_f16(float x, _Float16& hi, _Float16& lo) {
  asm volatile("" : "+v"(x));
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}

// the same for range-scaled GRADIENT operands (BPTT gate gradients, scaled by a power of two from max|dout|): saturate at the
// fp16 range instead of hi = inf, lo = -inf (NaN products) when back-propagation through time grows them past the headroom --
// the exact-fp32 kernels give large finite gradients there, which the global-norm clip then handles
__device__ __forceinline__ void split_f16_sat(float x, _Float16& hi, _Float16& lo) {
  x = fminf(fmaxf(x, -65504.f), 65504.f);
  split_f16(x, hi, lo);
}

// The hi and lo halves of four (H = f16v4) or eight (f16v8) consecutive values of a line; store(line) writes them, `line` pointing at
// the first value's hi half.  Used as  split_hl4<SAT>(v).store(line): the halves are formed before the address is.
template <class H>
struct HalfLine {
  H hi, lo;
  __device__ __forceinline__ void store(unsigned char* line) const {
    *reinterpret_cast<H*>(line) = hi;
    *reinterpret_cast<H*>(line + 64) = lo;
  }
};

// SAT: the saturating split.  get(e): value e of the four, for values that are formed one at a time (a scaled element, an LDS read)
template <bool SAT = false, class F>
__device__ __forceinline__ HalfLine<f16v4> split_hl4(F get) {
  HalfLine<f16v4> r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    _Float16 hh, ll;
    if constexpr (SAT) split_f16_sat(get(e), hh, ll);
    else split_f16(get(e), hh, ll);
    r.hi[e] = hh; r.lo[e] = ll;
  }
  return r;
}
template <bool SAT = false>
__device__ __forceinline__ HalfLine<f16v4> split_hl4(const f32x4 v) {
  return split_hl4<SAT>([&](int e) { return v[e]; });
}

// a: the first four values, b: the next four
template <bool SAT = false>
__device__ __forceinline__ HalfLine<f16v8> split_hl8(const f32x4 a, const f32x4 b) {
  HalfLine<f16v8> r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    _Float16 hh, ll;
    if constexpr (SAT) split_f16_sat(a[e], hh, ll);
    else split_f16(a[e], hh, ll);
    r.hi[e] = hh; r.lo[e] = ll;
    if constexpr (SAT) split_f16_sat(b[e], hh, ll);
    else split_f16(b[e], hh, ll);
    r.hi[4 + e] = hh; r.lo[4 + e] = ll;
  }
  return r;
}
