// The matrix-core operand types, the 16-bit conversions and the two operand
// splits that give the kernels float32-class results from 16-bit MFMAs
// (DESIGN.md §3.25).  Internal; included by dxr_common.h and out_store.h, so every
// translation unit of both libraries sees one definition of each.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dxr {

// ---------------------------------------------------------------------------
// Vector types of the MFMA and raw-buffer builtins: <element>x<lanes>_t.
// ---------------------------------------------------------------------------
typedef float f32x16_t __attribute__((ext_vector_type(16)));   // 32x32 accumulator
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));   // 32x32x16 bf16 operand
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));  // 32x32x16 f16 operand
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));     // 16-bit operand bits, type-free
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));  // buffer loads and stores
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void_t;     // LDS destination of a buffer DMA

// ---------------------------------------------------------------------------
// Conversions.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(uint16_t v) {
  return __uint_as_float(((uint32_t)v) << 16);
}

// Software round-to-nearest-even f32 -> bf16 that keeps NaN a NaN (~6 VALU per
// value; the kernels' hot paths use cvt_pk_bf16).
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// Widening of one f16x2 word: the hardware v_cvt_f32_f16 (exact, subnormals
// included).
__device__ __forceinline__ void f16x2_to_f32(uint32_t w, float* v) {
  const f16x2_t h = __builtin_bit_cast(f16x2_t, w);
  v[0] = (float)h[0];
  v[1] = (float)h[1];
}

// v_cvt_pk_bf16_f32: two floats rounded to nearest even into one bf16x2 word
// (first in the low half; NaN stays NaN, overflow to +-inf).
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// Two floats rounded to nearest even into one f16x2 word (overflow to +-inf,
// subnormals kept, NaN stays NaN) — never v_cvt_pkrtz_f16_f32, which rounds
// toward zero.  Not pinned: the compiler may fold the producing arithmetic into
// the conversion.  The splits below only hand it exact values, for which one
// rounding and two are the same; a stored result takes the pinned form.
__device__ __forceinline__ uint32_t cvt_pk_f16(float a, float b) {
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t));
}

// The 16 bits of a float32 value rounded to OT (_Float16 / __bf16) to nearest even
// by the hardware conversions (v_cvt_f16_f32: overflow to +-inf, subnormals kept;
// v_cvt_pk_bf16_f32): torch's .to(dtype) bit for bit.  Pinned: the value is held
// as a float32 register first.  Without that the compiler folds a producing fma
// and the conversion into v_fma_mixlo_f16, which rounds the exact sum once to
// float16 and so breaks ties differently from float32-then-cast.
template <typename OT>
__device__ __forceinline__ uint32_t out16_bits(float r) {
  static_assert(sizeof(OT) == 2, "16-bit output types");
  asm volatile("" : "+v"(r));
  return __builtin_bit_cast(uint16_t, static_cast<OT>(r));
}
__device__ __forceinline__ uint16_t f32_to_f16_bits(float f) {
  return (uint16_t)out16_bits<_Float16>(f);
}
__device__ __forceinline__ uint32_t cvt_pk_f16_pinned(float a, float b) {
  return (uint32_t)f32_to_f16_bits(a) | ((uint32_t)f32_to_f16_bits(b) << 16);
}

// ---------------------------------------------------------------------------
// The three-way bfloat16 split: x = hi + mid + lo, six MFMA products per f32
// product (hh, hm, mh, hl, lh, mm).  hi = RNE_bf16(x), mid = RNE_bf16(x - hi),
// lo = the top 16 bits of x - hi - mid, which is all of it: the residuals are
// multiples of ulp(x) spanning <= 16 and <= 8 significant bits, so both
// subtractions and lo are exact for |x| in the normal f32 range (the derivation
// and the dropped terms: csrc/corr_build.hip, "split" build).  It covers the
// whole f32 range and so is the fallback of every f16 pair kernel below, and
// the only split of corr_backward.hip's unbounded form.
//
// The variants differ in what they do where hi is not finite:
//
//                      GUARD_INF                    GUARD_INF_AND_RANGE
//   +-inf              hi = +-inf, mid = lo = 0     the same
//                      (without the guard inf - inf makes mid and lo NaN, and
//                      a +-inf product NaN)
//   NaN                hi, mid and lo all NaN       the same
//   finite, rounds     hi = +-inf, mid = lo = 0:    hi = x truncated to bf16
//   past bf16's        the operand turns into       (+-0x7f7f), mid and lo the
//   largest finite     +-inf                        exact rest: the operand
//   (|x| >= 0x7f7f8000                              stays finite and exact
//   = 3.3961e38)
//
//   kernel (file)                                         variant
//   corr_build_split_kernel fallback (corr_build.hip)     GUARD_INF
//   alt_corr_mfma_kernel fallback and its bf16-fmap form's
//     float32 levels; alt_volume_gemm_kernel fallback
//     (alt_corr.hip, alt_corr_out / _in16 / _inbf16.hip)  GUARD_INF
//   corr_lookup_conv1x1_h2_kernel fallback
//     (corr_lookup.hip and its variant units)             GUARD_INF_AND_RANGE
//   fmap-gradient GEMMs: fold records, pack pass and the
//     bounded form's in-register fallback
//     (corr_backward.hip)                                 GUARD_INF_AND_RANGE
//
// (DESIGN.md names the fallback per kernel — §3.1, §3.5, §3.6, §3.8 — but not
// its guards; tests/test_gpu_motion.py holds GUARD_INF_AND_RANGE's third row for
// the fused lookup.)
// ---------------------------------------------------------------------------
enum class Bf16Split { GUARD_INF, GUARD_INF_AND_RANGE };

struct Split3 {
  uint32_t h, m, l;  // bf16x2 words (first element in the low half)
};

template <Bf16Split G>
__device__ __forceinline__ Split3 split3_bf16(float a, float b) {
  uint32_t hp = cvt_pk_bf16(a, b);
  if constexpr (G == Bf16Split::GUARD_INF_AND_RANGE) {
    if (__builtin_isinf(__uint_as_float(hp << 16)) && !__builtin_isinf(a))
      hp = (hp & 0xffff0000u) | (__float_as_uint(a) >> 16);
    if (__builtin_isinf(__uint_as_float(hp & 0xffff0000u)) && !__builtin_isinf(b))
      hp = (hp & 0xffffu) | (__float_as_uint(b) & 0xffff0000u);
  }
  const float ha = __uint_as_float(hp << 16), hb = __uint_as_float(hp & 0xffff0000u);
  const float ra = __builtin_isinf(ha) ? 0.f : a - ha, rb = __builtin_isinf(hb) ? 0.f : b - hb;
  const uint32_t mp = cvt_pk_bf16(ra, rb);
  const float la = ra - __uint_as_float(mp << 16), lb = rb - __uint_as_float(mp & 0xffff0000u);
  return {hp, mp, __builtin_amdgcn_perm(__float_as_uint(lb), __float_as_uint(la), 0x07060302u)};
}

// 8 floats as three 8 x bf16 MFMA operands.
template <Bf16Split G>
__device__ __forceinline__ void split8_bf16(const float (&x)[8], uint4& h, uint4& m, uint4& l) {
  uint32_t hh[4], mm[4], ll[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const Split3 s = split3_bf16<G>(x[2 * e], x[2 * e + 1]);
    hh[e] = s.h;
    mm[e] = s.m;
    ll[e] = s.l;
  }
  h = make_uint4(hh[0], hh[1], hh[2], hh[3]);
  m = make_uint4(mm[0], mm[1], mm[2], mm[3]);
  l = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}

// ---------------------------------------------------------------------------
// The float16 pair split, three MFMA products per f32 product (hi*hi and the
// two cross terms; lo*lo, <= 2^-22 |x y| and sign-symmetric under RNE, is
// dropped).  f16 x f16 products are exact in f32.  hi = RNE_f16(x); x - hi is
// exact in f32, so lo carries the only rounding: <= 2^-22 |x| while hi is
// normal, <= 2^-36 absolute below (|x| < 2^-14, lo subnormal).
//
// Validity, stated once: hi must be finite, |x| < 65520.  A kernel on the pair
// detects a miss (an operand past that, inf or NaN) from its own non-finite
// sums and re-runs on the three-way bf16 split.  The forms:
//
//   split2_f16 / split8_f16      lo = RNE_f16((x - hi) * 2^11), x = hi + 2^-11 lo:
//       alt_corr.hip (alt_corr_mfma_kernel's cells and query planes,
//       alt_split_planes_kernel; alt_volume_gemm_kernel writes the pair out),
//       corr_lookup.hip (corr_lookup_conv1x1_h2_kernel's samples,
//       conv1x1_pack_weight_kernel).  No prescale: lo reaches 11 bits below
//       hi's range.
//   split2_f16_fused<PairLo::SCALED_2_11>   the same lo by one mixed-precision
//       step, RNE_f16(fma(hi, -2048, 2048 x)): 2048 x and 2048 hi are exact and
//       so is their difference, so the bits are split2_f16's; hi stays an f16
//       operand (v_fma_mix*_f16), 44 instead of 68 VALU per k step.
//       corr_build_split_kernel's main path.  Not folded into split2_f16: the
//       instruction streams differ.
//   split2_f16_fused<PairLo::UNSCALED>      lo = RNE_f16(x - hi), x = hi + lo, for
//       operands the caller has already scaled by a power of two so that
//       |x 2^e| < 2^14; an element is then carried to <= 2^-23 |x| unless it is
//       more than 2^16 below the scale's bound (then to <= 2^-39 of that bound):
//       split16_f16_record, split_pairs_kernel's records (corr_build.hip, one
//       scale per pixel), and split8_f16_prescaled, the fmap-gradient GEMMs'
//       bounded form (corr_backward.hip: one scale per channel, one for dV).
//       The caller undoes the scales exactly (ldexp) on the sums.
// ---------------------------------------------------------------------------
struct Split2 {
  uint32_t h, l;  // f16x2 words (first element in the low half)
};

__device__ __forceinline__ Split2 split2_f16(float a, float b) {
  const uint32_t h = cvt_pk_f16(a, b);
  const f16x2_t hv = __builtin_bit_cast(f16x2_t, h);
  return {h, cvt_pk_f16((a - (float)hv[0]) * 2048.f, (b - (float)hv[1]) * 2048.f)};
}

// 8 floats as two 8 x f16 MFMA operands (split2_f16 per pair, with the vectors
// written out: the form both families' kernels compile unchanged from).
__device__ __forceinline__ void split8_f16(const float (&x)[8], uint4& h, uint4& l) {
  uint32_t hh[4], ll[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x2_t v = {x[2 * e], x[2 * e + 1]};
    hh[e] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t));
    const f16x2_t hv = __builtin_bit_cast(f16x2_t, hh[e]);
    const f32x2_t r = {(x[2 * e] - (float)hv[0]) * 2048.f, (x[2 * e + 1] - (float)hv[1]) * 2048.f};
    ll[e] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2_t));
  }
  h = make_uint4(hh[0], hh[1], hh[2], hh[3]);
  l = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}

enum class PairLo { SCALED_2_11, UNSCALED };

template <PairLo LO>
__device__ __forceinline__ Split2 split2_f16_fused(float a, float b) {
  const uint32_t h = cvt_pk_f16(a, b);
  const f16x2_t hv = __builtin_bit_cast(f16x2_t, h);
  f16x2_t lv;
  if constexpr (LO == PairLo::SCALED_2_11) {
    lv[0] = (_Float16)__builtin_fmaf((float)hv[0], -2048.f, a * 2048.f);
    lv[1] = (_Float16)__builtin_fmaf((float)hv[1], -2048.f, b * 2048.f);
  } else {
    lv[0] = (_Float16)__builtin_fmaf((float)hv[0], -1.f, a);
    lv[1] = (_Float16)__builtin_fmaf((float)hv[1], -1.f, b);
  }
  return {h, __builtin_bit_cast(uint32_t, lv)};
}

// 16 consecutive channels of one pixel, already scaled, as the 64-byte record of
// split_pairs_kernel: hi 16 f16, then lo 16 f16.  The arithmetic of
// split2_f16_fused<PairLo::UNSCALED>, written out: through the pair function
// the same instructions come out in another order in split_pairs_kernel.
__device__ __forceinline__ void split16_f16_record(const float (&x)[16], uint4 (&rec)[4]) {
  uint32_t h[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = cvt_pk_f16(x[2 * e], x[2 * e + 1]);
    const f16x2_t hv = __builtin_bit_cast(f16x2_t, h[e]);
    f16x2_t lv;
    lv[0] = (_Float16)__builtin_fmaf((float)hv[0], -1.f, x[2 * e]);
    lv[1] = (_Float16)__builtin_fmaf((float)hv[1], -1.f, x[2 * e + 1]);
    l[e] = __builtin_bit_cast(uint32_t, lv);
  }
  rec[0] = make_uint4(h[0], h[1], h[2], h[3]);
  rec[1] = make_uint4(h[4], h[5], h[6], h[7]);
  rec[2] = make_uint4(l[0], l[1], l[2], l[3]);
  rec[3] = make_uint4(l[4], l[5], l[6], l[7]);
}

// 8 values scaled by 2^e (|x 2^e| < 2^14 by the caller's choice of e), then the
// unscaled pair.
__device__ __forceinline__ void split8_f16_prescaled(const float (&v)[8], int e, uint4& hi, uint4& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const Split2 s = split2_f16_fused<PairLo::UNSCALED>(__builtin_ldexpf(v[2 * i], e),
                                                        __builtin_ldexpf(v[2 * i + 1], e));
    h[i] = s.h;
    l[i] = s.l;
  }
  hi = make_uint4(h[0], h[1], h[2], h[3]);
  lo = make_uint4(l[0], l[1], l[2], l[3]);
}

}  // namespace dxr
