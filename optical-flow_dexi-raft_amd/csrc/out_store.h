// Output conversion and store helpers shared by the lookups' flagged output forms
// (DXR_OUT_F16 / DXR_OUT_BF16 / DXR_OUT_NHWC): csrc/corr_lookup.hip (the product
// lookup and the alternate block's volume lookup) and csrc/alt_corr.hip (the
// on-the-fly lookup).  One rounding routine for all of them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dexiraft_corr.h"
#include "mfma_operands.h"

namespace dxr {

// Parity (in elements) of a 2-byte aligned output base.
template <typename OT>
__device__ __forceinline__ int out16_base_parity(const OT* out) {
  return (int)((reinterpret_cast<uintptr_t>(out) >> 1) & 1);
}

// MODE 0: plain stores; 1: non-temporal; 2: write-through (agent scope), the
// float32 kernels' forms.  `word`: store the 32-bit word `w` at `p` (4-byte
// aligned), else the 16-bit element `h`.
template <typename OT, int MODE>
__device__ __forceinline__ void store_out16_one(OT* p, uint32_t h, uint32_t w, bool word) {
  if (word) {
    uint32_t* pw = reinterpret_cast<uint32_t*>(p);
    if constexpr (MODE == 1) __builtin_nontemporal_store(w, pw);
    else if constexpr (MODE == 2) __hip_atomic_store(pw, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *pw = w;
  } else {
    uint16_t* ph = reinterpret_cast<uint16_t*>(p);
    if constexpr (MODE == 1) __builtin_nontemporal_store((uint16_t)h, ph);
    else if constexpr (MODE == 2) __hip_atomic_store(ph, (uint16_t)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *ph = (uint16_t)h;
  }
}

// Store policy of the channels-last forms, a compile-time argument.
enum { NHWC_WRITE_THROUGH = 0, NHWC_NON_TEMPORAL = 1, NHWC_PLAIN = 2 };

template <int POL, typename T>
__device__ __forceinline__ void store_policy(T* p, T v) {
  if constexpr (POL == NHWC_NON_TEMPORAL) __builtin_nontemporal_store(v, p);
  else if constexpr (POL == NHWC_WRITE_THROUGH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// ---------------------------------------------------------------------------
// Pinned float32 arithmetic for the alternate block's flagged forms.
//
// The float32 NCHW kernels (alt_corr_mfma_kernel, corr_lookup_qm_kernel<ALT>)
// write the bilinear combination of a window's four sums as plain C++, and the
// compiler lowers it — the same way in every one of their instantiations, read
// off their disassembly — to the instruction sequences below.  A flagged form
// must reproduce those kernels' float32 bits, NaNs included: a non-finite
// coordinate makes dx a NaN and gx = 1 - dx a NaN of the other sign, and which
// of two NaN operands an instruction hands on depends on their order.  So the
// flagged forms issue exactly these instructions with exactly these operand
// orders, whatever the compiler would choose for their own source.  That the
// float32 kernels still compile to these sequences is an observation, held by
// tests/test_gpu_alt_out.py (every radius and form, all bits, NaNs included).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float pin_mul(float a, float b) {
  float d;
  asm("v_mul_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ float pin_add(float a, float b) {
  float d;
  asm("v_add_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ float pin_sub(float a, float b) {
  float d;
  asm("v_sub_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// acc + a * b, fused
__device__ __forceinline__ float pin_fmac(float acc, float a, float b) {
  asm("v_fmac_f32_e32 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b));
  return acc;
}
// a * b - c, fused: the fraction c * inv - floor(c * inv) of alt_corr_mfma_kernel
__device__ __forceinline__ float pin_fma_neg(float a, float b, float c) {
  float d;
  asm("v_fma_f32 %0, %1, %2, -%3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// gx*(gy*s00) + dx*(gy*s01) + gx*(dy*s10) + dx*(dy*s11) as those kernels issue it
// (gx = 1 - dx, gy = 1 - dy): one product, then three fused steps.  S_FIRST: the
// volume lookup multiplies s00 * gy, the on-the-fly kernel gy * s00.
template <bool S_FIRST>
__device__ __forceinline__ float alt_combine_pinned(float s00, float s01, float s10, float s11,
                                                    float dx, float dy, float gx, float gy) {
  const float a1 = pin_mul(gy, s01);
  const float a0 = S_FIRST ? pin_mul(s00, gy) : pin_mul(gy, s00);
  float t = pin_mul(dx, a1);
  t = pin_fmac(t, gx, a0);
  t = pin_fmac(t, gx, pin_mul(dy, s10));
  t = pin_fmac(t, dx, pin_mul(dy, s11));
  return t;
}

// The on-the-fly kernel at r = 0 (one output per query: the vectoriser packs the
// products before any contraction): eight products, three sums, none fused.
__device__ __forceinline__ float alt_combine_pinned_r0(float s00, float s01, float s10, float s11,
                                                       float dx, float dy, float gx, float gy) {
  const float a0 = pin_mul(gy, s00), a1 = pin_mul(gy, s01);
  const float b0 = pin_mul(dy, s10), b1 = pin_mul(dy, s11);
  float v = pin_add(pin_mul(gx, a0), pin_mul(dx, a1));
  v = pin_add(v, pin_mul(b0, gx));
  return pin_add(v, pin_mul(dx, b1));
}

// torch's float32 -> bfloat16 conversion maps every NaN to the one quiet NaN
// 0x7FC0 (sign and payload dropped; float16 keeps both, as the hardware
// conversions do).  The alternate block's flagged forms are out.to(dtype) bit
// for bit, so they hand their bfloat16 stores this value for a NaN.
__device__ __forceinline__ float bf16_nan_as_torch(float r) {
  return r != r ? __uint_as_float(0x7FC00000u) : r;
}

// The six output forms (element type x layout) as a bit set: the forms a
// translation unit may instantiate.
enum : unsigned {
  FORM_F32 = 1, FORM_F16 = 2, FORM_BF16 = 4,   // NCHW; channels-last: << 3
  FORMS_NCHW = 7, FORMS_NCHW16 = FORM_F16 | FORM_BF16, FORMS_NHWC = FORMS_NCHW << 3,
  FORMS_ALL = FORMS_NCHW | FORMS_NHWC, FORMS_FLAGGED = FORMS_ALL & ~FORM_F32
};

// A request's form (out_flag: 0, DXR_OUT_F16 or DXR_OUT_BF16) as the call
// f(OT* out, std::bool_constant<NHWC>), OT = float / _Float16 / __bf16; `f` is
// instantiated for the forms of FORMS only, any other form is DXR_EINVAL.
template <unsigned FORMS, typename F>
int dispatch_out_form(int out_flag, bool nhwc, void* out, F&& f) {
  const unsigned dt = out_flag == DXR_OUT_F16 ? FORM_F16 : out_flag == DXR_OUT_BF16 ? FORM_BF16 : FORM_F32;
  const unsigned form = nhwc ? dt << 3 : dt;
  if constexpr ((FORMS & FORM_F32) != 0)
    if (form == FORM_F32) return f(static_cast<float*>(out), std::false_type{});
  if constexpr ((FORMS & FORM_F16) != 0)
    if (form == FORM_F16) return f(static_cast<_Float16*>(out), std::false_type{});
  if constexpr ((FORMS & FORM_BF16) != 0)
    if (form == FORM_BF16) return f(static_cast<__bf16*>(out), std::false_type{});
  if constexpr ((FORMS & FORM_F32 << 3) != 0)
    if (form == FORM_F32 << 3) return f(static_cast<float*>(out), std::true_type{});
  if constexpr ((FORMS & FORM_F16 << 3) != 0)
    if (form == FORM_F16 << 3) return f(static_cast<_Float16*>(out), std::true_type{});
  if constexpr ((FORMS & FORM_BF16 << 3) != 0)
    if (form == FORM_BF16 << 3) return f(static_cast<__bf16*>(out), std::true_type{});
  return DXR_EINVAL;
}

// A form as the `okind` argument of the on-the-fly kernels: 1 float16, 2 bfloat16,
// + 4 channels-last.
template <typename OT, bool NHWC>
constexpr int out_kind() {
  return (std::is_same_v<OT, _Float16> ? 1 : 0) | (std::is_same_v<OT, __bf16> ? 2 : 0) | (NHWC ? 4 : 0);
}

}  // namespace dxr
