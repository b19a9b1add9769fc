// Fused SepConvGRU inference forward (include/dexiraft_gru.h; reference
// core/update.py:33-60): 1x5 then 5x1 gated convolutions on the matrix cores,
// 16-bit operands, float32 accumulation and state.  Linked into its own shared
// object, libdexiraft_gru.so (build.py), not into libdexiraft_corr.so.
//
// Five launches per call:
//   pack    h, x NCHW (f32 / f16 / bf16, read in place) -> h32, hc, xc NHWC
//   ZR(0)   z = sigmoid(convz1 [hc | xc]), rh = rne_c(sigmoid(convr1 [hc | xc]) * h32)
//   QH(0)   h32 <- (1 - z) h32 + z tanh(convq1 [rh | xc]), hc <- rne_c(h32)
//   ZR(1), QH(1)  the same along H with convz2 / convr2 / convq2; QH(1) writes the
//           NCHW output instead of h32 / hc
//
// A gate launch is an implicit GEMM.  A line is an image row (axis 0) or an image
// column (axis 1); a workgroup owns NPB * 32 consecutive pixels of one line and
// every output row (2 Ch for ZR, Ch for QH).  It stages those pixels plus a
// two-pixel halo, all Ch + Cx channels, once in LDS ([pixel][channel], zeros past
// the line's ends: the padding of the convolution), and then runs
// K = 5 * (Ch + Cx) as 5 taps x (Ch + Cx) / 16 steps of v_mfma_f32_32x32x16 with
// the LDS row offset shifted by the tap.  Wave w owns output rows 32w .. 32w+31
// as the A operand, read straight from L2 in operand order
// (dxg_sepconv_pack_weights: 1 KB per wave and step as two contiguous 512-byte
// runs, one per k half, 16 * rows bytes apart, four steps ahead); the B operand is 8 consecutive channels of pixel (lane & 31) + tap,
// one ds_read_b128 (row pitch 2 (Ch + Cx) + 16 bytes: conflict-free).  The
// accumulator has the pixel on the lane and four consecutive output channels in
// each register quad, so the NHWC gate stores are 16- and 8-byte vectors.
#include "dexiraft_gru.h"
#include "dxr_common.h"
#include "mfma_operands.h"

namespace {

using dxr::f32x16_t;
using dxr::bf16x8_t;
using dxr::f16x8_t;

constexpr int64_t G_MAX_HW = 1LL << 22;
constexpr int64_t G_MAX_N = 65535;          // grid.y limit
constexpr int G_BLK = 32;                   // pixels per MFMA column block
constexpr int G_HALO = 2;
constexpr int G_TAPS = 5;
constexpr int G_PF = 4;                     // weight fragments in flight per wave
constexpr int G_PAD = 16;                   // bytes added to an LDS pixel row
// 64-pixel workgroups once a launch has more 32-pixel tiles than this (launch_gate).
// scripts/ab_gru_tiles.py builds with other values to time one form against the
// other (profiles/r22/gru/ab_tiles_bfloat16.jsonl: the 32-pixel form is faster at
// 552 / 744 tiles, the 64-pixel one at 880 / 1024); the values do not depend on it.
#ifndef DXG_TILE64_ABOVE_WGS
#define DXG_TILE64_ABOVE_WGS 768
#endif


// DXR_OK, DXR_EINVAL or DXR_EUNSUPPORTED for the sizes alone.
inline int geometry_status(int64_t N, int64_t H, int64_t W, int64_t Ch, int64_t Cx) {
  if (N < 0 || H < 1 || W < 1 || Ch < 1 || Cx < 1) return DXR_EINVAL;
  if (Ch % 16 || Ch > 128 || Cx % 16 || Cx > 256) return DXR_EUNSUPPORTED;
  if (N > G_MAX_N || H > G_MAX_HW || W > G_MAX_HW || H * W > G_MAX_HW) return DXR_EUNSUPPORTED;
  return DXR_OK;
}
inline bool dtype_ok(int d) { return d == DXG_F32 || d == DXG_F16 || d == DXG_BF16; }
inline bool compute_ok(int d) { return d == DXG_F16 || d == DXG_BF16; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int64_t q_rows(int64_t Ch) { return (Ch + 31) / 32 * 32; }

// The workspace (dexiraft_gru.h): h32, hc, xc, z, rh.
struct Workspace {
  float* h32;
  uint16_t* hc;
  uint16_t* xc;
  float* z;
  uint16_t* rh;
};
inline Workspace carve(void* ws, int64_t P, int64_t Ch, int64_t Cx) {
  char* p = static_cast<char*>(ws);
  Workspace w;
  w.h32 = reinterpret_cast<float*>(p);
  p += 4 * P * Ch;
  w.hc = reinterpret_cast<uint16_t*>(p);
  p += 2 * P * Ch;
  w.xc = reinterpret_cast<uint16_t*>(p);
  p += 2 * P * Cx;
  w.z = reinterpret_cast<float*>(p);
  p += 4 * P * Ch;
  w.rh = reinterpret_cast<uint16_t*>(p);
  return w;
}

// The packed weights of one axis: ZR fragments, QH fragments, ZR biases, QH biases.
struct Packed {
  const uint4* zr;
  const uint4* q;
  const float* bias_zr;
  const float* bias_q;
};
inline Packed carve_packed(const void* packed, int64_t Ch, int64_t Cx) {
  const int64_t steps = G_TAPS * (Ch + Cx) / 16;
  const uint4* p = static_cast<const uint4*>(packed);
  Packed k;
  k.zr = p;
  k.q = p + steps * 2 * (2 * Ch);
  const float* b = reinterpret_cast<const float*>(k.q + steps * 2 * q_rows(Ch));
  k.bias_zr = b;
  k.bias_q = b + 2 * Ch;
  return k;
}

template <bool BF>
__device__ __forceinline__ uint16_t rne_c(float v) {
  if constexpr (BF) return dxr::f32_to_bf16(v);
  else return dxr::f32_to_f16_bits(v);
}

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(_Float16 v) { return (float)v; }
__device__ __forceinline__ float widen(uint16_t v) { return dxr::bf16_to_f32(v); }

__device__ __forceinline__ void narrow_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void narrow_store(_Float16* p, float v) {
  *reinterpret_cast<uint16_t*>(p) = dxr::f32_to_f16_bits(v);
}
__device__ __forceinline__ void narrow_store(uint16_t* p, float v) { *p = dxr::f32_to_bf16(v); }

// ---------------------------------------------------------------------------
// Weights: [Ch, C, 5] f32 x 3 -> operand order.  One thread per 8-channel fragment.
// ---------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(256) void pack_weights_kernel(
    const float* __restrict__ wz, const float* __restrict__ wr, const float* __restrict__ wq,
    const float* __restrict__ bz, const float* __restrict__ br, const float* __restrict__ bq,
    uint4* __restrict__ zr, uint4* __restrict__ q, float* __restrict__ bias_zr,
    float* __restrict__ bias_q, int Ch, int C) {
  const int ks_n = C / 16, steps = G_TAPS * ks_n;
  const int rz = 2 * Ch, rq = (Ch + 31) / 32 * 32;
  const int64_t n_zr = (int64_t)steps * 2 * rz, n_q = (int64_t)steps * 2 * rq;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < rz) bias_zr[i] = i < Ch ? bz[i] : br[i - Ch];
  if (i < rq) bias_q[i] = i < Ch ? bq[i] : 0.0f;
  if (i >= n_zr + n_q) return;
  const bool is_q = i >= n_zr;
  const int64_t e = is_q ? i - n_zr : i;
  const int rows = is_q ? rq : rz;
  const int row = (int)(e % rows);
  const int skh = (int)(e / rows), kh = skh & 1, s = skh >> 1;
  const int t = s / ks_n, ks = s - t * ks_n;
  const float* w = nullptr;   // the row's [C, 5] weights; null: a zero row
  if (is_q) {
    if (row < Ch) w = wq + (int64_t)row * C * G_TAPS;
  } else {
    w = row < Ch ? wz + (int64_t)row * C * G_TAPS : wr + (int64_t)(row - Ch) * C * G_TAPS;
  }
  uint32_t v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ci = ks * 16 + kh * 8 + 2 * k;
    const float a = w ? w[(int64_t)ci * G_TAPS + t] : 0.0f;
    const float b = w ? w[(int64_t)(ci + 1) * G_TAPS + t] : 0.0f;
    v[k] = (uint32_t)rne_c<BF>(a) | ((uint32_t)rne_c<BF>(b) << 16);
  }
  (is_q ? q : zr)[e] = make_uint4(v[0], v[1], v[2], v[3]);
}

// ---------------------------------------------------------------------------
// Inputs: NCHW -> NHWC.  A workgroup moves 16 channels x 64 pixels of one item
// through LDS: loads coalesced along pixels, stores along channels.
// blockIdx.y < Ch / 16: a tile of h (h32 and hc), else a tile of x (xc).
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void load_tile(const T* __restrict__ src, int64_t hw, int p0, int tid,
                                          float (*tile)[65]) {
  const int px = tid & 63, c4 = tid >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c4 + 4 * k;
    tile[c][px] = p0 + px < hw ? widen(src[(int64_t)c * hw + p0 + px]) : 0.0f;
  }
}

template <bool BF>
__global__ __launch_bounds__(256) void pack_inputs_kernel(
    const void* __restrict__ h, int h_dtype, const void* __restrict__ x, int x_dtype,
    float* __restrict__ h32, uint16_t* __restrict__ hc, uint16_t* __restrict__ xc, int hw, int Ch,
    int Cx) {
  __shared__ float tile[16][65];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int p0 = blockIdx.x * 64;
  const bool is_h = (int)blockIdx.y < Ch / 16;
  const int c0 = (is_h ? blockIdx.y : blockIdx.y - Ch / 16) * 16;
  const int Cs = is_h ? Ch : Cx;
  const int dtype = is_h ? h_dtype : x_dtype;
  const int64_t off = ((int64_t)n * Cs + c0) * hw;
  const void* src = is_h ? h : x;
  if (dtype == DXG_F32) load_tile(static_cast<const float*>(src) + off, hw, p0, tid, tile);
  else if (dtype == DXG_F16) load_tile(static_cast<const _Float16*>(src) + off, hw, p0, tid, tile);
  else load_tile(static_cast<const uint16_t*>(src) + off, hw, p0, tid, tile);
  __syncthreads();
  const int c = tid & 15, p4 = tid >> 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = p4 + 16 * k;
    if (p0 + px >= hw) continue;
    const float v = tile[c][px];
    const int64_t o = ((int64_t)n * hw + p0 + px) * Cs + c0 + c;
    if (is_h) {
      h32[o] = v;
      hc[o] = rne_c<BF>(v);
    } else {
      xc[o] = rne_c<BF>(v);
    }
  }
}

// ---------------------------------------------------------------------------
// The gate stages.
// ---------------------------------------------------------------------------
struct GateGeom {
  int H, W, Ch, Cx;
  int L;         // pixels of a line: W (axis 0) or H (axis 1)
  int segs;      // workgroups per line
  int pstride;   // pixels between neighbours on a line: 1 or W
  int vertical;
};

enum { MODE_ZR = 0, MODE_QH_STATE = 1, MODE_QH_OUT = 2 };

template <bool BF>
__device__ __forceinline__ f32x16_t mfma(const uint4& a, const uint4& b, const f32x16_t& acc) {
  if constexpr (BF)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                   __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a),
                                                  __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

// src_a: hc (ZR) or rh (QH).  dst16: rh (ZR) or hc (QH_STATE).  rows: 2 Ch (ZR) or
// Ch rounded up to 32 (QH); the workgroup has rows / 32 waves.
template <bool BF, int NPB, int MODE, typename OT>
__global__ __launch_bounds__(512) void gate_kernel(
    const uint4* __restrict__ wpk, const float* __restrict__ bias,
    const uint16_t* __restrict__ src_a, const uint16_t* __restrict__ xc, float* __restrict__ h32,
    float* __restrict__ z, uint16_t* __restrict__ dst16, OT* __restrict__ out, GateGeom g, int rows) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NPIX = NPB * G_BLK + 2 * G_HALO;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int Ch = g.Ch, Cx = g.Cx, C = Ch + Cx;
  const int pitch = 2 * C + G_PAD;
  const int seg = blockIdx.x % g.segs, line = blockIdx.x / g.segs, n = blockIdx.y;
  const int p0 = seg * (NPB * G_BLK);
  const int64_t line_base =
      g.vertical ? (int64_t)n * g.H * g.W + line : ((int64_t)n * g.H + line) * g.W;

  // ---- stage [NPIX][C] of the line, zeros outside it
  {
    const int cpp = C / 8, cph = Ch / 8;   // 16-byte chunks per pixel, of them from src_a
    for (int i = tid; i < NPIX * cpp; i += nthreads) {
      const int pl = i / cpp, ch = i - pl * cpp;
      const int p = p0 + pl - G_HALO;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (p >= 0 && p < g.L) {
        const int64_t pix = line_base + (int64_t)p * g.pstride;
        v = ch < cph ? reinterpret_cast<const uint4*>(src_a + pix * Ch)[ch]
                     : reinterpret_cast<const uint4*>(xc + pix * Cx)[ch - cph];
      }
      *reinterpret_cast<uint4*>(lds + pl * pitch + ch * 16) = v;
    }
  }
  __syncthreads();

  // ---- K loop: 5 taps x C / 16 steps, weights G_PF steps ahead
  const int lane = tid & 63, ob = tid >> 6, j = lane & 31, kh = lane >> 5;
  const int ks_n = C / 16, steps = G_TAPS * ks_n;
  const int64_t wstep = 2 * (int64_t)rows;                       // uint4 per step
  const uint4* wp = wpk + (int64_t)kh * rows + ob * G_BLK + j;   // + s * wstep
  f32x16_t acc[NPB];
#pragma unroll
  for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[pb][r] = 0.0f;
  uint4 wb[G_PF];
#pragma unroll
  for (int sl = 0; sl < G_PF; ++sl) wb[sl] = wp[min(sl, steps - 1) * wstep];
  int ks = 0;
  int boff = j * pitch + kh * 16;   // LDS byte offset of this lane's fragment at step s
  auto kstep = [&](int s, int sl) {
    const uint4 a = wb[sl];
    wb[sl] = wp[min(s + G_PF, steps - 1) * wstep];
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const uint4 b = *reinterpret_cast<const uint4*>(lds + boff + pb * G_BLK * pitch);
      acc[pb] = mfma<BF>(a, b, acc[pb]);
    }
    boff += 32;
    if (++ks == ks_n) {   // next tap: one pixel further, back to channel 0
      ks = 0;
      boff += pitch - 32 * ks_n;
    }
  };
  const int nfull = steps / G_PF * G_PF;
#pragma unroll 1
  for (int s0 = 0; s0 < nfull; s0 += G_PF) {
#pragma unroll
    for (int sl = 0; sl < G_PF; ++sl) kstep(s0 + sl, sl);
  }
#pragma unroll
  for (int sl = 0; sl < G_PF; ++sl)
    if (nfull + sl < steps) kstep(nfull + sl, sl);

  // ---- epilogue: register quad q4 holds rows 8 q4 + 4 kh .. + 3 of pixel j
#pragma unroll
  for (int pb = 0; pb < NPB; ++pb) {
    const int p = p0 + pb * G_BLK + j;
    if (p >= g.L) continue;
    const int64_t pix = line_base + (int64_t)p * g.pstride;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int o = ob * G_BLK + 8 * q4 + 4 * kh;
      float pre[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pre[e] = acc[pb][4 * q4 + e] + bias[o + e];
      if constexpr (MODE == MODE_ZR) {
        if (o < Ch) {
          *reinterpret_cast<float4*>(z + pix * Ch + o) =
              make_float4(sigmoidf(pre[0]), sigmoidf(pre[1]), sigmoidf(pre[2]), sigmoidf(pre[3]));
        } else {
          const int c = o - Ch;
          const float4 hv = *reinterpret_cast<const float4*>(h32 + pix * Ch + c);
          const float hs[4] = {hv.x, hv.y, hv.z, hv.w};
          uint16_t v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rne_c<BF>(sigmoidf(pre[e]) * hs[e]);
          *reinterpret_cast<uint2*>(dst16 + pix * Ch + c) =
              make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
        }
      } else {
        if (o >= Ch) continue;   // the zero rows that pad Ch to a multiple of 32
        const float4 hv = *reinterpret_cast<const float4*>(h32 + pix * Ch + o);
        const float4 zv = *reinterpret_cast<const float4*>(z + pix * Ch + o);
        const float hs[4] = {hv.x, hv.y, hv.z, hv.w}, zs[4] = {zv.x, zv.y, zv.z, zv.w};
        float hn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) hn[e] = (1.0f - zs[e]) * hs[e] + zs[e] * tanhf(pre[e]);
        if constexpr (MODE == MODE_QH_STATE) {
          *reinterpret_cast<float4*>(h32 + pix * Ch + o) = make_float4(hn[0], hn[1], hn[2], hn[3]);
          uint16_t v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rne_c<BF>(hn[e]);
          *reinterpret_cast<uint2*>(dst16 + pix * Ch + o) =
              make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
        } else {
          const int64_t hw = (int64_t)g.H * g.W;
          const int64_t q = g.vertical ? (int64_t)p * g.W + line : (int64_t)line * g.W + p;
#pragma unroll
          for (int e = 0; e < 4; ++e) narrow_store(out + ((int64_t)n * Ch + o + e) * hw + q, hn[e]);
        }
      }
    }
  }
}

template <bool BF, int NPB, int MODE, typename OT>
int launch_gate_as(const uint4* wpk, const float* bias, const uint16_t* src_a, const Workspace& w,
                   uint16_t* dst16, void* out, GateGeom g, int rows, int64_t N,
                   hipStream_t stream) {
  g.segs = (g.L + NPB * G_BLK - 1) / (NPB * G_BLK);
  const int64_t lines = g.vertical ? g.W : g.H;
  const dim3 grid((unsigned)(lines * g.segs), (unsigned)N);
  const size_t lds = (size_t)(NPB * G_BLK + 2 * G_HALO) * (2 * (g.Ch + g.Cx) + G_PAD);
  gate_kernel<BF, NPB, MODE, OT><<<grid, dim3(64 * (rows / G_BLK)), lds, stream>>>(
      wpk, bias, src_a, w.xc, w.h32, w.z, dst16, static_cast<OT*>(out), g, rows);
  return dxr::launch_status();
}

// 32-pixel workgroups while they do not fill the device's 256 CUs three times over,
// 64-pixel ones (each weight fragment used twice) beyond that.  The tile does not
// change any value: a pixel's sums have the same order in both.
template <bool BF, int MODE, typename OT>
int launch_gate(const uint4* wpk, const float* bias, const uint16_t* src_a, const Workspace& w,
                uint16_t* dst16, void* out, const GateGeom& g, int rows, int64_t N,
                hipStream_t stream) {
  const int64_t lines = g.vertical ? g.W : g.H;
  const int64_t wgs32 = N * lines * ((g.L + G_BLK - 1) / G_BLK);
  if (wgs32 <= DXG_TILE64_ABOVE_WGS || g.L <= G_BLK)
    return launch_gate_as<BF, 1, MODE, OT>(wpk, bias, src_a, w, dst16, out, g, rows, N, stream);
  return launch_gate_as<BF, 2, MODE, OT>(wpk, bias, src_a, w, dst16, out, g, rows, N, stream);
}

inline GateGeom make_geom(int axis, int64_t H, int64_t W, int64_t Ch, int64_t Cx) {
  GateGeom g;
  g.H = (int)H;
  g.W = (int)W;
  g.Ch = (int)Ch;
  g.Cx = (int)Cx;
  g.vertical = axis;
  g.L = axis ? (int)H : (int)W;
  g.pstride = axis ? (int)W : 1;
  g.segs = 0;
  return g;
}

// Everything the stage entry points share: sizes, dtypes, the workspace.
inline int check_stage(int64_t N, int64_t H, int64_t W, int64_t Ch, int64_t Cx, int compute_dtype,
                       const void* workspace, int64_t workspace_bytes) {
  const int st = geometry_status(N, H, W, Ch, Cx);
  if (st != DXR_OK) return st;
  if (!compute_ok(compute_dtype)) return DXR_EINVAL;
  if (!workspace || !aligned16(workspace)) return DXR_EINVAL;
  if (workspace_bytes < dxg_sepconv_workspace_bytes(N, H, W, Ch, Cx)) return DXR_EINVAL;
  return DXR_OK;
}

template <bool BF>
int run_zr(const void* packed, int axis, int64_t N, int64_t H, int64_t W, int64_t Ch, int64_t Cx,
           void* workspace, hipStream_t stream) {
  const Workspace w = carve(workspace, N * H * W, Ch, Cx);
  const Packed k = carve_packed(packed, Ch, Cx);
  return launch_gate<BF, MODE_ZR, float>(k.zr, k.bias_zr, w.hc, w, w.rh, nullptr,
                                         make_geom(axis, H, W, Ch, Cx), (int)(2 * Ch), N, stream);
}

template <bool BF>
int run_qh(const void* packed, int axis, int64_t N, int64_t H, int64_t W, int64_t Ch, int64_t Cx,
           void* out, int out_dtype, void* workspace, hipStream_t stream) {
  const Workspace w = carve(workspace, N * H * W, Ch, Cx);
  const Packed k = carve_packed(packed, Ch, Cx);
  const GateGeom g = make_geom(axis, H, W, Ch, Cx);
  const int rows = (int)q_rows(Ch);
  if (!out)
    return launch_gate<BF, MODE_QH_STATE, float>(k.q, k.bias_q, w.rh, w, w.hc, nullptr, g, rows, N,
                                                 stream);
  switch (out_dtype) {
    case DXG_F32:
      return launch_gate<BF, MODE_QH_OUT, float>(k.q, k.bias_q, w.rh, w, nullptr, out, g, rows, N,
                                                 stream);
    case DXG_F16:
      return launch_gate<BF, MODE_QH_OUT, _Float16>(k.q, k.bias_q, w.rh, w, nullptr, out, g, rows, N,
                                                    stream);
    default:
      return launch_gate<BF, MODE_QH_OUT, uint16_t>(k.q, k.bias_q, w.rh, w, nullptr, out, g, rows, N,
                                                    stream);
  }
}

}  // namespace

extern "C" int dxg_abi_version(void) { return DXG_ABI_VERSION; }

extern "C" int64_t dxg_sepconv_packed_weight_bytes(int64_t Ch, int64_t Cx) {
  if (geometry_status(0, 1, 1, Ch, Cx) != DXR_OK) return -1;
  const int64_t rows = 2 * Ch + q_rows(Ch);
  return (2 * G_TAPS * (Ch + Cx) * rows + 4 * rows + 15) / 16 * 16;
}

extern "C" int dxg_sepconv_pack_weights(const float* wz, const float* wr, const float* wq,
                                        const float* bz, const float* br, const float* bq,
                                        int64_t Ch, int64_t Cx, int compute_dtype, void* packed,
                                        int64_t packed_bytes, hipStream_t stream) {
  const int st = geometry_status(0, 1, 1, Ch, Cx);
  if (st != DXR_OK) return st;
  if (!compute_ok(compute_dtype)) return DXR_EINVAL;
  if (!wz || !wr || !wq || !bz || !br || !bq) return DXR_EINVAL;
  if (!packed || !aligned16(packed)) return DXR_EINVAL;
  if (packed_bytes < dxg_sepconv_packed_weight_bytes(Ch, Cx)) return DXR_EINVAL;
  const Packed k = carve_packed(packed, Ch, Cx);
  const int64_t frags = G_TAPS * (Ch + Cx) / 16 * 2 * (2 * Ch + q_rows(Ch));
  const dim3 grid((unsigned)((frags + 255) / 256));
  uint4* zr = const_cast<uint4*>(k.zr);
  uint4* q = const_cast<uint4*>(k.q);
  float* b_zr = const_cast<float*>(k.bias_zr);
  float* b_q = const_cast<float*>(k.bias_q);
  if (compute_dtype == DXG_BF16)
    pack_weights_kernel<true><<<grid, dim3(256), 0, stream>>>(wz, wr, wq, bz, br, bq, zr, q, b_zr,
                                                             b_q, (int)Ch, (int)(Ch + Cx));
  else
    pack_weights_kernel<false><<<grid, dim3(256), 0, stream>>>(wz, wr, wq, bz, br, bq, zr, q, b_zr,
                                                              b_q, (int)Ch, (int)(Ch + Cx));
  return dxr::launch_status();
}

extern "C" int64_t dxg_sepconv_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t Ch,
                                               int64_t Cx) {
  if (geometry_status(N, H, W, Ch, Cx) != DXR_OK) return -1;
  return N * H * W * (12 * Ch + 2 * Cx);
}

extern "C" int dxg_sepconv_pack_inputs(const void* h, int h_dtype, const void* x, int x_dtype,
                                       int64_t N, int64_t H, int64_t W, int64_t Ch, int64_t Cx,
                                       int compute_dtype, void* workspace, int64_t workspace_bytes,
                                       hipStream_t stream) {
  if (N == 0) return DXR_OK;
  const int st = check_stage(N, H, W, Ch, Cx, compute_dtype, workspace, workspace_bytes);
  if (st != DXR_OK) return st;
  if (!dtype_ok(h_dtype) || !dtype_ok(x_dtype)) return DXR_EINVAL;
  if (!h || !x) return DXR_EINVAL;
  const Workspace w = carve(workspace, N * H * W, Ch, Cx);
  const dim3 grid((unsigned)((H * W + 63) / 64), (unsigned)((Ch + Cx) / 16), (unsigned)N);
  if (compute_dtype == DXG_BF16)
    pack_inputs_kernel<true><<<grid, dim3(256), 0, stream>>>(h, h_dtype, x, x_dtype, w.h32, w.hc, w.xc,
                                                            (int)(H * W), (int)Ch, (int)Cx);
  else
    pack_inputs_kernel<false><<<grid, dim3(256), 0, stream>>>(h, h_dtype, x, x_dtype, w.h32, w.hc,
                                                             w.xc, (int)(H * W), (int)Ch, (int)Cx);
  return dxr::launch_status();
}

extern "C" int dxg_sepconv_gate_zr(const void* packed, int axis, int64_t N, int64_t H, int64_t W,
                                   int64_t Ch, int64_t Cx, int compute_dtype, void* workspace,
                                   int64_t workspace_bytes, hipStream_t stream) {
  if (N == 0) return DXR_OK;
  const int st = check_stage(N, H, W, Ch, Cx, compute_dtype, workspace, workspace_bytes);
  if (st != DXR_OK) return st;
  if (axis != 0 && axis != 1) return DXR_EINVAL;
  if (!packed || !aligned16(packed)) return DXR_EINVAL;
  return compute_dtype == DXG_BF16 ? run_zr<true>(packed, axis, N, H, W, Ch, Cx, workspace, stream)
                                   : run_zr<false>(packed, axis, N, H, W, Ch, Cx, workspace, stream);
}

extern "C" int dxg_sepconv_gate_qh(const void* packed, int axis, int64_t N, int64_t H, int64_t W,
                                   int64_t Ch, int64_t Cx, int compute_dtype, void* out,
                                   int out_dtype, void* workspace, int64_t workspace_bytes,
                                   hipStream_t stream) {
  if (N == 0) return DXR_OK;
  const int st = check_stage(N, H, W, Ch, Cx, compute_dtype, workspace, workspace_bytes);
  if (st != DXR_OK) return st;
  if (axis != 0 && axis != 1) return DXR_EINVAL;
  if (out && !dtype_ok(out_dtype)) return DXR_EINVAL;
  if (!packed || !aligned16(packed)) return DXR_EINVAL;
  return compute_dtype == DXG_BF16
             ? run_qh<true>(packed, axis, N, H, W, Ch, Cx, out, out_dtype, workspace, stream)
             : run_qh<false>(packed, axis, N, H, W, Ch, Cx, out, out_dtype, workspace, stream);
}

extern "C" int dxg_sepconv_gru(const void* h, int h_dtype, const void* x, int x_dtype,
                               const void* packed_h, const void* packed_v, int64_t N, int64_t H,
                               int64_t W, int64_t Ch, int64_t Cx, int compute_dtype, void* out,
                               int out_dtype, void* workspace, int64_t workspace_bytes,
                               hipStream_t stream) {
  if (N == 0) return DXR_OK;
  int st = check_stage(N, H, W, Ch, Cx, compute_dtype, workspace, workspace_bytes);
  if (st != DXR_OK) return st;
  if (!dtype_ok(h_dtype) || !dtype_ok(x_dtype) || !dtype_ok(out_dtype)) return DXR_EINVAL;
  if (!h || !x || !out) return DXR_EINVAL;
  if (!packed_h || !packed_v || !aligned16(packed_h) || !aligned16(packed_v)) return DXR_EINVAL;
  st = dxg_sepconv_pack_inputs(h, h_dtype, x, x_dtype, N, H, W, Ch, Cx, compute_dtype, workspace,
                               workspace_bytes, stream);
  if (st != DXR_OK) return st;
  st = dxg_sepconv_gate_zr(packed_h, 0, N, H, W, Ch, Cx, compute_dtype, workspace, workspace_bytes,
                           stream);
  if (st != DXR_OK) return st;
  st = dxg_sepconv_gate_qh(packed_h, 0, N, H, W, Ch, Cx, compute_dtype, nullptr, DXG_F32, workspace,
                           workspace_bytes, stream);
  if (st != DXR_OK) return st;
  st = dxg_sepconv_gate_zr(packed_v, 1, N, H, W, Ch, Cx, compute_dtype, workspace, workspace_bytes,
                           stream);
  if (st != DXR_OK) return st;
  return dxg_sepconv_gate_qh(packed_v, 1, N, H, W, Ch, Cx, compute_dtype, out, out_dtype, workspace,
                             workspace_bytes, stream);
}
