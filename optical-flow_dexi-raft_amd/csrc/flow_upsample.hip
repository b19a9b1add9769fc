// Convex 8x flow upsampling, forward and backward (include/dexiraft_upsample.h;
// reference core/raft.py:87-98): a softmax over the 9 taps of every fine pixel
// and a convex combination of the 3x3 neighbourhood of 8 * flow.
//
// Mapping (both kernels).  A workgroup is 8 waves over 64 consecutive coarse
// pixels of one item: lanes run along the flat pixel index p = h*W + w, wave i
// takes sub-row i of the 8x8 cell, and every thread loops j = 0..7.  A mask plane
// [H, W] is contiguous in p, so each of a thread's 72 mask loads is one
// coalesced wave-wide row whatever W is, and a thread's 8 outputs per channel
// (out[n, c, 8h+i, 8w .. 8w+7]) are contiguous, adjacent lanes adjacent in
// memory.  The 2 x 9 neighbourhood of 8 * flow sits in registers.
//
// Forward: one launch.  Backward: the main kernel recomputes the softmax, writes
// grad_mask and sums T[n, c, k, p] = sum_{i,j} w_k g_c (j in registers, then the
// 8 waves in ascending i through LDS) into the workspace; a gather launch adds
// the 9 shifted T planes into grad_flow.  No atomics: every sum has a fixed order.
//
// The arithmetic is spelled out (fmaf where a fused multiply-add is meant,
// contraction off elsewhere), so the three mask types run the same float32
// operations and the backward's weights equal the forward's.
#include "dexiraft_upsample.h"
#include "dxr_common.h"

namespace {

constexpr int UP_LANES = 64;                  // coarse pixels per workgroup
constexpr int UP_SUB = 8;                     // sub-rows i = waves per workgroup
constexpr int UP_THREADS = UP_LANES * UP_SUB;
constexpr int UP_GATHER = 256;                // threads per workgroup of the gather
constexpr int64_t UP_MAX_HW = 1LL << 22;
constexpr int64_t UP_MAX_N = 65535;           // grid.y / grid.z limit

inline bool geometry_ok(int64_t N, int64_t H, int64_t W) {
  return N >= 0 && N <= UP_MAX_N && H >= 1 && W >= 1 && H <= UP_MAX_HW && W <= UP_MAX_HW &&
         H * W <= UP_MAX_HW;
}

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(_Float16 v) { return (float)v; }
__device__ __forceinline__ float widen(uint16_t v) { return dxr::bf16_to_f32(v); }

__device__ __forceinline__ void narrow_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void narrow_store(_Float16* p, float v) {
  *reinterpret_cast<uint16_t*>(p) = dxr::f32_to_f16_bits(v);
}
__device__ __forceinline__ void narrow_store(uint16_t* p, float v) { *p = dxr::f32_to_bf16(v); }

// 8 * flow at the 9 taps of coarse pixel (h, w); 0 outside the map.
__device__ __forceinline__ void load_taps(const float* __restrict__ flow, int H, int W, int h, int w,
                                          float (&f)[2][9]) {
  const int hw = H * W;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int hh = h + k / 3 - 1, ww = w + k % 3 - 1;
    const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
    const int q = in ? hh * W + ww : 0;
    const float f0 = flow[q], f1 = flow[hw + q];
    f[0][k] = in ? 8.0f * f0 : 0.0f;
    f[1][k] = in ? 8.0f * f1 : 0.0f;
  }
}

// e_k = exp(x_k - max) for the 9 taps at mp[k * tap_stride]; returns 1 / sum_k e_k.
template <typename T>
__device__ __forceinline__ float softmax_taps(const T* __restrict__ mp, int64_t tap_stride,
                                              float (&e)[9]) {
#pragma clang fp contract(off)
  float x[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) x[k] = widen(mp[k * tap_stride]);
  float m = x[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) m = fmaxf(m, x[k]);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    e[k] = expf(x[k] - m);
    s = s + e[k];
  }
  return 1.0f / s;
}

// 8 contiguous floats; 16-byte accesses when the caller's base pointer allows them
// (the offsets are multiples of 32 bytes).
__device__ __forceinline__ void store8(float* p, const float (&v)[8], bool vec) {
  if (vec) {
    reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = v[j];
  }
}
__device__ __forceinline__ void load8(const float* __restrict__ p, float (&v)[8], bool vec) {
  if (vec) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j];
  }
}

template <typename T>
__global__ __launch_bounds__(UP_THREADS) void convex_upsample_kernel(
    const T* __restrict__ mask, const float* __restrict__ flow, float* __restrict__ out, int H, int W,
    bool vec) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, i = threadIdx.y, n = blockIdx.y;
  const int hw = H * W;
  const int p = blockIdx.x * UP_LANES + lane;
  if (p >= hw) return;
  const int h = p / W, w = p - h * W;
  float f[2][9];
  load_taps(flow + (int64_t)n * 2 * hw, H, W, h, w, f);
  const T* mp = mask + ((int64_t)n * 576 + 8 * i) * hw + p;   // channel 64k + 8i + j: + (64k + j) * hw
  float o[2][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float e[9];
    const float r = softmax_taps(mp + (int64_t)j * hw, (int64_t)64 * hw, e);
    float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      a0 = fmaf(e[k], f[0][k], a0);
      a1 = fmaf(e[k], f[1][k], a1);
    }
    o[0][j] = a0 * r;
    o[1][j] = a1 * r;
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float* op = out + (((int64_t)n * 2 + c) * 8 * H + 8 * h + i) * (8 * (int64_t)W) + 8 * w;
    store8(op, o[c], vec);
  }
}

// MASK: write grad_mask.  FLOW: sum T into `tws` ([N, 2, 9, H*W] floats).
template <typename T, bool MASK, bool FLOW>
__global__ __launch_bounds__(UP_THREADS) void convex_upsample_backward_kernel(
    const float* __restrict__ gout, const T* __restrict__ mask, const float* __restrict__ flow,
    T* __restrict__ gmask, float* __restrict__ tws, int H, int W, bool vec) {
#pragma clang fp contract(off)
  __shared__ float red[FLOW ? UP_SUB * 18 * UP_LANES : 1];
  const int lane = threadIdx.x, i = threadIdx.y, n = blockIdx.y;
  const int hw = H * W;
  const int p = blockIdx.x * UP_LANES + lane;
  float t[18];
#pragma unroll
  for (int q = 0; q < 18; ++q) t[q] = 0.0f;
  if (p < hw) {
    const int h = p / W, w = p - h * W;
    float f[2][9];
    if (MASK) load_taps(flow + (int64_t)n * 2 * hw, H, W, h, w, f);
    float g[2][8];
#pragma unroll
    for (int c = 0; c < 2; ++c)
      load8(gout + (((int64_t)n * 2 + c) * 8 * H + 8 * h + i) * (8 * (int64_t)W) + 8 * w, g[c], vec);
    const int64_t moff = ((int64_t)n * 576 + 8 * i) * hw + p;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float e[9];
      const float r = softmax_taps(mask + moff + (int64_t)j * hw, (int64_t)64 * hw, e);
      float wk[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) wk[k] = e[k] * r;
      if (MASK) {
        float a[9], dot = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          a[k] = fmaf(g[0][j], f[0][k], g[1][j] * f[1][k]);
          dot = fmaf(wk[k], a[k], dot);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k)
          narrow_store(gmask + moff + (int64_t)(64 * k + j) * hw, wk[k] * (a[k] - dot));
      }
      if (FLOW) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          t[k] = fmaf(wk[k], g[0][j], t[k]);
          t[9 + k] = fmaf(wk[k], g[1][j], t[9 + k]);
        }
      }
    }
  }
  if (FLOW) {
    // red[i][q][lane]; lanes past the map hold zeros and are not written out
#pragma unroll
    for (int q = 0; q < 18; ++q) red[(i * 18 + q) * UP_LANES + lane] = t[q];
    __syncthreads();
    for (int o = i * UP_LANES + lane; o < 18 * UP_LANES; o += UP_THREADS) {
      const int q = o / UP_LANES, l = o % UP_LANES;
      float s = 0.0f;
#pragma unroll
      for (int ii = 0; ii < UP_SUB; ++ii) s = s + red[(ii * 18 + q) * UP_LANES + l];
      const int pp = blockIdx.x * UP_LANES + l;
      if (pp < hw) tws[((int64_t)n * 18 + q) * hw + pp] = s;
    }
  }
}

// grad_flow[n, c, h', w'] = 8 * sum_k T[n, c, k, h' - (k/3 - 1), w' - (k%3 - 1)], k ascending.
__global__ __launch_bounds__(UP_GATHER) void convex_upsample_gather_kernel(
    const float* __restrict__ tws, float* __restrict__ gflow, int H, int W) {
#pragma clang fp contract(off)
  const int hw = H * W;
  const int p = blockIdx.x * UP_GATHER + threadIdx.x, c = blockIdx.y, n = blockIdx.z;
  if (p >= hw) return;
  const int h = p / W, w = p - h * W;
  const float* tp = tws + ((int64_t)n * 2 + c) * 9 * hw;
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int hs = h - (k / 3 - 1), ws = w - (k % 3 - 1);
    if (hs >= 0 && hs < H && ws >= 0 && ws < W) s = s + tp[(int64_t)k * hw + hs * W + ws];
  }
  gflow[((int64_t)n * 2 + c) * hw + p] = 8.0f * s;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int launch_forward(const void* mask, const float* flow, int64_t N, int64_t H, int64_t W, float* out,
                   hipStream_t stream) {
  const dim3 grid((unsigned)((H * W + UP_LANES - 1) / UP_LANES), (unsigned)N);
  convex_upsample_kernel<T><<<grid, dim3(UP_LANES, UP_SUB), 0, stream>>>(
      static_cast<const T*>(mask), flow, out, (int)H, (int)W, aligned16(out));
  return dxr::launch_status();
}

template <typename T>
int launch_backward(const float* grad_out, const void* mask, const float* flow, int64_t N, int64_t H,
                    int64_t W, void* grad_mask, float* grad_flow, void* workspace,
                    hipStream_t stream) {
  const dim3 grid((unsigned)((H * W + UP_LANES - 1) / UP_LANES), (unsigned)N);
  const dim3 block(UP_LANES, UP_SUB);
  const T* m = static_cast<const T*>(mask);
  T* gm = static_cast<T*>(grad_mask);
  float* tws = static_cast<float*>(workspace);
  const int h = (int)H, w = (int)W;
  const bool vec = aligned16(grad_out);
  if (gm && grad_flow)
    convex_upsample_backward_kernel<T, true, true><<<grid, block, 0, stream>>>(grad_out, m, flow, gm,
                                                                              tws, h, w, vec);
  else if (gm)
    convex_upsample_backward_kernel<T, true, false><<<grid, block, 0, stream>>>(grad_out, m, flow, gm,
                                                                               nullptr, h, w, vec);
  else
    convex_upsample_backward_kernel<T, false, true><<<grid, block, 0, stream>>>(grad_out, m, flow,
                                                                               nullptr, tws, h, w, vec);
  int st = dxr::launch_status();
  if (st != DXR_OK || !grad_flow) return st;
  const dim3 ggrid((unsigned)((H * W + UP_GATHER - 1) / UP_GATHER), 2, (unsigned)N);
  convex_upsample_gather_kernel<<<ggrid, dim3(UP_GATHER), 0, stream>>>(tws, grad_flow, h, w);
  return dxr::launch_status();
}

}  // namespace

extern "C" int dxu_abi_version(void) { return DXU_ABI_VERSION; }

extern "C" int dxu_convex_upsample(const void* mask, int mask_dtype, const float* flow, int64_t N,
                                   int64_t H, int64_t W, float* out, hipStream_t stream) {
  if (N == 0) return DXR_OK;
  if (!geometry_ok(N, H, W)) return DXR_EINVAL;
  if (!mask || !flow || !out) return DXR_EINVAL;
  switch (mask_dtype) {
    case DXU_MASK_F32: return launch_forward<float>(mask, flow, N, H, W, out, stream);
    case DXU_MASK_F16: return launch_forward<_Float16>(mask, flow, N, H, W, out, stream);
    case DXU_MASK_BF16: return launch_forward<uint16_t>(mask, flow, N, H, W, out, stream);
    default: return DXR_EINVAL;
  }
}

extern "C" int64_t dxu_convex_upsample_backward_workspace_bytes(int64_t N, int64_t H, int64_t W) {
  if (!geometry_ok(N, H, W)) return -1;
  return (18 * 4 * N * H * W + 15) / 16 * 16;
}

extern "C" int dxu_convex_upsample_backward(const float* grad_out, const void* mask, int mask_dtype,
                                            const float* flow, int64_t N, int64_t H, int64_t W,
                                            void* grad_mask, float* grad_flow, void* workspace,
                                            int64_t workspace_bytes, hipStream_t stream) {
  if (N == 0) return DXR_OK;
  if (!geometry_ok(N, H, W)) return DXR_EINVAL;
  if (mask_dtype != DXU_MASK_F32 && mask_dtype != DXU_MASK_F16 && mask_dtype != DXU_MASK_BF16)
    return DXR_EINVAL;
  if (!grad_out || !mask || !flow) return DXR_EINVAL;
  if (!grad_mask && !grad_flow) return DXR_EINVAL;
  if (grad_flow) {
    if (!workspace || !aligned16(workspace)) return DXR_EINVAL;
    if (workspace_bytes < dxu_convex_upsample_backward_workspace_bytes(N, H, W)) return DXR_EINVAL;
  }
  switch (mask_dtype) {
    case DXU_MASK_F32:
      return launch_backward<float>(grad_out, mask, flow, N, H, W, grad_mask, grad_flow, workspace,
                                    stream);
    case DXU_MASK_F16:
      return launch_backward<_Float16>(grad_out, mask, flow, N, H, W, grad_mask, grad_flow, workspace,
                                       stream);
    default:
      return launch_backward<uint16_t>(grad_out, mask, flow, N, H, W, grad_mask, grad_flow, workspace,
                                       stream);
  }
}
